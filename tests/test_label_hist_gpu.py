"""-m gpu: `ops.label_pair_hist` (csrc/labelhist.hip) against torch.bincount on the host, for exact integer equality of the histogram
and the rejected counter, and the two accumulators of ape_amd/evaluation.py end to end on the tiny panoptic fixture."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

NS = (0, 1, 63, 64, 65, 4099)
OFFSETS = (0, 1, 3)
DTYPES = (torch.uint8, torch.int16, torch.int32)


def host_hist(a, b, na, nb, a_ignore=None, b_ignore=None):
    """(hist [na, nb], rejected) with torch.bincount on the host"""
    a, b = a.detach().cpu().reshape(-1).long(), b.detach().cpu().reshape(-1).long()
    if a_ignore is not None:
        a = torch.where(a == a_ignore, torch.full_like(a, na - 1), a)
    if b_ignore is not None:
        b = torch.where(b == b_ignore, torch.full_like(b, nb - 1), b)
    ok = (a >= 0) & (a < na) & (b >= 0) & (b < nb)
    return torch.bincount(a[ok] * nb + b[ok], minlength=na * nb).reshape(na, nb), int((~ok).sum())


def check(a, b, na, nb, **kw):
    from ape_amd import ops
    hist, rejected = ops.label_pair_hist(a, b, na, nb, **kw)
    want, want_rejected = host_hist(a, b, na, nb, **kw)
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (na, nb) and rejected.dtype == torch.int64
    assert torch.equal(hist.cpu(), want), (na, nb, a.numel(), int((hist.cpu() != want).sum()))
    assert int(rejected.cpu()[0]) == want_rejected
    return hist


def _dtype_for(nlabels):
    return torch.uint8 if nlabels <= 256 else torch.int16


def _random(n, nlabels, seed, dtype=None, pad=0):
    """n labels of [0, nlabels) behind `pad` leading elements of a larger buffer"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, nlabels, (n + pad,), generator=g).to(dtype or _dtype_for(nlabels)).cuda()
    return t[pad:]


def _table(name):
    """the switch point between the two paths comes from the library, not from a constant here"""
    from ape_amd import ops
    if name in ("lds_max", "lds_max_plus_1"):
        side = math.isqrt(ops.label_hist_lds_bins())
        assert side * side * 4 >= 64 * 1024, "the LDS path must reach past the 64 KiB a kernel gets without asking"
        side += name == "lds_max_plus_1"
        return side, side
    return name


@pytest.mark.parametrize("table", [(1, 1), (2, 3), (134, 134), (151, 151), "lds_max", "lds_max_plus_1", (460, 460), (101, 501)],
                         ids=lambda t: t if isinstance(t, str) else f"{t[0]}x{t[1]}")
def test_sizes_and_unaligned_bases(table):
    """every n around the vector and wave boundaries, the base pointers 0, 1 and 3 elements into a larger buffer (together, which keeps
    the vector body behind a scalar head, and apart, which leaves no common vector boundary)"""
    na, nb = _table(table)
    seed = 0
    for n in NS:
        for off in OFFSETS:
            seed += 1
            a, b = _random(n, na, seed, pad=off), _random(n, nb, 1000 + seed, pad=off)
            check(a, b, na, nb)
        check(_random(n, na, seed, pad=1), _random(n, nb, 1000 + seed, pad=3), na, nb)


@pytest.mark.parametrize("ta", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("tb", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_dtype_pairs(ta, tb):
    n, na, nb = 1003, 7, 5
    a, b = _random(n, na + 1, 1, dtype=ta, pad=1), _random(n, nb + 1, 2, dtype=tb, pad=1)      # the values na / nb are rejected
    check(a, b, na, nb)


@pytest.mark.parametrize("table", [(2, 3), (460, 460)], ids=["lds", "global"])
def test_one_bin_only(table):
    """200 000 pixels of one pair: every add meets the same counter, and the count does not fit 16 bits"""
    na, nb = table
    n = 200_000
    a = torch.full((n,), na - 1, dtype=torch.int16, device="cuda")
    b = torch.full((n,), nb - 2, dtype=_dtype_for(nb), device="cuda")
    hist = check(a, b, na, nb)
    assert int(hist[na - 1, nb - 2]) == n


@pytest.mark.parametrize("table", [(134, 134), (460, 460)], ids=["lds", "global"])
@pytest.mark.parametrize("kind", ["coherent", "random"])
def test_coherent_and_random_maps(kind, table):
    na, nb = table
    H, W = 300, 400
    if kind == "coherent":                                   # constant 37 x 53 blocks
        by, bx = torch.arange(H)[:, None] // 37, torch.arange(W)[None, :] // 53
        a = ((by * 8 + bx) * 7 % na).to(torch.int16).cuda()
        b = ((by * 8 + bx) * 11 % nb).to(_dtype_for(nb)).cuda()
    else:
        a, b = _random(H * W, na, 3, dtype=torch.int16).view(H, W), _random(H * W, nb, 4).view(H, W)
    check(a, b, na, nb)


def test_ignore_label_and_rejected_values():
    from ape_amd import ops
    na, nb = 6, 5
    a = torch.tensor([0, 1, 2, 5, 6, 100, 3, 3, 255, 4], dtype=torch.uint8).cuda()
    b = torch.tensor([0, 255, 4, 255, 1, 1, 5, 2, 0, 254], dtype=torch.uint8).cuda()
    hist = check(a, b, na, nb, b_ignore=255)
    assert int(hist[1, 4]) == 1 and int(hist[5, 4]) == 1                   # 255 on the b side is the last bin
    check(a, b, na, nb, a_ignore=255, b_ignore=255)
    check(a, b, na, nb)                                                    # without an ignore value 255 is out of range
    for dt in (torch.int16, torch.int32):
        lo = torch.iinfo(dt).min
        a = torch.tensor([0, -1, 2, lo, 5, 3, 6, 1, -2, 4] * 13, dtype=dt).cuda()
        b = torch.tensor([1, 1, -1, 0, 4, lo, 0, 5, 2, 255] * 13, dtype=dt).cuda()
        hist, rejected = ops.label_pair_hist(a, b, na, nb, b_ignore=255)
        assert int(rejected) == 13 * 7 and int(hist.sum()) == 13 * 3
        check(a, b, na, nb, b_ignore=255)
        check(a, b, na, nb)                                                # -1 = no ignore value: a label of -1 is rejected, not remapped


def test_accumulates_into_int64_out():
    from ape_amd import ops
    na, nb = 134, 134
    a1, b1 = _random(5000, na, 1, dtype=torch.int16), _random(5000, nb + 3, 2)
    a2, b2 = _random(777, na, 3, dtype=torch.int16), _random(777, nb + 3, 4)
    out = torch.zeros((na, nb), dtype=torch.int64, device="cuda")
    out[3, 4] = 2 ** 40
    rejected = torch.zeros((1,), dtype=torch.int64, device="cuda")
    rejected[0] = 2 ** 40
    for a, b in ((a1, b1), (a2, b2)):
        h, r = ops.label_pair_hist(a, b, na, nb, out=out, rejected=rejected)
        assert h is out and r is rejected
    (w1, r1), (w2, r2) = host_hist(a1, b1, na, nb), host_hist(a2, b2, na, nb)
    want = w1 + w2
    want[3, 4] += 2 ** 40
    assert torch.equal(out.cpu(), want) and int(rejected) == 2 ** 40 + r1 + r2 and r1 + r2 > 0


def test_rejects_wrong_inputs():
    from ape_amd import ops
    a = torch.zeros((4, 6), dtype=torch.int16, device="cuda")
    with pytest.raises(TypeError):
        ops.label_pair_hist(a.long(), a, 2, 2)
    with pytest.raises(TypeError):
        ops.label_pair_hist(a, a.bool(), 2, 2)
    with pytest.raises(ValueError):
        ops.label_pair_hist(a.t(), a.t(), 2, 2)
    with pytest.raises(ValueError):
        ops.label_pair_hist(a, a[:2], 2, 2)
    with pytest.raises(ValueError):
        ops.label_pair_hist(a, a, 2, 2, out=torch.zeros((2, 2), dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("table", [(134, 134), (460, 460)], ids=["lds", "global"])
def test_captures_into_a_graph(table):
    """one launch, no allocation and no host synchronisation: captured in a single-branch graph, two replays add twice the counts"""
    from ape_amd import ops
    na, nb = table
    a, b = _random(30_011, na, 7, dtype=torch.int16), _random(30_011, nb + 1, 8)
    out = torch.zeros((na, nb), dtype=torch.int64, device="cuda")
    rejected = torch.zeros((1,), dtype=torch.int64, device="cuda")
    ops.label_pair_hist(a, b, na, nb, out=out, rejected=rejected)          # first use sets the kernel's attributes
    torch.cuda.synchronize()
    out.zero_()
    rejected.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.label_pair_hist(a, b, na, nb, out=out, rejected=rejected)
    torch.cuda.synchronize()
    assert int(out.sum()) == 0 and int(rejected) == 0                      # capturing does not run the kernel
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    want, want_rejected = host_hist(a, b, na, nb)
    assert torch.equal(out.cpu(), 2 * want) and int(rejected) == 2 * want_rejected and want_rejected > 0


def test_accumulators_on_the_models_own_outputs():
    """model.forward's sem_seg / panoptic_seg of the tiny panoptic fixture scored against themselves: 100 everywhere; against themselves
    shifted by one pixel: strictly less"""
    import model_util as M
    from ape_amd import ops
    from ape_amd.evaluation import PanopticAccumulator, SemSegAccumulator

    model, image, text, gold = M.build_model("tiny_panoptic", device="cuda", dtype=torch.float32)
    mv = model.model_vision
    meta = gold["semantic_meta"]
    mv.dataset_names, mv.dataset_name_to_idx, mv.dataset_prompts = ["coco"], {"coco": 0}, ["name"]
    mv.set_metadata(0, name="coco_2017_val", thing_classes=meta["thing_classes"], stuff_classes=meta["stuff_classes"],
                    thing_dataset_id_to_contiguous_id={i + 1: i for i in range(len(meta["thing_classes"]))})
    mv.semantic_on = mv.panoptic_on = True
    mv.panoptic_configs = dict(gold["panoptic_cfg"])
    mv.set_model_language(M.TextStub(text.cuda()))
    mv.set_eval_dataset("coco_2017_val")
    H, W = gold["out_hw"]
    res = model([{"image": image.cuda(), "height": H, "width": W}])[0]

    scores = res["sem_seg"]
    C = scores.shape[0]
    labels = ops.argmax_labels(scores.float().contiguous())
    assert labels.is_cuda and len(torch.unique(labels)) > 1
    same, shifted = SemSegAccumulator(C), SemSegAccumulator(C)
    same.update(scores, labels)                              # [C, H, W] scores against their own label map
    shifted.update(labels, torch.roll(labels, 1, 1).cpu())   # int16 labels against a host ground truth one pixel to the right
    r0, r1 = same.compute(), shifted.compute()
    assert r0["mIoU"] == 100.0 and r0["pACC"] == 100.0 and int(same.conf.sum()) == H * W
    assert r1["mIoU"] < 100.0 and r1["pACC"] < 100.0 and int(shifted.conf.sum()) == H * W

    seg, info = res["panoptic_seg"]
    assert seg.is_cuda and seg.dtype == torch.int32 and len(info) > 1
    # thing and stuff category ids are separate number spaces in the model's output: one space for the scorer
    pred_info = [dict(d, category_id=d["category_id"] + (0 if d["isthing"] else 1000)) for d in info]
    gt_info = [{"id": d["id"], "category_id": d["category_id"], "iscrowd": 0} for d in pred_info]
    categories = {d["category_id"]: d["isthing"] for d in pred_info}
    same, shifted = PanopticAccumulator(categories), PanopticAccumulator(categories)
    same.update(seg, pred_info, seg, gt_info)
    shifted.update(seg, pred_info, torch.roll(seg, 1, 1).cpu(), gt_info)
    q0, q1 = same.compute(), shifted.compute()
    assert q0["All"]["n"] == len(categories) and q0["Things"]["n"] > 0 and q0["Stuff"]["n"] > 0      # the fixture has both kinds
    for group in ("All", "Things", "Stuff"):
        assert q0[group]["PQ"] == q0[group]["SQ"] == q0[group]["RQ"] == 100.0, q0
    assert q1["All"]["PQ"] < 100.0 and q1["All"]["SQ"] < 100.0, q1
