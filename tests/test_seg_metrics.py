"""Semantic and panoptic scores (ape_amd/evaluation.py) on the CPU: known answers worked out by hand from the published definitions
(detectron2's SemSegEvaluator, panopticapi's pq_compute), the accumulators' host logic with `ops.label_pair_hist` replaced by the
torch.bincount definition below, and the C entry point's argument checks (which need no GPU)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def bincount_hist(a, b, na, nb, a_ignore=None, b_ignore=None, out=None, rejected=None):
    """ops.label_pair_hist restated with torch.bincount"""
    for t in (a, b):
        if t.dtype not in (torch.uint8, torch.int16, torch.int32):
            raise TypeError(f"label maps are uint8, int16 or int32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError("label maps must be contiguous")
    a, b = a.reshape(-1).long(), b.reshape(-1).long()
    assert a.numel() == b.numel()
    if a_ignore is not None:
        a = torch.where(a == a_ignore, torch.full_like(a, na - 1), a)
    if b_ignore is not None:
        b = torch.where(b == b_ignore, torch.full_like(b, nb - 1), b)
    ok = (a >= 0) & (a < na) & (b >= 0) & (b < nb)
    hist = torch.bincount(a[ok] * nb + b[ok], minlength=na * nb).reshape(na, nb)
    if out is None:
        out = torch.zeros((na, nb), dtype=torch.int64)
    if rejected is None:
        rejected = torch.zeros((1,), dtype=torch.int64)
    out += hist
    rejected += int((~ok).sum())
    return out, rejected


@pytest.fixture
def host_hist(monkeypatch, fake_ops):
    import ape_amd.ops as ops
    monkeypatch.setattr(ops, "label_pair_hist", bincount_hist, raising=True)


def _close(got, want):
    assert got == pytest.approx(want, rel=1e-9, abs=1e-12), (got, want)


# ---------------------------------------------------------------------------------------------------- semantic
def test_semantic_known_answer():
    from ape_amd.evaluation import semantic_metrics
    conf = torch.tensor([[2, 1, 0], [1, 1, 1], [0, 0, 0]])          # [pred, gt] of gt = 0 0 0 1 1 255, pred = 0 0 1 1 0 1
    res = semantic_metrics(conf, class_names=["sky", "sea"])
    _close(res["mIoU"], 100 * (2 / 4 + 1 / 3) / 2)
    _close(res["mACC"], 100 * (2 / 3 + 1 / 2) / 2)
    _close(res["pACC"], 60.0)
    _close(res["fwIoU"], 100 * (0.6 * 2 / 4 + 0.4 * 1 / 3))
    _close(res["mIoU"], 41.666666666666667)
    _close(res["mACC"], 58.333333333333333)
    _close(res["fwIoU"], 43.333333333333333)
    _close(res["IoU-sky"], 50.0)
    _close(res["ACC-sea"], 50.0)


def test_semantic_class_without_ground_truth_is_left_out_of_every_mean():
    from ape_amd.evaluation import semantic_metrics
    conf = torch.zeros((4, 4), dtype=torch.int64)                   # three classes; class 2 has no GT pixel but is predicted twice
    conf[:2, :2] = torch.tensor([[2, 1], [1, 1]])
    conf[2, 0] = 2
    res = semantic_metrics(conf)
    # gt: class 0 has 5 pixels, class 1 has 2; predictions of class 2 enlarge class 0's union only
    _close(res["mIoU"], 100 * (2 / (5 + 3 - 2) + 1 / (2 + 2 - 1)) / 2)
    _close(res["mACC"], 100 * (2 / 5 + 1 / 2) / 2)
    _close(res["pACC"], 100 * 3 / 7)
    _close(res["fwIoU"], 100 * (5 / 7 * 2 / 6 + 2 / 7 * 1 / 3))
    assert res["IoU-2"] != res["IoU-2"] and res["ACC-2"] != res["ACC-2"]          # NaN: not scored


def test_semseg_accumulator_known_answer_and_ignore(host_hist):
    from ape_amd.evaluation import SemSegAccumulator
    acc = SemSegAccumulator(2, ignore_label=255)
    gt = torch.tensor([[0, 0, 0], [1, 1, 255]], dtype=torch.uint8)
    pred = torch.tensor([[0, 0, 1], [1, 0, 1]], dtype=torch.int16)
    acc.update(pred, gt)
    assert acc.conf.tolist() == [[2, 1, 0], [1, 1, 1], [0, 0, 0]]
    res = acc.compute()
    _close(res["mIoU"], 41.666666666666667)
    _close(res["pACC"], 60.0)
    acc.update(pred, gt)                                           # accumulates
    assert acc.conf.tolist() == [[4, 2, 0], [2, 2, 2], [0, 0, 0]]
    _close(acc.compute()["mIoU"], 41.666666666666667)


def test_semseg_scores_and_int16_labels_give_the_same_matrix(host_hist):
    from ape_amd.evaluation import SemSegAccumulator
    g = torch.Generator().manual_seed(0)
    scores = torch.randn(5, 9, 11, generator=g)
    gt = torch.randint(0, 5, (9, 11), generator=g).to(torch.uint8)
    gt[0, :3] = 255
    a, b = SemSegAccumulator(5), SemSegAccumulator(5)
    a.update(scores, gt)
    b.update(scores.argmax(0).to(torch.int16), gt.to(torch.int32))
    assert torch.equal(a.conf, b.conf) and int(a.conf.sum()) == 99 and int(a.conf[:, 5].sum()) == 3


def test_semseg_rejected_pixels_raise_in_compute_and_sizes_must_match(host_hist):
    from ape_amd.evaluation import SemSegAccumulator
    acc = SemSegAccumulator(3)
    acc.update(torch.tensor([[0, 1, 2, 1]], dtype=torch.int16), torch.tensor([[0, 1, 7, 255]], dtype=torch.uint8))   # GT 7: no such class
    assert int(acc.rejected) == 1 and int(acc.conf.sum()) == 3
    with pytest.raises(ValueError, match="outside"):
        acc.compute()
    with pytest.raises(ValueError):
        acc.update(torch.zeros((2, 3), dtype=torch.int16), torch.zeros((3, 2), dtype=torch.uint8))
    with pytest.raises(ValueError):
        SemSegAccumulator(3).update(torch.zeros((4, 2, 2)), torch.zeros((2, 2), dtype=torch.uint8))                  # 4 score planes, 3 classes
    with pytest.raises(ValueError):
        SemSegAccumulator(300, ignore_label=255)


# ---------------------------------------------------------------------------------------------------- panoptic
CATEGORIES = {0: True, 5: False, 7: False}
G1, G2, G3 = 0x0A0B0C, 0xFFFFFE, 0x010000          # packed-RGB sized ids, out of order


def _panoptic_case():
    """4 x 6: g1 thing(0) columns 0-1; g2 thing(0) crowd columns 2-3; g3 stuff(5) columns 4-5 rows 0-2; VOID columns 4-5 row 3.
    p1 (0) columns 0-1 rows 0-2; p2 (0) columns 2-3; p3 (5) columns 4-5; p4 (7) columns 0-1 row 3."""
    gt = torch.zeros((4, 6), dtype=torch.int64)
    gt[:, 0:2], gt[:, 2:4], gt[0:3, 4:6] = G1, G2, G3
    gt_info = [{"id": G1, "category_id": 0, "iscrowd": 0}, {"id": G2, "category_id": 0, "iscrowd": 1},
               {"id": G3, "category_id": 5, "iscrowd": 0}]
    pred = torch.zeros((4, 6), dtype=torch.int32)
    pred[0:3, 0:2], pred[:, 2:4], pred[:, 4:6], pred[3, 0:2] = 1, 2, 3, 4
    pred_info = [{"id": 1, "isthing": True, "category_id": 0}, {"id": 2, "isthing": True, "category_id": 0},
                 {"id": 3, "isthing": False, "category_id": 5}, {"id": 4, "isthing": False, "category_id": 7}]
    return pred, pred_info, gt, gt_info


def test_panoptic_known_answer(host_hist):
    from ape_amd.evaluation import PanopticAccumulator
    acc = PanopticAccumulator(CATEGORIES)
    acc.update(*_panoptic_case())
    assert acc.per_class() == {0: {"tp": 1, "fp": 0, "fn": 0, "iou": 0.75},          # p1 ~ g1 at 6 / 8; p2 absorbed by the crowd g2
                               5: {"tp": 1, "fp": 0, "fn": 0, "iou": 1.0},           # p3 ~ g3: its two VOID pixels leave the union
                               7: {"tp": 0, "fp": 1, "fn": 0, "iou": 0.0}}           # p4: no GT of its category
    res = acc.compute()
    _close(res["All"]["PQ"], 100 * (0.75 + 1.0 + 0.0) / 3)
    _close(res["All"]["PQ"], 58.333333333333333)
    _close(res["All"]["SQ"], 58.333333333333333)
    _close(res["All"]["RQ"], 66.666666666666667)
    assert res["All"]["n"] == 3
    _close(res["Things"]["PQ"], 75.0)
    assert res["Things"]["n"] == 1
    _close(res["Stuff"]["PQ"], 50.0)
    assert res["Stuff"]["n"] == 2


def test_panoptic_quality_counts_only_classes_that_occur():
    from ape_amd.evaluation import panoptic_quality
    per_class = {1: {"tp": 2, "fp": 1, "fn": 1, "iou": 1.5}, 2: {"tp": 0, "fp": 0, "fn": 0, "iou": 0.0}, 3: {"tp": 0, "fp": 0, "fn": 4, "iou": 0.0}}
    res = panoptic_quality(per_class, {1: True, 2: True, 3: False})
    _close(res["Things"]["PQ"], 100 * 1.5 / 3)
    _close(res["Things"]["SQ"], 75.0)
    _close(res["Things"]["RQ"], 100 * 2 / 3)
    assert res["Things"]["n"] == 1 and res["Stuff"]["n"] == 1 and res["All"]["n"] == 2
    _close(res["Stuff"]["PQ"], 0.0)
    _close(res["All"]["PQ"], 25.0)


def test_panoptic_gt_ids_are_compacted_and_unknown_ids_raise(host_hist, monkeypatch):
    import ape_amd.ops as ops
    from ape_amd.evaluation import PanopticAccumulator
    pred, pred_info, gt, gt_info = _panoptic_case()
    seen = {}

    def spy(a, b, na, nb, **kw):
        seen["a"], seen["shape"] = a.clone(), (na, nb)
        return bincount_hist(a, b, na, nb, **kw)
    monkeypatch.setattr(ops, "label_pair_hist", spy)
    acc = PanopticAccumulator([{"id": c, "isthing": t} for c, t in CATEGORIES.items()])
    acc.update(pred, pred_info, gt, gt_info)
    assert seen["shape"] == (4, 5) and seen["a"].dtype == torch.int32                  # G + 1 rows, P + 1 columns
    want = torch.zeros((4, 6), dtype=torch.int32)                                      # gt_info's order: g1 -> 1, g2 -> 2, g3 -> 3
    want[:, 0:2], want[:, 2:4], want[0:3, 4:6] = 1, 2, 3
    assert torch.equal(seen["a"].reshape(4, 6), want)
    bad = gt.clone()
    bad[0, 0] = 0x123456
    with pytest.raises(KeyError, match=str(0x123456)):
        PanopticAccumulator(CATEGORIES).update(pred, pred_info, bad, gt_info)
    stray = pred.clone()
    stray[0, 0] = 9
    with pytest.raises(KeyError):
        PanopticAccumulator(CATEGORIES).update(stray, pred_info, gt, gt_info)
    with pytest.raises(KeyError):
        PanopticAccumulator(CATEGORIES).update(pred, pred_info[:3], gt, gt_info)       # segment 4 is in the map, not in the list
    with pytest.raises(KeyError):
        PanopticAccumulator({0: True, 5: False}).update(pred, pred_info, gt, gt_info)  # category 7 unknown
    with pytest.raises(ValueError):
        PanopticAccumulator(CATEGORIES).update(pred[:, :5], pred_info, gt, gt_info)


# ---------------------------------------------------------------------------------------------------- reduce over two ranks
def _images():
    g = torch.Generator().manual_seed(5)
    sem = [(torch.randint(0, 4, (7, 9), generator=g).to(torch.int16), torch.randint(0, 5, (7, 9), generator=g).to(torch.uint8)) for _ in range(4)]
    sem = [(p, torch.where(t == 4, torch.full_like(t, 255), t)) for p, t in sem]           # four classes and the ignore label
    pan = []
    for i in range(4):
        pred, pred_info, gt, gt_info = _panoptic_case()
        pan.append((torch.roll(pred, i, 1), pred_info, gt, gt_info))           # shifted predictions: every segment keeps its pixels
    return sem, pan


def _score(sem, pan, reduce):
    from ape_amd.evaluation import PanopticAccumulator, SemSegAccumulator
    s, p = SemSegAccumulator(4), PanopticAccumulator(CATEGORIES)
    for pred, gt in sem:
        s.update(pred, gt)
    for args in pan:
        p.update(*args)
    if reduce:
        s.reduce()
        p.reduce()
    return s.conf.tolist(), s.compute(), p.per_class(), p.compute()


def _worker(rank, world, port, ret):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    import ape_amd.ops as ops
    ops.label_pair_hist = bincount_hist
    sem, pan = _images()
    ret[rank] = _score(sem[rank::world], pan[rank::world], reduce=True)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_reduce_equals_the_single_process_result(host_hist):
    import torch.multiprocessing as mp
    world = 2
    port = 31500 + (os.getpid() % 2000)
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    want = _score(*_images(), reduce=True)                            # no process group here: reduce is a no-op
    assert want[0] != [[0] * 5] * 5 and sum(v["tp"] + v["fp"] + v["fn"] for v in want[2].values()) > 3
    for rank in range(world):
        conf, sem_res, per_class, pq = ret[rank]
        assert conf == want[0] and per_class[0]["tp"] == want[2][0]["tp"] and per_class[7] == want[2][7]
        for c in per_class:
            assert {k: per_class[c][k] for k in ("tp", "fp", "fn")} == {k: want[2][c][k] for k in ("tp", "fp", "fn")}
            _close(per_class[c]["iou"], want[2][c]["iou"])
        for k in ("mIoU", "fwIoU", "mACC", "pACC"):
            _close(sem_res[k], want[1][k])
        for grp in ("All", "Things", "Stuff"):
            assert pq[grp]["n"] == want[3][grp]["n"]
            _close(pq[grp]["PQ"], want[3][grp]["PQ"])


# ---------------------------------------------------------------------------------------------------- C entry point, no GPU
def test_label_pair_hist_argument_errors_are_reported_without_a_gpu():
    import ctypes
    from ape_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.load()
    one = ctypes.c_void_p(64)            # never dereferenced: every call below is refused, or has nothing to do, before any HIP call
    f = lib.ape_hip_label_pair_hist
    assert f(None, 1, one, 1, 5, 2, 2, -1, -1, one, one, None) != 0 and b"null" in lib.ape_hip_last_error()
    assert f(one, 1, None, 1, 5, 2, 2, -1, -1, one, one, None) != 0 and b"null" in lib.ape_hip_last_error()
    assert f(one, 1, one, 1, 5, 2, 2, -1, -1, None, one, None) != 0 and b"null" in lib.ape_hip_last_error()
    assert f(one, 1, one, 1, 5, 2, 2, -1, -1, one, None, None) != 0 and b"null" in lib.ape_hip_last_error()
    assert f(one, 3, one, 1, 5, 2, 2, -1, -1, one, one, None) != 0 and b"width" in lib.ape_hip_last_error()
    assert f(one, 1, one, 8, 5, 2, 2, -1, -1, one, one, None) != 0 and b"width" in lib.ape_hip_last_error()
    assert f(one, 1, one, 1, 5, 0, 2, -1, -1, one, one, None) != 0 and b"table" in lib.ape_hip_last_error()
    assert f(one, 1, one, 1, 5, 2, 0, -1, -1, one, one, None) != 0 and b"table" in lib.ape_hip_last_error()
    assert f(one, 1, one, 1, 5, 65536, 65536, -1, -1, one, one, None) != 0 and b"table" in lib.ape_hip_last_error()
    assert f(None, 2, None, 4, 0, 3, 3, -1, -1, None, None, None) == 0            # n == 0: a successful no-op
