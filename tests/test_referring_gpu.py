"""-m gpu: `ops.mask_paired_counts` (csrc/maskiou.hip) for exact equality with host integer arithmetic -- `(a & b).sum`, `a.sum`, `b.sum`
in int64 -- over sizes, value sets, every pair of misalignments, the multi-workgroup path and a captured graph; `ReferringAccumulator`
against `referring_metrics` of host counts; and the scores end to end on the tiny fixture model in expression mode."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 63), (3, 21), (8, 8), (5, 13), (37, 53), (64, 64), (200, 333)]      # below a vector, below a wave step, 4096 pixels, across steps


def host_counts(a, b):
    a, b = a.cpu().flatten(1) != 0, b.cpu().flatten(1) != 0
    return torch.stack([(a & b).long().sum(1), a.long().sum(1), b.long().sum(1)], 1)


def _values(shape, seed, kind):
    g = torch.Generator().manual_seed(seed)
    if kind == "bool":
        return torch.rand(shape, generator=g) < 0.4
    return torch.tensor([0, 1, 2, 255], dtype=torch.uint8)[torch.randint(0, 4, shape, generator=g)]


# ---------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_counts_over_sizes_value_sets_and_unaligned_bases(hw):
    """values {0, 1, 2, 255} and bool storage on either side; n = 4 from slice [0:] and from slice [1:] of a larger buffer (an odd H * W
    then gives odd byte addresses, and the two sides' addresses differ in their alignment)"""
    from ape_amd import ops
    H, W = hw
    for ka, kb in (("u8", "u8"), ("u8", "bool"), ("bool", "u8")):
        ha, hb = _values((5, H, W), H * 1000 + W, ka), _values((5, H, W), H * 1000 + W + 7, kb)
        da, db = ha.cuda(), hb.cuda()
        for fa, fb in ((0, 0), (1, 1), (0, 1), (1, 0)):
            a, b = da[fa: fa + 4], db[fb: fb + 4]
            assert a.is_contiguous() and a.data_ptr() == da.data_ptr() + fa * H * W
            got = ops.mask_paired_counts(a, b)
            assert got.dtype == torch.int64 and tuple(got.shape) == (4, 3) and got.is_cuda
            assert torch.equal(got.cpu(), host_counts(ha[fa: fa + 4], hb[fb: fb + 4])), (hw, ka, kb, fa, fb)


def test_counts_at_every_pair_of_misalignments():
    """3 x (37 x 53) masks with a behind 0 .. 16 leading bytes and b behind 0 .. 16 leading bytes: all 289 combinations.  Both buffers hold
    255 around the masks, so a byte read outside them changes a count."""
    from ape_amd import ops
    n, H, W = 3, 37, 53
    ha, hb = _values((n, H, W), 7, "u8"), _values((n, H, W), 8, "u8")
    want = host_counts(ha, hb)
    views = []
    for host in (ha, hb):
        side = []
        for off in range(17):
            buf = torch.full((off + n * H * W + 64,), 255, dtype=torch.uint8, device="cuda")
            buf[off: off + n * H * W] = host.reshape(-1).cuda()
            side.append(buf[off: off + n * H * W].view(n, H, W))
        views.append(side)
    out = torch.empty((17, 17, n, 3), dtype=torch.int64, device="cuda")
    for i, a in enumerate(views[0]):
        for j, b in enumerate(views[1]):
            ops.mask_paired_counts(a, b, out=out[i, j])
    got = out.cpu()
    bad = [(i, j) for i in range(17) for j in range(17) if not torch.equal(got[i, j], want)]
    assert not bad, bad[:10]


def test_interior_steps_at_every_pair_of_misalignments():
    """the same at 2 x (150 x 101) masks, 15 150 pixels = 3.7 wave steps: the steps that lie wholly inside a mask take the path that loads
    without looking at the ends, at every fourth misalignment of either side and the last one"""
    from ape_amd import ops
    n, H, W = 2, 150, 101
    ha, hb = _values((n, H, W), 17, "u8"), _values((n, H, W), 18, "bool")
    want = host_counts(ha, hb)
    offs = (0, 1, 4, 8, 12, 15)
    views = []
    for host in (ha, hb.view(torch.uint8) * 3):
        side = []
        for off in offs:
            buf = torch.full((off + n * H * W + 64,), 255, dtype=torch.uint8, device="cuda")
            buf[off: off + n * H * W] = host.reshape(-1).cuda()
            side.append(buf[off: off + n * H * W].view(n, H, W))
        views.append(side)
    out = torch.empty((len(offs), len(offs), n, 3), dtype=torch.int64, device="cuda")
    for i, a in enumerate(views[0]):
        for j, b in enumerate(views[1]):
            ops.mask_paired_counts(a, b, out=out[i, j])
    got = out.cpu()
    bad = [(offs[i], offs[j]) for i in range(len(offs)) for j in range(len(offs)) if not torch.equal(got[i, j], want)]
    assert not bad, bad[:10]


@pytest.mark.parametrize("n", [1, 3])
def test_counts_on_the_multi_workgroup_path(n):
    """512 x 512: 64 wave steps per pair, spread over workgroups that meet in atomics on `out`, which the call zeroes itself: all-zero,
    all-one (counts past 16 bits) and random contents, and a second call into the same `out` leaves the single-call result"""
    from ape_amd import ops
    S = 512
    zero = torch.zeros((n, S, S), dtype=torch.uint8, device="cuda")
    one = torch.ones((n, S, S), dtype=torch.uint8, device="cuda")
    assert ops.mask_paired_counts(zero, zero).tolist() == [[0, 0, 0]] * n
    assert ops.mask_paired_counts(one, one).tolist() == [[S * S] * 3] * n
    assert ops.mask_paired_counts(zero, one).tolist() == [[0, 0, S * S]] * n
    ha, hb = _values((n, S, S), 31 + n, "u8"), _values((n, S, S), 41 + n, "bool")
    a, b = ha.cuda(), hb.cuda()
    want = host_counts(ha, hb)
    out = torch.full((n, 3), 2 ** 40, dtype=torch.int64, device="cuda")
    for _ in range(2):
        assert ops.mask_paired_counts(a, b, out=out) is out
        assert torch.equal(out.cpu(), want)


def test_empty_batch_and_empty_masks():
    from ape_amd import ops
    e = torch.zeros((0, 37, 53), dtype=torch.uint8, device="cuda")
    got = ops.mask_paired_counts(e, e)
    assert tuple(got.shape) == (0, 3) and got.dtype == torch.int64
    z = torch.zeros((2, 0, 5), dtype=torch.uint8, device="cuda")                # no pixels: the call still zeroes out
    out = torch.full((2, 3), 9, dtype=torch.int64, device="cuda")
    assert ops.mask_paired_counts(z, z, out=out).tolist() == [[0, 0, 0]] * 2


def test_wrapper_rejects_wrong_inputs():
    from ape_amd import ops
    m = torch.zeros((2, 6, 10), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        ops.mask_paired_counts(m, m[:, :, :9].contiguous())                     # size mismatch
    with pytest.raises(ValueError):
        ops.mask_paired_counts(m, m[:1])                                        # different n
    with pytest.raises(TypeError):
        ops.mask_paired_counts(m.int(), m)                                      # wrong dtype
    with pytest.raises(TypeError):
        ops.mask_paired_counts(m, m.float())
    with pytest.raises(ValueError):
        ops.mask_paired_counts(m.transpose(1, 2), m.transpose(1, 2))            # not contiguous
    with pytest.raises(ValueError):
        ops.mask_paired_counts(m, m, out=torch.zeros((2, 2), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ops.mask_paired_counts(m, m, out=torch.zeros((2, 3), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ops.mask_paired_counts(m, m, out=torch.zeros((2, 6), dtype=torch.int64, device="cuda")[:, ::2])
    with pytest.raises(RuntimeError):
        ops.mask_paired_counts(m.cpu(), m)                                      # a host tensor: no CPU path
    with pytest.raises(RuntimeError):
        ops.mask_paired_counts(m, m, out=torch.zeros((2, 3), dtype=torch.int64))


def test_counts_capture_into_a_graph():
    """a single-branch graph of the memset node and the kernel: capturing runs nothing, two replays leave exactly the single-run counts"""
    from ape_amd import ops
    ha, hb = _values((3, 200, 333), 21, "u8"), _values((3, 200, 333), 22, "u8")
    a, b = ha.cuda(), hb.cuda()
    want = host_counts(ha, hb)
    assert torch.equal(ops.mask_paired_counts(a, b).cpu(), want)                # warm: nothing is set up lazily inside the capture
    out = torch.empty((3, 3), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.mask_paired_counts(a, b, out=out)
    torch.cuda.synchronize()
    out.fill_(-7)
    torch.cuda.synchronize()
    assert int(out[0, 0]) == -7                                                 # capturing did not run the kernel
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want)


# ---------------------------------------------------------------------------------------------------- accumulator
def _blob(H, W, seed, p=0.5):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand((1, 1, (H + 3) // 4 + 1, (W + 3) // 4 + 1), generator=g)
    return (torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)[0, 0] > p).to(torch.uint8)


def _stream():
    """12 samples of differing sizes: (pred mask or None, gt mask, pred box or None, gt box), all on the host"""
    sizes = [(37, 53), (64, 64), (5, 13), (200, 333), (48, 64), (1, 63), (120, 90), (37, 53), (8, 8), (33, 77), (64, 48), (100, 100)]
    g = torch.Generator().manual_seed(3)
    samples = []
    for i, (H, W) in enumerate(sizes):
        pred, gt = _blob(H, W, 100 + i, 0.45), _blob(H, W, 200 + i, 0.5)
        if i % 3 == 0:
            pred = (gt.bool() & _blob(H, W, 300 + i, 0.3).bool()).to(torch.uint8)      # a part of the ground truth: a high IoU
        gb = torch.tensor([2.0, 3.0, 2.0 + W, 3.0 + H], dtype=torch.float64)
        pb = gb + torch.rand(4, generator=g, dtype=torch.float64) * (i % 4) * 0.1 * min(H, W)
        if i == 4:
            pred, pb = None, None                                                      # no prediction
        if i == 8:
            pred.zero_()
            gt.zero_()                                                                 # empty against empty
        samples.append((pred, gt, pb, gb))
    return samples


def _host_reference(samples, boxes=True):
    from ape_amd.evaluation import referring_metrics
    counts, rows = [], []
    for pred, gt, pb, gb in samples:
        p = torch.zeros_like(gt) if pred is None else pred
        counts.append(host_counts(p[None], gt[None])[0])
        rows.append(torch.cat([torch.zeros(4, dtype=torch.float64) if pb is None else pb, gb]))
    return referring_metrics(torch.stack(counts), torch.stack(rows) if boxes else None)


@pytest.mark.parametrize("form", ["device", "host", "rle"])
def test_accumulator_on_a_stream_of_samples(form):
    """the prediction as a device tensor, as a host tensor and as an RLE dict; one sample without prediction, one empty against empty.
    Every key equals `referring_metrics` of the counts of host integer arithmetic."""
    from ape_amd.evaluation import ReferringAccumulator, encode_masks, referring_scores
    samples = _stream()
    want = _host_reference(samples)
    acc = ReferringAccumulator()
    listed = []
    for i, (pred, gt, pb, gb) in enumerate(samples):
        if pred is not None:
            pred = {"device": lambda m: m.cuda(), "host": lambda m: m, "rle": lambda m: encode_masks(m[None].cuda())[0]}[form](pred)
        gt_in = [gt.cuda(), gt, encode_masks(gt[None].cuda())[0], gt[None].bool().cuda()][i % 4]      # the ground truth in every form, too
        acc.update(None, gt_in, gb, pred_mask=pred, pred_box=pb)
        listed.append((None if pred is None else (pred, pb), gt_in, gb))
    assert acc.n == len(samples) and acc.counts.is_cuda and acc.counts.dtype == torch.int64 and acc.boxes.dtype == torch.float64
    acc.reduce()                                                # no process group: a no-op
    got = acc.compute()
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    assert 0.0 < got["mIoU"] < 100.0 and got["samples"] == 12
    assert referring_scores(listed) == want                     # the one-call form


def test_accumulator_takes_instances_and_the_highest_score():
    """`Instances` with several detections: the highest-scoring one is scored, on a tie the first; an `Instances` of length 0 is a sample
    without prediction; masks as `pred_masks` on the device, on the host, and as `pred_masks_rle`"""
    from ape_amd.evaluation import ReferringAccumulator, encode_masks, referring_metrics
    from ape_amd.structures import make_instances
    H, W = 37, 53
    masks = torch.stack([_blob(H, W, 50 + i) for i in range(4)])
    boxes = torch.tensor([[0, 0, 10, 10], [1, 2, 30, 20], [5, 5, 40, 30], [0, 0, 53, 37]], dtype=torch.float32)
    scores = torch.tensor([0.2, 0.9, 0.9, 0.1])                 # a tie between 1 and 2: the first wins
    classes = torch.zeros(4, dtype=torch.long)
    gt, gb = _blob(H, W, 60), torch.tensor([1.0, 2.0, 31.0, 22.0])
    want_counts = [host_counts(masks[1][None], gt[None])[0], host_counts(torch.zeros_like(gt)[None], gt[None])[0]]
    want_boxes = [torch.cat([boxes[1].double(), gb.double()]), torch.cat([torch.zeros(4, dtype=torch.float64), gb.double()])]
    want = referring_metrics(torch.stack(want_counts), torch.stack(want_boxes))
    none = make_instances((H, W), boxes[:0], scores[:0], classes[:0], masks[:0])
    for form in ("device", "host", "rle"):
        if form == "device":
            inst = make_instances((H, W), boxes.cuda(), scores.cuda(), classes.cuda(), masks.cuda())
        elif form == "host":
            inst = make_instances((H, W), boxes, scores, classes, masks.bool())
        else:
            inst = make_instances((H, W), boxes, scores, classes, pred_masks_rle=encode_masks(masks.cuda()))
        acc = ReferringAccumulator()
        acc.update(inst, gt.cuda(), gb)
        acc.update(none, gt.cuda(), gb)
        assert acc.compute() == want, form
    acc = ReferringAccumulator()
    acc.update(inst, gt, None)
    assert not any(k.startswith("P@") for k in acc.compute())   # no sample has boxes: no P@k
    with pytest.raises(ValueError):
        acc.update(inst, gt, gb)                                # some with boxes, some without
    with pytest.raises(ValueError):
        acc.update(inst, _blob(H, W + 1, 1), None)              # size mismatch
    with pytest.raises(ValueError):
        ReferringAccumulator().update(None, gt, gb, pred_mask=masks[0])       # gt_box without a box for the prediction


def test_accumulator_grows_past_its_capacity():
    from ape_amd.evaluation import ReferringAccumulator
    samples = _stream()
    want = _host_reference(samples)
    acc = ReferringAccumulator(capacity=2)
    for pred, gt, pb, gb in samples:
        acc.update(None, gt.cuda(), gb.cuda(), pred_mask=None if pred is None else pred.cuda(), pred_box=None if pb is None else pb.cuda())
    assert acc.capacity == 16 and tuple(acc.counts.shape) == (16, 3) and tuple(acc.boxes.shape) == (16, 8) and acc.n == 12
    assert acc.compute() == want                                # the earlier rows survived three doublings


def test_update_with_device_inputs_does_not_synchronise():
    """masks (and boxes, here on either side of the bus) already on the device: `update` runs with torch's synchronisation check set to
    raise -- no device-to-host copy, no blocking host-to-device copy, no stream synchronisation, also while the tables grow"""
    from ape_amd.evaluation import ReferringAccumulator
    samples = _stream()
    want = _host_reference(samples)
    dev = [(None if p is None else p.cuda(), g.cuda(), None if pb is None else pb.cuda(), gb) for p, g, pb, gb in samples]
    acc = ReferringAccumulator(device="cuda", capacity=4)
    acc.update(None, dev[0][1], dev[0][3], pred_mask=dev[0][0], pred_box=dev[0][2])       # the first call loads the library
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for pred, gt, pb, gb in dev[1:]:
            acc.update(None, gt, gb, pred_mask=pred, pred_box=pb)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert acc.compute() == want


# ---------------------------------------------------------------------------------------------------- end to end
def test_expression_mode_scores_end_to_end():
    """the tiny phrase fixture on the device in float32, called with prompt "expression": one instance.  Against its own mask and box
    every score is 100 (an empty mask has no union: oIoU is then 0 by definition); against the complement of its mask mIoU is 0."""
    import model_util as M
    from ape_amd.evaluation import ReferringAccumulator, referring_scores
    model, orc, image, text, gold = M.build_pair("tiny_phrase", device="cuda", dtype=torch.float32)
    h, w = image.shape[-2:]
    inst = model([{"image": image, "height": h, "width": w, "text_features": text, "prompt": "expression"}])[0]["instances"]
    assert len(inst) == 1 and inst.has("pred_masks") and tuple(inst.pred_masks.shape) == (1, h, w)
    mask, box = inst.pred_masks[0], inst.pred_boxes.tensor[0]
    area = int(mask.sum())
    print(f"[expression] mask area {area} of {h * w}, box {box.tolist()}")
    acc = ReferringAccumulator()
    acc.update(inst, mask.cuda(), box)
    r = acc.compute()
    assert r["samples"] == 1 and r["mIoU"] == 100.0 and r["P@0.5"] == 100.0 and r["P@0.9"] == 100.0 and r["mask_P@0.9"] == 100.0
    assert r["oIoU"] == (100.0 if area > 0 else 0.0)
    assert referring_scores([(inst, mask, box)]) == r
    flipped = referring_scores([(inst, ~mask.bool())])
    if area > 0:
        # nothing in common, a union of the whole image: oIoU is exactly 0, and mIoU is the reference's epsilon quotient for it,
        # float32 (0 + 1e-6) / (h w + 1e-6) -- 0.0 to nine decimals, not the float 0.0
        eps_quotient = float((torch.zeros((), dtype=torch.float32) + 1e-6) / (torch.tensor(float(h * w), dtype=torch.float32) + 1e-6))
        assert flipped["mIoU"] == 100.0 * eps_quotient and flipped["mIoU"] < 1e-6
        assert flipped["oIoU"] == 0.0 and flipped["mask_P@0.5"] == 0.0
    assert "P@0.5" not in flipped
