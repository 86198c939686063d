"""-m gpu: `ops.coco_match` (coco_match_kernel in csrc/boxcover.hip) for exact equality of matches and flags with COCOeval's scan written
out literally on the host (coco_util.literal_match -- not the two-phase form the kernel uses), over group layouts, tie-rich and generic IoUs,
crowd fractions and areas on the range boundaries; the rules by name; strided input, junk-filled outputs and a captured graph; the crowd
column of mask IoU from integer counts; `COCOAccumulator` for boxes and masks against the host pipeline (literal matcher + `coco_metrics`);
and that `update` never synchronises.  No tolerances anywhere."""
import functools

import numpy as np
import pytest
import torch

import coco_util as U

pytestmark = pytest.mark.gpu

SIZES = [(0, 0), (0, 3), (3, 0), (1, 1), (5, 7), (7, 5), (63, 3), (3, 65), (65, 64), (100, 130)]       # (detections, ground truth) of a group
LAYOUTS = [(s,) for s in SIZES] + [
    ((5, 7), (0, 0), (7, 5)),
    ((0, 3), (63, 3), (3, 0)),
    ((1, 1), (0, 0), (3, 65), (0, 3), (65, 64), (3, 0), (5, 7)),
    ((0, 0), (0, 0), (100, 130), (0, 0), (0, 3), (7, 5), (0, 0)),
]
AREAS = [0.0, 1024.0, 9216.0, 1e10, 500.0, 5000.0, 20000.0]        # the four range ends exactly, and one inside each of small / medium / large


def _layout_id(layout):
    return "+".join(f"{d}x{g}" for d, g in layout)


@functools.lru_cache(maxsize=None)
def case(layout, family, crowd_tenths):
    """host tensors (iou, det_order, det_offsets, gt_order, gt_offsets, gt_crowd, gt_area, det_area) and the literal loop's (match, flag).
    The matrix has two rows and three columns no group refers to, and the groups' rows and columns are scattered over it."""
    g = torch.Generator().manual_seed(1000 * len(layout) + 10 * sum(d + 3 * m for d, m in layout) + crowd_tenths + (family == "generic"))
    nd, ng = sum(d for d, _ in layout), sum(m for _, m in layout)
    n, m = nd + 2, ng + 3
    if family == "lattice":
        iou = torch.randint(0, 21, (n, m), generator=g).double() / 20          # twentieths: ties everywhere, thresholds hit exactly
    else:
        iou = torch.rand((n, m), generator=g, dtype=torch.float64)
    det_order = torch.randperm(n, generator=g)[:nd].to(torch.int32)
    gt_order = torch.randperm(m, generator=g)[:ng].to(torch.int32)
    det_offsets = torch.tensor([0] + list(np.cumsum([d for d, _ in layout])), dtype=torch.int32)
    gt_offsets = torch.tensor([0] + list(np.cumsum([k for _, k in layout])), dtype=torch.int32)
    crowd = (torch.rand(m, generator=g) * 10 < crowd_tenths).to(torch.uint8)
    areas = torch.tensor(AREAS, dtype=torch.float64)
    gt_area = areas[torch.randint(0, len(AREAS), (m,), generator=g)]
    det_area = areas[torch.randint(0, len(AREAS), (n,), generator=g)]
    args = (iou, det_order, det_offsets, gt_order, gt_offsets, crowd, gt_area, det_area)
    return args, U.host_match(*[a.numpy() for a in args])


def check(got, want, what=""):
    (mt, fl), (hmt, hfl) = got, want
    assert mt.dtype == torch.int32 and fl.dtype == torch.uint8 and mt.is_cuda and fl.is_cuda
    assert tuple(mt.shape) == tuple(hmt.shape) and tuple(fl.shape) == tuple(hfl.shape), (what, tuple(mt.shape), tuple(hmt.shape))
    bad = (fl.cpu() != hfl).nonzero()
    assert bad.numel() == 0, (what, "flag", bad[:5].tolist(), [int(fl.cpu()[tuple(b)]) for b in bad[:5]], [int(hfl[tuple(b)]) for b in bad[:5]])
    bad = (mt.cpu() != hmt).nonzero()
    assert bad.numel() == 0, (what, "match", bad[:5].tolist(), [int(mt.cpu()[tuple(b)]) for b in bad[:5]], [int(hmt[tuple(b)]) for b in bad[:5]])


def run(args, **kw):
    from ape_amd import ops
    return ops.coco_match(*[a.cuda() for a in args], **kw)


# ---------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("crowd_tenths", [0, 3, 10], ids=lambda c: f"crowd{c}")
@pytest.mark.parametrize("family", ["lattice", "generic"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=_layout_id)
def test_matches_and_flags_equal_the_literal_loop(layout, family, crowd_tenths):
    args, want = case(layout, family, crowd_tenths)
    got = run(args)
    assert tuple(got[0].shape) == (4, 10, sum(d for d, _ in layout))
    check(got, want, (layout, family, crowd_tenths))
    if family == "lattice" and crowd_tenths == 3 and sum(min(d, g) for d, g in layout) >= 60:
        flags = set(want[1].unique().tolist())                            # the case is not vacuous: matches of both kinds, and -- where a
        assert {1, 2} <= flags and (0 in flags or layout == ((100, 130),))      # group has more detections than ground truth -- misses


def _one_class(iou, crowd, gt_area, det_area, thresholds=None, ranges=None):
    """a single group in natural order; thresholds / ranges as lists"""
    from ape_amd import ops
    iou = torch.tensor(iou, dtype=torch.float64).reshape(len(det_area), len(gt_area))
    n, m = iou.shape
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)                    # noqa: E731
    args = (iou, i32(list(range(n))), i32([0, n]), i32(list(range(m))), i32([0, m]), torch.tensor(crowd, dtype=torch.uint8),
            torch.tensor(gt_area, dtype=torch.float64), torch.tensor(det_area, dtype=torch.float64))
    got = ops.coco_match(*[a.cuda() for a in args], thresholds=thresholds, ranges=ranges)
    want = U.host_match(*[a.numpy() for a in args], thresholds=U.THRESHOLDS if thresholds is None else thresholds,
                        ranges=U.RANGES if ranges is None else ranges)
    check(got, want)
    return got[0].cpu(), got[1].cpu()


def test_threshold_bits_and_iou_one():
    """17 / 20 is at or above numpy.linspace(.5, .95, 10)[7] (and below 0.5 + 0.05 * 7): a true positive at thresholds 0 .. 7.  An IoU of
    exactly 1 matches at every threshold, 1.0 itself included (lim = min(t, 1 - 1e-10))"""
    mt, fl = _one_class([[17 / 20]], [0], [100.0], [100.0])
    assert fl[0, :, 0].tolist() == [1] * 8 + [0] * 2 and mt[0, :, 0].tolist() == [0] * 8 + [-1] * 2
    mt, fl = _one_class([[1.0]], [0], [100.0], [100.0], thresholds=list(U.THRESHOLDS) + [1.0])
    assert fl[0, :, 0].tolist() == [1] * 11 and mt[0, :, 0].tolist() == [0] * 11
    mt, fl = _one_class([[1.0 - 1e-9]], [0], [100.0], [100.0], thresholds=[0.95, 1.0])
    assert fl[0, :, 0].tolist() == [1, 0]


def test_crowd_rules():
    one = [(0.0, 1e10)]
    # two detections on one crowd region: both ignored, the crowd is never used up; a third below the threshold is a false positive
    mt, fl = _one_class([[0.8], [0.7], [0.3]], [1], [100.0], [100.0] * 3, thresholds=[0.5], ranges=one)
    assert mt[0, 0].tolist() == [0, 0, -1] and fl[0, 0].tolist() == [2, 2, 0]
    # a not-ignored ground truth wins over a crowd of higher IoU; the next detection then falls to the crowd
    mt, fl = _one_class([[0.6, 0.9], [0.6, 0.9]], [0, 1], [100.0] * 2, [100.0] * 2, thresholds=[0.5], ranges=one)
    assert mt[0, 0].tolist() == [0, 1] and fl[0, 0].tolist() == [1, 2]
    # ... whatever the annotation order
    mt, fl = _one_class([[0.9, 0.6], [0.9, 0.6]], [1, 0], [100.0] * 2, [100.0] * 2, thresholds=[0.5], ranges=one)
    assert mt[0, 0].tolist() == [1, 0] and fl[0, 0].tolist() == [1, 2]


def test_area_ignored_ground_truth_is_taken_once():
    """under "small" a ground truth of area 5000 is ignored but no crowd: the first detection on it is ignored, the second finds it used
    up and is a false positive -- or ignored itself if its own area lies outside the range.  Both ends of a range are inside."""
    small = [(0.0, 1024.0)]
    mt, fl = _one_class([[0.8], [0.7], [0.7]], [0], [5000.0], [100.0, 100.0, 5000.0], thresholds=[0.5], ranges=small)
    assert mt[0, 0].tolist() == [0, -1, -1] and fl[0, 0].tolist() == [2, 0, 2]
    mt, fl = _one_class([[0.8], [0.1], [0.1]], [0], [1024.0], [1024.0, 0.0, 1024.5], thresholds=[0.5], ranges=small)
    assert mt[0, 0].tolist() == [0, -1, -1] and fl[0, 0].tolist() == [1, 0, 2]


def test_equal_ious_go_to_the_last_ground_truth():
    one = [(0.0, 1e10)]
    mt, fl = _one_class([[0.6] * 5] * 3, [0] * 5, [100.0] * 5, [100.0] * 3, thresholds=[0.5], ranges=one)
    assert mt[0, 0].tolist() == [4, 3, 2] and fl[0, 0].tolist() == [1, 1, 1]
    # across the lanes of a wave and across its passes: 130 equal columns
    mt, fl = _one_class([[0.75] * 130] * 2, [0] * 130, [100.0] * 130, [100.0] * 2, thresholds=[0.5], ranges=one)
    assert mt[0, 0].tolist() == [129, 128]
    # among the ignored as well
    mt, fl = _one_class([[0.6] * 3], [1, 1, 0], [100.0, 100.0, 5000.0], [100.0], thresholds=[0.5], ranges=[(0.0, 1024.0)])
    assert mt[0, 0].tolist() == [2] and fl[0, 0].tolist() == [2]


# ---------------------------------------------------------------------------------------------------- buffers and replay
def test_strided_iou_view_and_junk_in_the_outputs():
    from ape_amd import ops
    layout = LAYOUTS[12]
    args, want = case(layout, "lattice", 3)
    dargs = [a.cuda() for a in args]
    n, m = args[0].shape
    wide = torch.ones((n, m + 5), dtype=torch.float64, device="cuda")        # what lies between the rows would match everything
    wide[:, :m] = dargs[0]
    view = wide[:, :m]
    assert not view.is_contiguous() and view.stride() == (m + 5, 1)
    nd = args[1].numel()
    match = torch.full((4, 10, nd), 12345, dtype=torch.int32, device="cuda")
    flag = torch.full((4, 10, nd), 77, dtype=torch.uint8, device="cuda")
    for _ in range(2):
        r = ops.coco_match(view, *dargs[1:], match=match, flag=flag)
        assert r[0] is match and r[1] is flag
        check((match, flag), want)
    # no detections: two empty results, nothing launched
    e = ops.coco_match(dargs[0], dargs[1][:0], dargs[2] * 0, *dargs[3:])
    assert tuple(e[0].shape) == (4, 10, 0) and tuple(e[1].shape) == (4, 10, 0)
    # no ground truth at all: every detection is unmatched, its flag its own area's
    none = ops.coco_match(dargs[0][:, :0], dargs[1], dargs[2], dargs[3][:0], dargs[4] * 0, dargs[5][:0], dargs[6][:0], dargs[7])
    lo, hi = torch.tensor(U.RANGES, dtype=torch.float64).t()
    area = args[7][args[1].long()]
    outside = ((area[None, :] < lo[:, None]) | (area[None, :] > hi[:, None])).to(torch.uint8) * 2
    assert int((none[0] != -1).sum()) == 0 and torch.equal(none[1].cpu(), outside[:, None, :].expand(4, 10, nd))


def test_call_captures_into_a_graph():
    """one kernel node, no memset: capturing runs nothing, two replays leave exactly the single-run bytes"""
    from ape_amd import ops
    args, want = case(LAYOUTS[13], "lattice", 3)
    dargs = [a.cuda() for a in args]
    thr, rng = ops.coco_match_tables("cuda")
    check(ops.coco_match(*dargs, thresholds=thr, ranges=rng), want)            # warm: nothing is set up lazily inside the capture
    nd = args[1].numel()
    match = torch.empty((4, 10, nd), dtype=torch.int32, device="cuda")
    flag = torch.empty((4, 10, nd), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.coco_match(*dargs, thresholds=thr, ranges=rng, match=match, flag=flag)
    torch.cuda.synchronize()
    match.fill_(-7)
    flag.fill_(7)
    torch.cuda.synchronize()
    assert int(match[0, 0, 0]) == -7 and int(flag[0, 0, 0]) == 7              # capturing did not run the kernel
    graph.replay()
    torch.cuda.synchronize()
    first = (match.clone(), flag.clone())
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first[0], match) and torch.equal(first[1], flag)
    check((match, flag), want)


def test_wrapper_and_library_reject_wrong_inputs():
    from ape_amd import _lib, ops
    args, _ = case(LAYOUTS[4], "lattice", 3)
    d = [a.cuda() for a in args]
    with pytest.raises(RuntimeError):
        ops.coco_match(d[0].cpu(), *d[1:])                                     # a host tensor: no CPU path
    with pytest.raises(RuntimeError):
        ops.coco_match(*d, flag=torch.zeros((4, 10, 5), dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.coco_match(*d, match=torch.zeros((4, 10, 6), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ops.coco_match(*d, flag=torch.zeros((4, 10, 5), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ops.coco_match(d[0].t().contiguous().t(), *d[1:])                      # unit stride along the rows, not the columns
    with pytest.raises(ValueError):
        ops.coco_match(d[0], d[1], d[2], torch.zeros(4097, dtype=torch.int32, device="cuda"), *d[4:])
    with pytest.raises(ValueError):
        ops.coco_match(d[0], torch.zeros(65536, dtype=torch.int32, device="cuda"), *d[2:])
    lib = _lib.load()
    ptr = torch.zeros(64, dtype=torch.float64, device="cuda").data_ptr()
    call = lambda **kw: lib.ape_hip_coco_match(*[kw.get(k, v) for k, v in (                               # noqa: E731
        ("iou", ptr), ("n", 4), ("m", 4), ("ld", 4), ("det_order", ptr), ("nd", 4), ("det_offsets", ptr), ("gt_order", ptr), ("ng", 4),
        ("gt_offsets", ptr), ("K", 1), ("gt_crowd", ptr), ("gt_area", ptr), ("det_area", ptr), ("thresholds", ptr), ("T", 1),
        ("ranges", ptr), ("A", 1), ("match", ptr), ("flag", ptr), ("stream", None))])
    assert call(ng=4097) == -1 and b"4097" in lib.ape_hip_last_error()
    assert call(nd=65536) == -1
    assert call(n=-1) == -1
    assert call(ld=3) == -1
    assert call(K=0) == -1
    assert call(match=None) == -1 and b"null" in lib.ape_hip_last_error()
    assert call(gt_area=None) == -1
    assert call(nd=0, det_order=None, match=None, flag=None) == 0              # no detections: a no-op
    assert call(T=0) == 0 and call(A=0) == 0


# ---------------------------------------------------------------------------------------------------- accumulator
H, W = 37, 53
K = 5


def _lattice_boxes(k, g):
    """corners on multiples of 4 inside a 160 x 120 image, sides multiples of 8: IoUs are ratios of small integers, and areas 64 .. 9216
    (the upper end exactly) fall in all area ranges and on their ends"""
    xy = 4.0 * torch.randint(0, 16, (k, 2), generator=g)
    wh = 8.0 * torch.randint(1, 13, (k, 2), generator=g)
    return torch.cat([xy, xy + wh], 1).double()


def _rect_masks(k, g):
    """filled rectangles in a 37 x 53 image, 4 .. 36 pixels a side before the image's edge cuts them: areas on both sides of 32 x 32"""
    y0, x0 = torch.randint(0, H - 4, (k,), generator=g), torch.randint(0, W - 4, (k,), generator=g)
    hh, ww = torch.randint(4, 37, (k,), generator=g), torch.randint(4, 37, (k,), generator=g)
    ys, xs = torch.arange(H)[None, :, None], torch.arange(W)[None, None, :]
    return ((ys >= y0[:, None, None]) & (ys < (y0 + hh)[:, None, None]) & (xs >= x0[:, None, None]) & (xs < (x0 + ww)[:, None, None])).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def _stream(kind):
    """six images on the host: (pred, scores, classes, gt, gt_classes, gt_crowd or None, gt_areas or None).  Scores are twentieths, so they
    tie within and across images; image 2 has no detections, image 4 no ground truth, image 5 (boxes) 150 detections of ONE class next to
    others -- more than the largest limit; every other image marks a third of its ground truth as crowd, every third gives its own areas"""
    sizes = [(12, 7), (30, 9), (0, 4), (25, 12), (9, 0), (40, 6)]
    g = torch.Generator().manual_seed(5 if kind == "bbox" else 6)
    make = _lattice_boxes if kind == "bbox" else _rect_masks
    images = []
    for i, (n, m) in enumerate(sizes):
        gt = make(m, g)
        gc = torch.randint(0, K - 1, (m,), generator=g)                        # class K - 1 has no ground truth anywhere
        if m > 0 and n > 0:                                                    # half of the detections are ground truth, moved or as it is
            src = torch.randint(0, m, (n // 2,), generator=g)
            near, near_c = gt[src], gc[src]
            if kind == "bbox":
                near = near + 4.0 * torch.randint(-1, 2, (n // 2, 4), generator=g)
            else:
                near = torch.roll(near, shifts=(int(torch.randint(-2, 3, (1,), generator=g)), 1), dims=(1, 2))
            pred = torch.cat([near, make(n - n // 2, g)])
            dc = torch.cat([near_c, torch.randint(0, K, (n - n // 2,), generator=g)])
        else:
            pred, dc = make(n, g), torch.randint(0, K, (n,), generator=g)
        if i == 5 and kind == "bbox":
            pred = torch.cat([pred, gt[torch.randint(0, m, (150,), generator=g)] + 4.0 * torch.randint(-1, 2, (150, 4), generator=g)])
            dc = torch.cat([dc, torch.full((150,), int(gc[0]))])
        ds = torch.randint(1, 20, (pred.shape[0],), generator=g).double() / 20
        crowd = (torch.rand(m, generator=g) < 0.34).to(torch.uint8) if i % 2 == 1 else None
        if kind == "bbox":
            box_area = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
            areas = box_area * 0.75 if i % 3 == 0 else None
        else:
            areas = gt.reshape(m, -1).sum(1).double() * 4.0 if i % 3 == 0 else None
        images.append((pred, ds, dc, gt, gc, crowd, areas))
    return images


@functools.lru_cache(maxsize=None)
def _host_scores(kind):
    from ape_amd.evaluation import coco_metrics
    records = []
    for pred, ds, dc, gt, gc, crowd, areas in _stream(kind):
        crowd = torch.zeros(len(gt), dtype=torch.uint8) if crowd is None else crowd
        iou, det_area, gt_area = (U.box_iou if kind == "bbox" else U.mask_iou)(pred, gt, crowd)
        gt_area = gt_area if areas is None else areas
        records.append(U.host_record(iou.numpy(), ds.numpy(), dc.numpy(), gc.numpy(), crowd.numpy(), gt_area.numpy(), det_area.numpy(), K))
    return coco_metrics(records, K, class_names=[f"c{k}" for k in range(K)]), records


def _same(got, want):
    assert set(got) == set(want), set(got) ^ set(want)
    for k in want:
        assert got[k] == want[k] or (got[k] != got[k] and want[k] != want[k]), (k, got[k], want[k])


@pytest.mark.parametrize("kind,form", [("bbox", "device"), ("bbox", "host"), ("bbox", "instances"), ("segm", "device"), ("segm", "host"),
                                       ("segm", "rle"), ("segm", "instances")])
def test_accumulator_equals_the_host_pipeline(kind, form):
    from ape_amd.evaluation import COCOAccumulator, coco_eval, encode_masks
    from ape_amd.structures import Boxes, Instances
    want, records = _host_scores(kind)
    assert want["images"] == 6 and want["classes"] == K - 1 and 0.0 < want["AP"] < 1.0 and want["AR@1"] < want["AR@10"] <= want["AR@100"]
    assert want["dets"] < sum(len(s[0]) for s in _stream(kind)) or kind == "segm"       # the limit cuts the 150 boxes of one class
    names = [f"c{k}" for k in range(K)]
    acc = COCOAccumulator(kind, K, class_names=names)
    dets, gts = [], []
    for pred, ds, dc, gt, gc, crowd, areas in _stream(kind):
        if form in ("device", "instances"):
            pred, ds, dc, gt, gc = pred.cuda(), ds.cuda(), dc.cuda(), gt.cuda(), gc.cuda()
            crowd, areas = None if crowd is None else crowd.cuda(), None if areas is None else areas.cuda()
        if form == "rle":
            pred = encode_masks(pred.cuda()) if len(pred) else []
            gt = encode_masks(gt.cuda()) if len(gt) else []
        if form == "instances":
            size = (120, 160) if kind == "bbox" else (H, W)
            fields = dict(pred_boxes=Boxes(pred.float() if kind == "bbox" else torch.zeros((len(pred), 4), device=ds.device)), scores=ds,
                          pred_classes=dc)
            if kind == "segm":
                fields["pred_masks"] = pred
            inst = Instances(size, **fields)
            acc.update(inst, gt=Boxes(gt) if kind == "bbox" else gt, gt_classes=gc, gt_crowd=crowd, gt_areas=areas)
            dets.append(inst)
        else:
            acc.update(pred, ds, dc, gt, gc, gt_crowd=crowd, gt_areas=areas)
            dets.append((pred, ds, dc))
        gts.append((gt, gc, crowd, areas))
    acc.reduce()                                                            # no process group: a no-op
    _same(acc.compute(), want)
    assert len(acc.records) == 6
    for (s, c, f, gc, gi), (hs, hc, hf, hgc, hgi) in zip(acc.records, records):
        assert torch.equal(s, hs) and torch.equal(c, hc) and torch.equal(f, hf) and torch.equal(gc, hgc) and torch.equal(gi, hgi)
    _same(coco_eval(dets, gts, kind, class_names=names), want)              # the one-call form


def test_crowd_mask_iou_is_inter_over_area_det():
    """mask IoU is a ratio of integer counts: inter / union, and inter / area_det in a crowd column, the float64 quotient exactly"""
    from ape_amd import ops
    from ape_amd.evaluation import _coco_count_iou
    g = torch.Generator().manual_seed(3)
    a, b = _rect_masks(9, g), _rect_masks(7, g)
    a[8] = 0                                                                # an empty detection: 0 / 0 is 0 in either kind of column
    crowd = torch.tensor([0, 1, 0, 1, 1, 0, 1], dtype=torch.uint8)
    a_bits, area_a = ops.mask_pack_bits(a.cuda())
    b_bits, area_b = ops.mask_pack_bits(b.cuda())
    inter = ops.bitmask_pair_counts(a_bits, b_bits)
    got = _coco_count_iou(inter, area_a, area_b, crowd.cuda() != 0).cpu()
    want, det_area, gt_area = U.mask_iou(a, b, crowd)
    assert torch.equal(got, want) and torch.equal(area_a.cpu().double(), det_area) and torch.equal(area_b.cpu().double(), gt_area)
    inter, area_a, area_b = inter.cpu(), area_a.cpu(), area_b.cpu()
    for i in range(9):
        for j in range(7):
            den = int(area_a[i]) if crowd[j] else int(area_a[i]) + int(area_b[j]) - int(inter[i, j])
            assert float(got[i, j]) == (int(inter[i, j]) / den if den else 0.0)
    assert int((inter > 0).sum()) > 5 and float(got[:, crowd != 0].max()) > float(U.mask_iou(a, b, crowd * 0)[0][:, crowd != 0].max())


@pytest.mark.parametrize("kind", ["bbox", "segm"])
def test_update_with_device_inputs_does_not_synchronise(kind):
    from ape_amd.evaluation import COCOAccumulator
    want, _ = _host_scores(kind)
    dev = [tuple(None if t is None else t.cuda() for t in s) for s in _stream(kind)]
    acc = COCOAccumulator(kind, K, device="cuda", class_names=[f"c{k}" for k in range(K)])
    pred, ds, dc, gt, gc, crowd, areas = dev[0]
    acc.update(pred, ds, dc, gt, gc, gt_crowd=crowd, gt_areas=areas)          # the first call loads the library and the tables
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for pred, ds, dc, gt, gc, crowd, areas in dev[1:]:
            acc.update(pred, ds, dc, gt, gc, gt_crowd=crowd, gt_areas=areas)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _same(acc.compute(), want)


def test_classes_out_of_range_on_the_device_raise_in_compute():
    from ape_amd.evaluation import COCOAccumulator
    g = torch.Generator().manual_seed(1)
    boxes = _lattice_boxes(4, g).cuda()
    acc = COCOAccumulator("bbox", 3)
    acc.update(boxes, torch.rand(4).cuda(), torch.tensor([0, 1, 3, 2]).cuda(), boxes, torch.tensor([0, 1, 2, 2]).cuda())
    with pytest.raises(ValueError):
        acc.compute()
