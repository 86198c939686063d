"""-m gpu: `ops.box_cover_overlaps` (csrc/boxcover.hip) for exact equality -- overlaps AND matched rows -- with a host restatement of the
greedy coverage loop in float32, over shapes, tie-rich lattice boxes and generic float boxes, duplicates, area boundaries, limits,
unaligned views, result reuse and a captured graph; `ProposalRecallAccumulator` against `proposal_recall_metrics` of the host's tables;
and the scores end to end on the tiny fixture model.  No tolerances anywhere."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 5), (5, 1), (7, 5), (5, 7), (63, 3), (65, 64), (300, 17), (1000, 40), (1100, 40)]
RANGES = [(0.0, 1e5 ** 2), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e5 ** 2)]       # all, small, medium, large
COMBOS = [(lo, hi, limit) for limit in (100, 1000) for lo, hi in RANGES]
KEYS = ["AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", "ARs@1000", "ARm@1000", "ARl@1000"]


# ---------------------------------------------------------------------------------------------------- the host's word
def host_iou(p, g):
    """[n, m] float32 on the CPU, one rounding per operation: area = (x2 - x1) * (y2 - y1), inter = max(.., 0) * max(.., 0),
    inter / ((area_p + area_g) - inter) where the boxes intersect, 0 elsewhere"""
    p, g = p.float().cpu(), g.float().cpu()
    area_p = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    area_g = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    w = (torch.minimum(p[:, None, 2], g[None, :, 2]) - torch.maximum(p[:, None, 0], g[None, :, 0])).clamp_min(0)
    h = (torch.minimum(p[:, None, 3], g[None, :, 3]) - torch.maximum(p[:, None, 1], g[None, :, 1])).clamp_min(0)
    inter = w * h
    union = (area_p[:, None] + area_g[None, :]) - inter
    hit = inter > 0
    return torch.where(hit, inter / torch.where(hit, union, torch.ones_like(union)), torch.zeros_like(inter))


def host_cover(p, g, areas, combos=COMBOS):
    """(overlaps float32 [C, m], match int32 [C, m]) as the definition gives them: per combination the ground truth with lo <= area <= hi
    against the first `limit` proposals; as often as the smaller side allows, take each column's maximum over the rows (first index of
    a tie), then the maximum of those (first index of a tie), record it and blank its row and its column"""
    p, g, areas = p.float().cpu(), g.float().cpu(), areas.float().cpu()
    m = g.shape[0]
    ov = torch.full((len(combos), m), -1.0, dtype=torch.float32)
    mt = torch.full((len(combos), m), -1, dtype=torch.int32)
    for c, (lo, hi, limit) in enumerate(combos):
        inside = (areas >= torch.tensor(lo, dtype=torch.float32)) & (areas <= torch.tensor(hi, dtype=torch.float32))
        cols = inside.nonzero().flatten()
        ov[c, cols] = 0.0
        rows = p[:limit] if limit > 0 else p
        if rows.shape[0] == 0 or cols.numel() == 0:
            continue
        table = host_iou(rows, g[cols])
        for _ in range(min(table.shape)):
            best, best_row = table.max(dim=0)
            value, col = best.max(dim=0)
            row = int(best_row[col])
            ov[c, cols[col]] = value
            mt[c, cols[col]] = row
            table[row, :] = -1
            table[:, col] = -1
    return ov, mt


def box_area(b):
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def lattice_boxes(k, seed):
    """corners on multiples of 4, sizes multiples of 8, inside 0 .. 320: IoUs are ratios of small integers, and some tie (the
    crowded lattices of `test_tie_rule_on_crowded_lattices` tie everywhere); areas from 64 to 16384 fall in all three area classes"""
    g = torch.Generator().manual_seed(seed)
    xy = 4.0 * torch.randint(0, 48, (k, 2), generator=g)
    wh = 8.0 * torch.randint(1, 17, (k, 2), generator=g)
    return torch.cat([xy, xy + wh], 1).float()


def generic_boxes(k, seed):
    """float corners in 0 .. 2048, sides 1 .. 200: no two IoUs tie, and a fused multiply-add or a division that is not correctly rounded
    shows in a last bit"""
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand((k, 2), generator=g) * 1800
    wh = torch.rand((k, 2), generator=g) * 199 + 1
    return torch.cat([xy, xy + wh], 1).float()


@functools.lru_cache(maxsize=None)
def case(n, m, family):
    """(proposals, gt, overlaps, match) on the host, computed once per case and shared"""
    make = {"lattice": lattice_boxes, "generic": generic_boxes}[family]
    p, g = make(n, 1000 * n + m), make(m, 2000 * n + m + 1)
    ov, mt = host_cover(p, g, box_area(g))
    return p, g, ov, mt


def check(got, want, what=""):
    (ov, mt), (hov, hmt) = got, want
    assert ov.dtype == torch.float32 and mt.dtype == torch.int32 and ov.is_cuda and mt.is_cuda
    assert tuple(ov.shape) == tuple(hov.shape) and tuple(mt.shape) == tuple(hmt.shape)
    bad = (ov.cpu() != hov).nonzero()
    assert bad.numel() == 0, (what, "overlaps", bad[:5].tolist(), ov.cpu()[tuple(bad[0])].item(), hov[tuple(bad[0])].item())
    assert torch.equal(mt.cpu(), hmt), (what, "match", (mt.cpu() != hmt).nonzero()[:5].tolist())


# ---------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("family", ["lattice", "generic"])
@pytest.mark.parametrize("nm", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_overlaps_and_matches_equal_the_host_loop(nm, family):
    from ape_amd import ops
    p, g, hov, hmt = case(nm[0], nm[1], family)
    got = ops.box_cover_overlaps(p.cuda(), g.cuda())
    check(got, (hov, hmt), (nm, family))
    if family == "lattice" and min(nm) >= 5:
        assert int((hov[0] > 0).sum()) > 0                       # the case is not vacuous: something overlaps


@pytest.mark.parametrize("nm", [(40, 1100), (3, 4096), (65535, 3), (2100, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes_past_one_pass_and_at_the_limits_of_a_call(nm):
    """more ground truth than the workgroup has threads (1024: columns are walked in several passes), the most a call takes on either
    side, and more proposals than any limit; the second set of rows is unlimited here"""
    from ape_amd import ops
    n, m = nm
    p, g = lattice_boxes(n, 3000 + n), lattice_boxes(m, 4000 + m)
    combos = [(lo, hi, limit) for limit in (1000, 0) for lo, hi in RANGES]
    got = ops.box_cover_overlaps(p.cuda(), g.cuda(), limits=[1000, 0])
    check(got, host_cover(p, g, box_area(g), combos), nm)


def _last_index_cover(p, g):
    """the same loop with the LAST index of a tie, rows and columns: what the tie rule is pinned against"""
    table = host_iou(p, g)
    n, m = table.shape
    ov, mt = torch.zeros(m), torch.full((m,), -1, dtype=torch.int32)
    for _ in range(min(n, m)):
        best, best_row = table.flip(0).max(dim=0)
        value, col = best.flip(0).max(dim=0)
        col = m - 1 - int(col)
        row = n - 1 - int(best_row[col])
        ov[col], mt[col] = value, row
        table[row, :] = -1
        table[:, col] = -1
    return ov, mt


def test_tie_rule_on_crowded_lattices():
    """40 problems of 7 x 5 boxes with sides 8 / 16 / 24 on a 4-pixel lattice of 8 positions: equal IoUs everywhere.  With the last index
    of a tie most of them get other rows, and a quarter other overlaps (a check on the data, on the host) -- the device's equal the
    first-index loop's in all of them"""
    from ape_amd import ops

    def crowded(k, seed):
        g = torch.Generator().manual_seed(seed)
        xy = 4.0 * torch.randint(0, 8, (k, 2), generator=g)
        return torch.cat([xy, xy + 8.0 * torch.randint(1, 4, (k, 2), generator=g)], 1).float()
    other_rows = other_overlaps = 0
    for s in range(40):
        p, g = crowded(7, 500 + s), crowded(5, 600 + s)
        want = host_cover(p, g, box_area(g))
        lov, lmt = _last_index_cover(p, g)
        other_rows += not torch.equal(lmt, want[1][0])
        other_overlaps += not torch.equal(lov.sort().values, want[0][0].sort().values)
        check(ops.box_cover_overlaps(p.cuda(), g.cuda()), want, s)
    assert other_rows >= 20 and other_overlaps >= 5, (other_rows, other_overlaps)


def test_fewer_rows_than_ground_truth():
    """(5, 7): exactly 5 columns of the all-areas row are recorded, with 5 distinct rows; the other two stay (0, -1)"""
    from ape_amd import ops
    for family in ("lattice", "generic"):
        p, g, hov, hmt = case(5, 7, family)
        ov, mt = ops.box_cover_overlaps(p.cuda(), g.cuda())
        mt = mt.cpu()
        assert int((mt[0] >= 0).sum()) == 5 and sorted(mt[0][mt[0] >= 0].tolist()) == [0, 1, 2, 3, 4]
        assert ov.cpu()[0][mt[0] < 0].tolist() == [0.0, 0.0]
        check((ov, mt.cuda()), (hov, hmt))


def test_duplicates_disjoint_boxes_and_empty_ranges():
    from ape_amd import ops
    # every proposal twice, every ground truth twice: the second copy of a ground truth gets the second copy of its proposal
    p, g = lattice_boxes(9, 11), lattice_boxes(6, 12)
    p2, g2 = torch.cat([p, p]), torch.cat([g, g])
    want = host_cover(p2, g2, box_area(g2))
    check(ops.box_cover_overlaps(p2.cuda(), g2.cuda()), want, "duplicates")
    same = torch.cat([g, g])                                     # proposals = ground truth, doubled: every overlap is 1
    ov, mt = ops.box_cover_overlaps(same.cuda(), same.cuda())
    assert ov.cpu()[0].tolist() == [1.0] * 12 and sorted(mt.cpu()[0].tolist()) == list(range(12))
    check((ov, mt), host_cover(same, same, box_area(same)), "identical")
    # all disjoint: every IoU is 0, and the rule alone decides -- round k gives column k row k
    p = torch.tensor([[100.0 * i, 0.0, 100.0 * i + 40, 40.0] for i in range(6)])
    g = torch.tensor([[100.0 * i, 500.0, 100.0 * i + 40, 540.0] for i in range(4)])
    ov, mt = ops.box_cover_overlaps(p.cuda(), g.cuda())
    assert ov.cpu()[0].tolist() == [0.0] * 4 and mt.cpu()[0].tolist() == [0, 1, 2, 3]
    check((ov, mt), host_cover(p, g, box_area(g)), "disjoint")
    # ground truth of 40 x 40 = 1600 only: medium.  The small and large rows are all -1
    assert ov.cpu()[1].tolist() == [-1.0] * 4 and ov.cpu()[3].tolist() == [-1.0] * 4
    assert mt.cpu()[1].tolist() == [-1] * 4 and mt.cpu()[3].tolist() == [-1] * 4 and ov.cpu()[2].tolist() == [0.0] * 4


def test_area_boundaries_are_inclusive_in_float32():
    """areas of exactly 32^2 and 96^2 count in both adjacent ranges; one float32 ulp outside, in one only"""
    from ape_amd import ops
    inf = torch.tensor(float("inf"))
    a32, a96 = torch.tensor(1024.0), torch.tensor(9216.0)
    areas = torch.stack([a32, torch.nextafter(a32, -inf), torch.nextafter(a32, inf), a96, torch.nextafter(a96, -inf),
                         torch.nextafter(a96, inf), torch.tensor(0.0), torch.tensor(1e10)]).float()
    g = lattice_boxes(8, 21)
    p = lattice_boxes(20, 22)
    ov, mt = ops.box_cover_overlaps(p.cuda(), g.cuda(), gt_areas=areas.cuda())
    inside = (ov.cpu()[:4] >= 0).int().tolist()
    #                1024  -ulp  +ulp  9216  -ulp  +ulp  0  1e10
    assert inside == [[1, 1, 1, 1, 1, 1, 1, 1],
                      [1, 1, 0, 0, 0, 0, 1, 0],
                      [1, 0, 1, 1, 1, 0, 0, 0],
                      [0, 0, 0, 1, 0, 1, 0, 1]]
    check((ov, mt), host_cover(p, g, areas), "boundaries")


def test_limits_cut_the_proposals():
    """n = 1100: rows 0 .. 3 (limit 100) equal a call on the first 100 proposals alone, rows 4 .. 7 one on the first 1000, and neither
    equals the unlimited result; no matched row lies behind its limit"""
    from ape_amd import ops
    for family in ("lattice", "generic"):
        p, g, hov, hmt = case(1100, 40, family)
        dp, dg = p.cuda(), g.cuda()
        ov, mt = ops.box_cover_overlaps(dp, dg)
        for rows, limit in ((slice(0, 4), 100), (slice(4, 8), 1000)):
            sov, smt = ops.box_cover_overlaps(dp[:limit].contiguous(), dg, limits=[0])
            assert torch.equal(ov[rows], sov) and torch.equal(mt[rows], smt)
            assert int(mt[rows].max()) < limit
        fov, fmt = ops.box_cover_overlaps(dp, dg, limits=[0, -1])             # <= 0: no limit
        assert torch.equal(fov[:4], fov[4:]) and int(fmt.max()) >= 1000 and not torch.equal(fov[:4], ov[4:])
        check((fov, fmt), host_cover(p, g, box_area(g), [(lo, hi, 0) for _ in range(2) for lo, hi in RANGES]), "unlimited")


def test_explicit_ranges_and_limits_tensors():
    from ape_amd import ops
    p, g, _, _ = case(300, 17, "lattice")
    combos = [(0.0, 1e10, 7), (2000.0, 1e10, 0), (5.0, 6.0, 50), (0.0, 2000.0, 300), (0.0, 1e10, 1)]
    ranges = torch.tensor([[lo, hi] for lo, hi, _ in combos], dtype=torch.float32, device="cuda")
    limits = torch.tensor([k for _, _, k in combos], dtype=torch.int32, device="cuda")
    got = ops.box_cover_overlaps(p.cuda(), g.cuda(), ranges=ranges, limits=limits)
    assert tuple(got[0].shape) == (5, 17)
    check(got, host_cover(p, g, box_area(g), combos), "explicit")


def test_unaligned_views_read_nothing_outside():
    """proposals, ground truth and areas as views 4 bytes into larger buffers: around the boxes the buffers go on with boxes
    (0, 0, 4096, 4096), which overlap everything, around the areas with 1500 (medium) -- a row or a column read before or behind an input
    would take part in the assignment"""
    from ape_amd import ops
    for n, m in ((7, 5), (65, 64), (300, 17)):
        p, g, hov, hmt = case(n, m, "lattice")

        def view(t, boxes):
            k = t.numel() + 17
            if boxes:
                buf = torch.where((torch.arange(k) - 1) % 4 < 2, 0.0, 4096.0).float().cuda()
            else:
                buf = torch.full((k,), 1500.0, dtype=torch.float32, device="cuda")
            buf[1: 1 + t.numel()] = t.reshape(-1).cuda()
            v = buf[1: 1 + t.numel()].view(t.shape)
            assert v.is_contiguous() and v.data_ptr() % 16 == 4
            return v
        check(ops.box_cover_overlaps(view(p, True), view(g, True), gt_areas=view(box_area(g), False)), (hov, hmt), (n, m))


def test_out_and_match_are_overwritten_entirely():
    from ape_amd import ops
    p, g, hov, hmt = case(65, 64, "generic")
    dp, dg = p.cuda(), g.cuda()
    out = torch.full((8, 64), float("nan"), dtype=torch.float32, device="cuda")
    match = torch.full((8, 64), 12345, dtype=torch.int32, device="cuda")
    for _ in range(2):
        r = ops.box_cover_overlaps(dp, dg, out=out, match=match)
        assert r[0] is out and r[1] is match
        check((out, match), (hov, hmt))
    # no proposals: in-range ground truth gets (0, -1), the rest (-1, -1) -- also into junk
    out.fill_(float("nan"))
    match.fill_(777)
    ops.box_cover_overlaps(dp[:0], dg, out=out, match=match)
    assert torch.equal(out.cpu(), torch.where(hov >= 0, torch.zeros_like(hov), hov)) and int((match != -1).sum()) == 0
    # no ground truth: two empty results
    e = ops.box_cover_overlaps(dp, dg[:0])
    assert tuple(e[0].shape) == (8, 0) and tuple(e[1].shape) == (8, 0)


def test_wrapper_rejects_wrong_inputs():
    from ape_amd import ops
    p, g = lattice_boxes(5, 1).cuda(), lattice_boxes(3, 2).cuda()
    with pytest.raises(TypeError):
        ops.box_cover_overlaps(p.double(), g)
    with pytest.raises(TypeError):
        ops.box_cover_overlaps(p, g.half())
    with pytest.raises(TypeError):
        ops.box_cover_overlaps(p, g, gt_areas=box_area(g).double())
    with pytest.raises(ValueError):
        ops.box_cover_overlaps(p[:, :3].contiguous(), g)
    with pytest.raises(ValueError):
        ops.box_cover_overlaps(p, g[:, [0, 1, 2, 3, 0]][:, :4])                 # [3, 4] with a row stride of 5
    with pytest.raises(ValueError):
        ops.box_cover_overlaps(p, g, gt_areas=box_area(p))                      # [5] for 3 boxes
    with pytest.raises(ValueError):
        ops.box_cover_overlaps(p, g, out=torch.zeros((8, 4), device="cuda"))
    with pytest.raises(ValueError):
        ops.box_cover_overlaps(p, g, out=torch.zeros((8, 3), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ops.box_cover_overlaps(p, g, match=torch.zeros((8, 3), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ops.box_cover_overlaps(p, g, match=torch.zeros((8, 6), dtype=torch.int32, device="cuda")[:, ::2])
    with pytest.raises(ValueError):
        ops.box_cover_overlaps(p, g, ranges=torch.zeros((2, 2), device="cuda"))                  # a tensor on one side only
    with pytest.raises(ValueError):
        ops.box_cover_overlaps(p, g, ranges=torch.zeros((2, 2), device="cuda"), limits=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ops.box_cover_overlaps(p, torch.zeros((4097, 4), device="cuda"))        # more ground truth than a call takes
    with pytest.raises(ValueError):
        ops.box_cover_overlaps(torch.zeros((65536, 4), device="cuda"), g)
    with pytest.raises(RuntimeError):
        ops.box_cover_overlaps(p.cpu(), g)                                      # a host tensor: no CPU path
    with pytest.raises(RuntimeError):
        ops.box_cover_overlaps(p, g, out=torch.zeros((8, 3)))
    with pytest.raises(RuntimeError):
        ops.box_cover_overlaps(p, g, ranges=torch.zeros((2, 2)), limits=torch.zeros(2, dtype=torch.int32))
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            ops.box_cover_overlaps(p, g.to("cuda:1"))


def test_library_rejects_what_the_wrapper_would():
    """the C entry checks for itself: sizes past its limits, negative sizes and null pointers are argument errors, not launches"""
    from ape_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    ptr = buf.data_ptr()
    assert lib.ape_hip_box_cover_overlaps(ptr, 4, ptr, ptr, 4097, ptr, ptr, 1, ptr, ptr, None) == -1
    assert b"4097" in lib.ape_hip_last_error()
    assert lib.ape_hip_box_cover_overlaps(ptr, 65536, ptr, ptr, 4, ptr, ptr, 1, ptr, ptr, None) == -1
    assert lib.ape_hip_box_cover_overlaps(ptr, -1, ptr, ptr, 4, ptr, ptr, 1, ptr, ptr, None) == -1
    assert lib.ape_hip_box_cover_overlaps(None, 4, ptr, ptr, 4, ptr, ptr, 1, ptr, ptr, None) == -1
    assert b"null" in lib.ape_hip_last_error()
    assert lib.ape_hip_box_cover_overlaps(ptr, 4, ptr, ptr, 4, ptr, ptr, 1, None, ptr, None) == -1
    assert lib.ape_hip_box_cover_overlaps(None, 4, None, None, 0, None, None, 1, None, None, None) == 0       # m == 0: a no-op
    assert lib.ape_hip_box_cover_overlaps(None, 4, None, None, 4, None, None, 0, None, None, None) == 0       # C == 0: a no-op


def test_call_captures_into_a_graph():
    """a single-branch graph of one kernel node: capturing runs nothing, two replays leave exactly the single-run result"""
    from ape_amd import ops
    p, g, hov, hmt = case(300, 17, "lattice")
    dp, dg = p.cuda(), g.cuda()
    areas = box_area(dg)
    check(ops.box_cover_overlaps(dp, dg, gt_areas=areas), (hov, hmt))           # warm: nothing is set up lazily inside the capture
    out = torch.empty((8, 17), dtype=torch.float32, device="cuda")
    match = torch.empty((8, 17), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.box_cover_overlaps(dp, dg, gt_areas=areas, out=out, match=match)
    torch.cuda.synchronize()
    out.fill_(-7.0)
    match.fill_(-7)
    torch.cuda.synchronize()
    assert float(out[0, 0]) == -7.0 and int(match[0, 0]) == -7                  # capturing did not run the kernel
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    check((out, match), (hov, hmt))


# ---------------------------------------------------------------------------------------------------- accumulator
def _stream():
    """12 images of mixed (n, m) on the host: (boxes, logits, gt_boxes, gt_areas or None).  Logits are tenths, so scores tie within an
    image and the stable order decides which of two equal-score boxes lies inside a limit; image 3 has no proposals, image 7 no ground
    truth; image 9 has more than 100 and image 10 more than 1000 proposals"""
    sizes = [(7, 5), (5, 7), (63, 3), (0, 4), (65, 64), (1, 1), (300, 17), (20, 0), (40, 40), (150, 30), (1100, 12), (12, 9)]
    g = torch.Generator().manual_seed(9)
    images = []
    for i, (n, m) in enumerate(sizes):
        make = generic_boxes if i % 3 == 2 else lattice_boxes
        boxes, gt = make(n, 300 + i), make(m, 400 + i)
        logits = torch.randint(0, 10, (n,), generator=g).float() / 10
        areas = (box_area(gt) * 0.75).float() if i % 2 == 1 else None          # a segment's area is not its box's
        images.append((boxes, logits, gt, areas))
    return images


@functools.lru_cache(maxsize=None)
def _host_tables():
    from ape_amd.evaluation import proposal_recall_metrics, proposal_recall_thresholds
    thr = proposal_recall_thresholds()
    counts, num_pos, seen = torch.zeros((8, 10), dtype=torch.int64), torch.zeros(8, dtype=torch.int64), 0
    for boxes, logits, gt, areas in _stream():
        seen += 1
        if boxes.shape[0] == 0 or gt.shape[0] == 0:
            continue
        order = torch.sort(logits, descending=True, stable=True)[1]
        ov, _ = host_cover(boxes[order], gt, box_area(gt) if areas is None else areas)
        counts += (ov[:, :, None] >= thr).sum(1)
        num_pos += (ov >= 0).sum(1)
    return proposal_recall_metrics(counts, num_pos, images=seen, thresholds=thr), counts, num_pos


def _same(got, want):
    assert set(got) == set(want), set(got) ^ set(want)
    for k in want:
        assert got[k] == want[k] or (got[k] != got[k] and want[k] != want[k]), (k, got[k], want[k])


@pytest.mark.parametrize("form", ["device", "host", "proposals", "detections"])
def test_accumulator_on_a_stream_of_images(form):
    """tensors on the device, tensors on the host, `Instances` with proposal_boxes + objectness_logits and with pred_boxes + scores:
    every key equals `proposal_recall_metrics` of the host's tables"""
    from ape_amd.evaluation import ProposalRecallAccumulator, proposal_recall
    from ape_amd.structures import Boxes, Instances
    want, counts, num_pos = _host_tables()
    assert set(want) == set(KEYS) | {"images", "gt", "thresholds"} and want["images"] == 12 and want["gt"] == int(num_pos[0])
    assert 0.0 < want["AR@100"] < want["AR@1000"] < 100.0       # the limit matters in this stream
    acc = ProposalRecallAccumulator()
    listed = []
    for boxes, logits, gt, areas in _stream():
        if form == "device":
            boxes, logits, gt, areas = boxes.cuda(), logits.cuda(), gt.cuda(), None if areas is None else areas.cuda()
        if form in ("device", "host"):
            acc.update(None, gt, areas, boxes=boxes, logits=logits)
            listed.append(((boxes, logits), gt, areas))
            continue
        if form == "proposals":
            inst = Instances((2048, 2048), proposal_boxes=Boxes(boxes), objectness_logits=logits)
        else:
            inst = Instances((2048, 2048), pred_boxes=Boxes(boxes.cuda()), scores=logits.cuda())
        acc.update(inst, Boxes(gt), areas)
        listed.append((inst, gt, areas) if areas is not None else (inst, gt))
    assert acc.counts.is_cuda and acc.counts.dtype == torch.int64 and acc.num_pos.dtype == torch.int64
    assert torch.equal(acc.counts.cpu(), counts) and torch.equal(acc.num_pos.cpu(), num_pos)
    acc.reduce()                                                # no process group: a no-op
    _same(acc.compute(), want)
    _same(proposal_recall(listed), want)                        # the one-call form


def test_stable_order_decides_among_equal_scores():
    """150 proposals of ONE score: the limit-100 rows see the first 100 in input order, whatever an unstable sort would do"""
    from ape_amd.evaluation import ProposalRecallAccumulator
    boxes, gt = lattice_boxes(150, 71), lattice_boxes(30, 72)
    acc = ProposalRecallAccumulator()
    acc.update(None, gt.cuda(), boxes=boxes.cuda(), logits=torch.full((150,), 0.5, device="cuda"))
    ov, _ = host_cover(boxes, gt, box_area(gt))
    thr = acc.thresholds
    assert torch.equal(acc.counts.cpu(), (ov[:, :, None] >= thr).sum(1)) and torch.equal(acc.num_pos.cpu(), (ov >= 0).sum(1))


def test_update_with_device_inputs_does_not_synchronise():
    from ape_amd.evaluation import ProposalRecallAccumulator
    want, counts, num_pos = _host_tables()
    dev = [(b.cuda(), l.cuda(), g.cuda(), None if a is None else a.cuda()) for b, l, g, a in _stream()]
    acc = ProposalRecallAccumulator(device="cuda")
    acc.update(None, dev[0][2], dev[0][3], boxes=dev[0][0], logits=dev[0][1])  # the first call loads the library and the combinations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for boxes, logits, gt, areas in dev[1:]:
            acc.update(None, gt, areas, boxes=boxes, logits=logits)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(acc.counts.cpu(), counts) and torch.equal(acc.num_pos.cpu(), num_pos)
    _same(acc.compute(), want)


# ---------------------------------------------------------------------------------------------------- end to end
def test_proposal_recall_end_to_end():
    """the tiny square fixture on the device in float32.  Its own detections as ground truth are covered completely: AR@100 is 100;
    the same ground truth moved outside the image is not covered at all: 0"""
    import model_util as M
    from ape_amd.evaluation import ProposalRecallAccumulator, proposal_recall
    model, orc, image, text, gold = M.build_pair("tiny_square", device="cuda", dtype=torch.float32)
    h, w = image.shape[-2:]
    inst = model([{"image": image.cuda(), "height": h, "width": w, "text_features": text.cuda()}])[0]["instances"]
    boxes = inst.pred_boxes.tensor
    first = boxes[torch.sort(inst.scores, descending=True, stable=True)[1][:100]]               # AR@100 looks at the first 100
    gt = first[(first[:, 2] > first[:, 0]) & (first[:, 3] > first[:, 1])].clone()               # an empty box covers nothing, itself included
    print(f"[proposals] {len(inst)} detections, {gt.shape[0]} of the first {first.shape[0]} with a non-empty box as ground truth")
    assert gt.shape[0] > 0
    acc = ProposalRecallAccumulator()
    acc.update(inst, gt)
    r = acc.compute()
    assert r["AR@100"] == 100.0 and r["AR@1000"] == 100.0 and r["images"] == 1 and r["gt"] == gt.shape[0]
    _same(proposal_recall([(inst, gt)]), r)
    moved = gt + torch.tensor([10.0 * w, 10.0 * h, 10.0 * w, 10.0 * h])
    away = proposal_recall([(inst, moved)])
    assert away["AR@100"] == 0.0 and away["AR@1000"] == 0.0 and away["gt"] == gt.shape[0]
