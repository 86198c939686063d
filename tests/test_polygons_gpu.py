"""ops.poly_rasterize (csrc/polygon.hip) against tests/polygon_refs.py, the rleFrPoly restatement: masks and areas EQUAL, on the smallest
shapes that can break each stage -- the toggle pass (one wave per edge, 64 points per step), the fill pass (1024 words = 65536 pixels per
chunk) and the output pass (16-byte pieces at any address)."""
import numpy as np
import pytest
import torch

import polygon_refs as pr
from test_polygon_refs import LITERAL

pytestmark = pytest.mark.gpu

FILL_CHUNK = 1024 * 64                                        # pixels per chunk of the fill pass (PF_THREADS words)


def reference(objs, H, W):
    return torch.from_numpy(np.stack([pr.segm_mask_ref(p, H, W) for p in objs])) if objs else torch.zeros((0, H, W), dtype=torch.uint8)


def rasterize(objs, H, W, out=None):
    from ape_amd import ops
    from ape_amd.evaluation import pack_polygons
    xy, vo, po = pack_polygons(objs)
    return ops.poly_rasterize(xy.cuda(), vo.cuda(), po.cuda(), H, W, out=out)


def check(objs, H, W, want=None):
    want = reference(objs, H, W) if want is None else want
    masks, area = rasterize(objs, H, W)
    assert masks.dtype == torch.uint8 and tuple(masks.shape) == (len(objs), H, W) and area.dtype == torch.int64
    got = masks.cpu()
    assert torch.equal(got, want), [(i, int((got[i] != want[i]).sum())) for i in range(len(objs)) if not torch.equal(got[i], want[i])]
    assert torch.equal(area.cpu(), want.flatten(1).sum(1, dtype=torch.int64))
    return want


# ------------------------------------------------------------------------------------------------ polygons
def tenths(rng, H, W, k):
    """multiples of 0.1: 5 x + .5 lands on integers (or a hair beside them)"""
    return (np.round(np.stack([rng.uniform(-0.25 * W, 1.25 * W, k), rng.uniform(-0.25 * H, 1.25 * H, k)], 1) * 10) / 10).reshape(-1).tolist()


def cents(rng, H, W, k):
    """two decimals, COCO's precision"""
    return np.round(np.stack([rng.uniform(-0.25 * W, 1.25 * W, k), rng.uniform(-0.25 * H, 1.25 * H, k)], 1), 2).reshape(-1).tolist()


def ties(rng, H, W, k):
    """integer vertices joined by edges with dx = 2 dy or dy = 2 dx: s * t + .5 hits halves all along the edge"""
    p = np.array([rng.integers(0, W + 1), rng.integers(0, H + 1)])
    out = [p.copy()]
    for _ in range(k - 1):
        a = int(rng.integers(1, max(2, min(H, W) // 3)))
        step = np.array([2 * a, a]) if rng.integers(0, 2) else np.array([a, 2 * a])
        p = p + step * rng.choice([-1, 1], 2)
        out.append(p.copy())
    return np.stack(out).astype(np.float64).reshape(-1).tolist()


def family_objects(H, W, seed):
    """six objects, two of each family, 3 .. 9 vertices, vertices in and out of the image"""
    rng = np.random.default_rng(seed)
    return [[f(rng, H, W, int(rng.integers(3, 10)))] for f in (tenths, cents, ties, tenths, cents, ties)]


# ------------------------------------------------------------------------------------------------ 1. known answers
@pytest.mark.parametrize("h,w,xy,runs", LITERAL)
def test_literal_cases(h, w, xy, runs):
    want = torch.from_numpy(pr.runs_to_mask(runs, h, w))[None]
    check([[xy]], h, w, want)


# ------------------------------------------------------------------------------------------------ 2. tiny masks, exact bytes
@pytest.mark.parametrize("h,w,objs", [(1, 1, [[[0, 0, 1, 0, 1, 1, 0, 1]], [[0.2, 0.2, 0.4, 0.2, 0.4, 0.4]], []]),
                                      (3, 7, [[[0.5, 0.5, 6.5, 0.5, 6.5, 2.5, 0.5, 2.5]], [[1, 0, 7, 3, 0, 3]], [[-2, -2, 9, -1, 8, 5, -1, 4]]]),
                                      (8, 8, [[[4, 4, 8, 4, 8, 8, 4, 8]], [[0, 0, 8, 0, 8, 8, 0, 8]], [[1.5, 2.5, 6.25, 3, 4, 7.75]]])])
def test_small_masks_write_exactly_their_bytes(h, w, objs):
    """H * W < 64 (one partial word), H * W == 64 with a polygon that records index 64; `out` inside a buffer of canary bytes, at an
    aligned and at an odd address: the n * H * W bytes are written, no byte beside them"""
    want = check(objs, h, w)
    total = len(objs) * h * w
    for offset in (16, 17, 31):
        buf = torch.full((total + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        out = buf[offset: offset + total].view(len(objs), h, w)
        masks, area = rasterize(objs, h, w, out=out)
        assert masks.data_ptr() == out.data_ptr()
        host = buf.cpu()
        assert torch.equal(host[offset: offset + total].view(len(objs), h, w), want), offset
        assert bool((host[:offset] == 0xAB).all()) and bool((host[offset + total:] == 0xAB).all()), offset
        assert torch.equal(area.cpu(), want.flatten(1).sum(1))


# ------------------------------------------------------------------------------------------------ 3. the three families, by size
@pytest.mark.parametrize("h,w", [(37, 53), (64, 64), (65, 3), (3, 65), (255, 257), (256, 256), (241, 272), (257, 256), (200, 333)])
def test_coordinate_families_at_word_and_chunk_edges(h, w):
    """columns that straddle 64-bit words (37 x 53, 65 x 3), whole words (64 x 64), and the fill pass's chunk of 65536 pixels from both
    sides: 65535 pixels, 65536, one word more (241 x 272 = 1025 words), a few more (257 x 256) and 200 x 333"""
    if h * w > 60000:
        assert {255 * 257, 256 * 256} == {FILL_CHUNK - 1, FILL_CHUNK} and -(-241 * 272 // 64) == FILL_CHUNK // 64 + 1
    check(family_objects(h, w, 1000 * h + w), h, w)


# ------------------------------------------------------------------------------------------------ 4. where the polygon lies
def test_vertices_outside_on_every_side_empty_and_full():
    H, W = 20, 30
    objs = [[[-6, 5, 12, 4.5, 11.25, 14, -3, 15]],                             # out on the left
            [[18, 6, 41, 3, 37.5, 12, 19.5, 16]],                             # on the right
            [[8, -9, 20, -4.5, 22, 8, 7, 9.75]],                              # above
            [[6, 12, 21, 11, 25, 31, 4, 27.5]],                               # below
            [[-10, -7, 39, -3, 35, 28, -6, 24]],                              # on every side: covers the image
            [[15, -8, 38, 10, 15, 28, -8, 10]],                               # a diamond with all four vertices outside, corners cut
            [[40, 5, 50, 5, 50, 15, 40, 15]],                                 # fully outside: right
            [[-30, -30, -5, -30, -5, -5, -30, -5]],                           # fully outside: above left
            [[2, 25, 20, 25, 20, 40, 2, 40]],                                 # fully outside: below
            [[0, 0, 30, 0, 30, 20, 0, 20]]]                                   # exactly the image
    want = check(objs, H, W)
    assert int(want[4].sum()) == H * W and int(want[9].sum()) == H * W
    assert int(want[6].sum()) == 0 and int(want[7].sum()) == 0 and int(want[8].sum()) == 0
    assert 0 < int(want[5].sum()) < H * W


def test_degenerate_and_self_intersecting_polygons():
    H, W = 40, 40
    objs = [[[5, 5, 5, 5, 30, 6, 30, 6, 30, 6, 28, 33, 6, 30]],               # duplicate consecutive vertices (zero-length edges)
            [[5, 5, 15, 5, 25, 5, 35, 5, 35, 20, 35, 35, 20, 35, 5, 35, 5, 20]],       # collinear vertices
            [[3, 3, 37, 35, 36, 4, 2, 36]],                                   # a bow-tie
            [[20, 2, 26, 38, 4, 14, 37, 13, 9, 37]],                          # a pentagram
            [[4.5, 4.5, 4.5, 4.5, 4.5, 4.5]],                                 # a single point three times
            [[2, 2, 38, 38, 2, 2, 38, 38]],                                   # a line there and back
            [[10, 10, 30, 10, 30, 10, 10, 10, 20, 30]]]                       # an edge retraced, then a triangle
    check(objs, H, W)


def test_long_edges_and_many_vertices():
    """an edge of 300 pixels is 1500 points, 24 steps of a wave; a polygon of 1600 vertices is 1600 waves and spans many workgroups"""
    H, W = 14, 330
    check([[[1, 1, 326, 11, 3, 12.5]], [[0.5, 13, 329.5, 0.5, 329.5, 13.5]], [[-20, 7, 350, 6, 350, 9, -20, 8]]], H, W)
    H, W = 320, 12
    check([[[1, 1, 11, 318, 2.5, 300]], [[6, -40, 9, 360, 3, 360]]], H, W)
    rng = np.random.default_rng(3)
    ang = np.sort(rng.uniform(0, 2 * np.pi, 1600))
    rad = 40 + 8 * np.sin(9 * ang) + rng.uniform(-1.5, 1.5, 1600)
    star = np.round(np.stack([50 + rad * np.cos(ang), 48 + rad * np.sin(ang)], 1), 2).reshape(-1).tolist()
    want = check([[star], [[10, 10, 20, 10, 20, 20]]], 96, 100)
    assert 3000 < int(want[0].sum()) < 96 * 100


# ------------------------------------------------------------------------------------------------ 5. objects
def test_union_of_overlapping_polygons_empty_objects_and_no_objects():
    H, W = 36, 44
    three = [[4, 4, 26, 5, 24, 22, 5, 20], [14.5, 10.25, 40, 12, 38.75, 30, 16, 28], [10, 16, 30, 15, 28, 34, 9, 33]]
    single = [pr.poly_mask_ref(p, H, W) for p in three]
    union, xor = single[0] | single[1] | single[2], single[0] ^ single[1] ^ single[2]
    assert (single[0] & single[1] & single[2]).any() and (union != xor).any()          # the case really overlaps: OR and XOR differ
    objs = [three, [], [three[1]], [], []]
    want = check(objs, H, W)
    assert torch.equal(want[0], torch.from_numpy(union)) and int(want[1].sum()) == 0 and int(want[3].sum()) == 0
    check([[], []], 5, 9)                                                             # objects, but no polygon and no vertex at all
    masks, area = rasterize([], 7, 9)
    assert tuple(masks.shape) == (0, 7, 9) and tuple(area.shape) == (0,)


def test_twenty_objects_in_one_call_equal_one_call_each():
    H, W = 61, 83
    rng = np.random.default_rng(20)
    objs = [[f(rng, H, W, int(rng.integers(3, 12))) for f in (tenths, cents, ties)[: 1 + i % 3]] for i in range(20)]
    masks, area = rasterize(objs, H, W)
    for i, o in enumerate(objs):
        m1, a1 = rasterize([o], H, W)
        assert torch.equal(m1[0], masks[i]) and int(a1[0]) == int(area[i]), i
    assert torch.equal(masks.cpu(), reference(objs, H, W))


# ------------------------------------------------------------------------------------------------ 6. determinism, graph capture
def test_two_runs_are_bit_identical_and_a_captured_graph_replays_to_the_eager_result():
    from ape_amd import ops
    from ape_amd.evaluation import pack_polygons
    H, W = 200, 333
    objs = family_objects(H, W, 77) + [[]]
    xy, vo, po = [t.cuda() for t in pack_polygons(objs)]
    m0, a0 = ops.poly_rasterize(xy, vo, po, H, W)
    m1, a1 = ops.poly_rasterize(xy, vo, po, H, W)
    assert torch.equal(m0, m1) and torch.equal(a0, a1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mg, ag = ops.poly_rasterize(xy, vo, po, H, W)
    torch.cuda.synchronize()
    for _ in range(2):                                                                # the second replay finds the first one's toggles
        mg.fill_(7)
        ag.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(mg, m0) and torch.equal(ag, a0)
    assert torch.equal(m0.cpu(), reference(objs, H, W))


# ------------------------------------------------------------------------------------------------ 7. the wrapper
def test_wrapper_rejects_wrong_inputs():
    from ape_amd import ops
    from ape_amd.evaluation import pack_polygons
    xy, vo, po = [t.cuda() for t in pack_polygons([[[1, 1, 5, 1, 3, 4]]])]
    with pytest.raises(TypeError):
        ops.poly_rasterize(xy.float(), vo, po, 8, 8)
    with pytest.raises(TypeError):
        ops.poly_rasterize(xy, vo.long(), po, 8, 8)
    with pytest.raises(TypeError):
        ops.poly_rasterize(xy, vo, po.long(), 8, 8)
    with pytest.raises(ValueError):
        ops.poly_rasterize(xy.reshape(-1), vo, po, 8, 8)
    with pytest.raises(ValueError):
        ops.poly_rasterize(xy.t().contiguous().t(), vo, po, 8, 8)
    with pytest.raises(ValueError):
        ops.poly_rasterize(xy, vo[:0], po, 8, 8)
    with pytest.raises(ValueError):
        ops.poly_rasterize(xy, vo, po, 0, 8)
    with pytest.raises(ValueError):
        ops.poly_rasterize(xy, vo, po, 8, 8, out=torch.empty((1, 8, 9), dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError):
        ops.poly_rasterize(xy.cpu(), vo, po, 8, 8)
    # offsets are data: ranges that leave their arrays are clamped, nothing outside is read or written
    bad_vo, bad_po = torch.tensor([-5, 400], dtype=torch.int32).cuda(), torch.tensor([-3, 9], dtype=torch.int32).cuda()
    masks, _ = ops.poly_rasterize(xy, bad_vo, bad_po, 8, 8)
    assert torch.equal(masks.cpu(), reference([[[1, 1, 5, 1, 3, 4]]], 8, 8))


# ------------------------------------------------------------------------------------------------ 8. end to end
def test_accumulators_on_polygon_ground_truth_equal_the_reference_masks():
    from ape_amd.evaluation import COCOAccumulator, ReferringAccumulator, segmentations_to_masks
    H, W = 90, 120
    rng = np.random.default_rng(8)
    gt = [[cents(rng, H, W, 6)], [tenths(rng, H, W, 5), cents(rng, H, W, 7)], [ties(rng, H, W, 4)], [cents(rng, H, W, 9)]]
    gt_classes, crowd = [0, 1, 1, 2], [0, 0, 1, 0]
    want = reference(gt, H, W)
    assert all(int(m.sum()) > 0 for m in want)
    pred = torch.cat([want, torch.roll(want, (3, -4), (1, 2)), torch.roll(want, (-9, 11), (1, 2))]).cuda()
    scores = torch.linspace(0.95, 0.2, pred.shape[0]).cuda()
    classes = torch.tensor(gt_classes * 3).cuda()
    got, area = segmentations_to_masks(gt, H, W, return_area=True)
    assert got.is_cuda and torch.equal(got.cpu(), want) and torch.equal(area.cpu(), want.flatten(1).sum(1))
    res = []
    for g, kw in ((want.cuda(), {}), (gt, {}), (gt, {"image_size": (H, W)})):
        acc = COCOAccumulator("segm", 3)
        acc.update(pred, scores, classes, g, gt_classes, gt_crowd=crowd, **kw)
        res.append(acc.compute())
    assert 0 < res[0]["AP"] <= 1
    for r in res[1:]:
        assert all(r[k] == res[0][k] or (r[k] != r[k] and res[0][k] != res[0][k]) for k in res[0]) and r.keys() == res[0].keys()
    res = []
    for polygons in (False, True):
        acc = ReferringAccumulator()
        for i in range(len(gt)):
            for j in range(3):
                acc.update(gt_mask=gt[i] if polygons else want[i].cuda(), pred_mask=pred[4 * j + i])
            acc.update(gt_mask=gt[i] if polygons else want[i].cuda(), image_size=(H, W))          # no prediction
        res.append(acc.compute())
    assert res[0]["samples"] == 16 and res[1] == res[0] and 0 < res[0]["oIoU"] < 100
