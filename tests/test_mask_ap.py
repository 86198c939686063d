"""Mask AP (ape_amd/evaluation.py) on the CPU: `ops.mask_pack_bits`, `ops.bitmask_pair_counts`, `ops.mask_pair_iou` and `ops.rle_decode`
are replaced by the torch restatements below, so what runs here is the host logic -- the protocol shared with `box_ap`, the input
forms, the accumulator and its two-rank reduce.  Masks of integer-coordinate rectangles have the IoUs of their boxes, so the known
answers of tests/test_box_ap.py carry over.  The host function `ape_hip_rle_from_string` and the C entry points' argument checks run
on the real library (they need no GPU)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------ torch restatements
def _bytes(masks):
    if masks.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f"masks are uint8 or bool, got {masks.dtype}")
    if masks.dim() != 3 or not masks.is_contiguous():
        raise ValueError("masks must be contiguous [n, H, W]")
    return masks


def pack_bits(masks):
    """ops.mask_pack_bits restated: pixel p = bit p % 64 of word p // 64, int64 storage"""
    masks = _bytes(masks)
    n = masks.shape[0]
    flat = (masks.reshape(n, -1) != 0).long()
    words = (flat.shape[1] + 63) // 64
    padded = torch.zeros((n, words * 64), dtype=torch.int64)
    padded[:, : flat.shape[1]] = flat
    weight = torch.tensor([1 << k for k in range(63)] + [-(1 << 63)], dtype=torch.int64)
    return (padded.reshape(n, words, 64) * weight).sum(-1), flat.sum(1)


def _unpack(bits):
    return ((bits[:, :, None] >> torch.arange(64)) & 1).reshape(bits.shape[0], -1)


def pair_counts(a_bits, b_bits, out=None):
    """ops.bitmask_pair_counts restated"""
    if a_bits.dtype != torch.int64 or b_bits.dtype != torch.int64:
        raise TypeError("packed masks are int64 words")
    if a_bits.shape[1] != b_bits.shape[1]:
        raise ValueError("word counts differ")
    inter = _unpack(a_bits) @ _unpack(b_bits).T
    if out is not None:
        out.copy_(inter)
        return out
    return inter


def pair_iou(a, b):
    """ops.mask_pair_iou restated on the two restatements above"""
    a, b = _bytes(a), _bytes(b)
    if tuple(a.shape[1:]) != tuple(b.shape[1:]):
        raise ValueError("mask sizes differ")
    (a_bits, area_a), (b_bits, area_b) = pack_bits(a), pack_bits(b)
    inter = pair_counts(a_bits, b_bits)
    union = area_a[:, None] + area_b[None, :] - inter
    iou = torch.where(union > 0, inter.double() / union.clamp_min(1).double(), torch.zeros((), dtype=torch.float64))
    return iou, inter, area_a, area_b


def decode_runs(counts, nruns, H, W, out=None):
    """ops.rle_decode restated: column-major runs starting with the zeros, clipped to H * W"""
    n, cap = counts.shape
    res = torch.zeros((n, H, W), dtype=torch.uint8)
    for i in range(n):
        runs = (counts[i, : min(int(nruns[i]), cap)].long() & 0xFFFFFFFF).tolist()
        flat = np.zeros(H * W, np.uint8)
        pos = 0
        for k, r in enumerate(runs):
            flat[pos: pos + r] = k & 1
            pos = min(pos + r, H * W)
        res[i] = torch.from_numpy(flat.reshape(W, H).T.copy())
    if out is not None:
        out.copy_(res)
        return out
    return res


def _patch(ops, setter):
    setter(ops, "mask_pack_bits", pack_bits)
    setter(ops, "bitmask_pair_counts", pair_counts)
    setter(ops, "mask_pair_iou", pair_iou)
    setter(ops, "rle_decode", decode_runs)


@pytest.fixture
def host_masks(monkeypatch, fake_ops):
    import ape_amd.ops as ops
    from ape_amd import build
    build.build(verbose=False)                       # ops.rle_from_string is the library's host function
    _patch(ops, lambda o, name, fn: monkeypatch.setattr(o, name, fn, raising=True))


def draw(boxes, H, W):
    """integer XYXY boxes -> uint8 [n, H, W] masks of the pixels [y0, y1) x [x0, x1)"""
    m = torch.zeros((len(boxes), H, W), dtype=torch.uint8)
    for i, (x0, y0, x1, y1) in enumerate(torch.as_tensor(boxes).long().tolist()):
        m[i, y0:y1, x0:x1] = 1
    return m


def to_rles(masks, form="bytes"):
    """RLE dicts of host masks through the (patched) encoder ops"""
    import ape_amd.ops as ops
    counts, nruns = ops.rle_encode(masks, cap=masks.shape[1] * masks.shape[2] + 1)
    out = []
    for i in range(masks.shape[0]):
        runs = counts[i, : int(nruns[i])]
        c = ops.rle_to_string(runs)
        out.append({"size": [masks.shape[1], masks.shape[2]], "counts": c if form == "bytes" else c.decode() if form == "str" else runs.tolist()})
    return out


# ------------------------------------------------------------------------------------------------ the protocol, on rectangles
def test_hand_computed_case_of_box_ap_redrawn_as_masks(host_masks):
    """tests/test_box_ap.py's case at half the scale: GT 50 x 50 squares, the third detection covers 31 of 50 columns of GT 2 (IoU 0.62)"""
    from ape_amd.evaluation import box_ap, mask_ap
    gt_b = torch.tensor([[0, 0, 50, 50], [100, 100, 150, 150]])
    det_b = torch.tensor([[0, 0, 50, 50], [250, 250, 300, 300], [100, 100, 131, 150]])
    scores, classes = torch.tensor([0.9, 0.8, 0.7]), torch.tensor([3, 3, 3])
    r = mask_ap([(draw(det_b, 300, 300), scores, classes)], [(draw(gt_b, 300, 300), torch.tensor([3, 3]))])
    want = (3 * (51 + 50 * 2.0 / 3.0) / 101 + 7 * 51 / 101) / 10
    assert abs(r["AP"] - want) < 1e-9 and abs(r["AP50"] - (51 + 50 * 2.0 / 3.0) / 101) < 1e-9 and abs(r["AP75"] - 51 / 101) < 1e-9
    assert r["classes"] == 1 and r["gt"] == 2 and r["dets"] == 3
    rb = box_ap([(det_b.double(), scores, classes)], [(gt_b.double(), torch.tensor([3, 3]))])
    assert set(r) == set(rb) and all(abs(r[k] - rb[k]) < 1e-9 for k in r)


H, W = 80, 192           # one rectangle per 16 x 16 cell of the left half (5 x 6 cells, so no two of an image overlap); + SHIFT moves a
SHIFT = 96               # copy to the right half, where it meets nothing


def _images(seed=0, count=4, per=30):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(count):
        cell = torch.randperm(30, generator=g)[:per]
        xy = torch.stack([cell % 6, cell // 6], 1) * 16 + torch.randint(0, 3, (per, 2), generator=g)
        wh = torch.randint(3, 14, (per, 2), generator=g)
        out.append((torch.cat([xy, xy + wh], 1), torch.randint(0, 5, (per,), generator=g)))
    return out, g


def _shift(b):
    return b + torch.tensor([SHIFT, 0, SHIFT, 0])


def test_rectangle_masks_have_their_boxes_ious_and_properties_carry_over(host_masks):
    from ape_amd.evaluation import box_ap, mask_ap
    gt_b, g = _images()
    gt = [(draw(b, H, W), c) for b, c in gt_b]
    det_b = [(b, torch.rand(len(b), generator=g), c) for b, c in gt_b]

    def both(dets, gts_b=gt_b, gts=gt, **kw):
        """mask AP of the drawn rectangles; it must be the box AP of the rectangles themselves"""
        rm = mask_ap([(draw(b, H, W), s, c) for b, s, c in dets], gts, **kw)
        rb = box_ap([(b.double(), s, c) for b, s, c in dets], [(b.double(), c) for b, c in gts_b], **kw)
        assert all(abs(rm[k] - rb[k]) < 1e-9 for k in rb), (rm, rb)
        return rm

    assert both(det_b)["AP"] == 1.0                                                   # the ground truth itself, any scores
    assert both([(b, s, (c + 1) % 5) for b, s, c in det_b])["AP"] == 0.0             # right masks, wrong classes
    fp_first = [(torch.cat([_shift(b), b]), torch.cat([s + 1, s]), torch.cat([c, c])) for b, s, c in det_b]
    assert abs(both(fp_first)["AP"] - 0.5) < 1e-12                                    # every true positive behind as many false ones
    fp_last = [(torch.cat([b, _shift(b)]), torch.cat([s + 1, s]), torch.cat([c, c])) for b, s, c in det_b]
    assert both(fp_last)["AP"] == 1.0
    extra = [(torch.cat([b, b[:1]]), torch.cat([s, s[:1]]), torch.cat([c, torch.tensor([7])])) for b, s, c in det_b]
    assert both(extra)["AP"] == 1.0                                                   # a class without ground truth is not scored
    miss = [(b[c != 0], s[c != 0], c[c != 0]) for b, s, c in det_b]
    assert abs(both(miss)["AP"] - 0.8) < 1e-12                                        # a class with ground truth and no detection is 0
    # max_dets counts per (image, category): per class n true positives behind 4 n better-scored false ones
    b0, c0 = gt_b[0]
    many = [(torch.cat([b0] + [_shift(b0)] * 4), torch.cat([torch.rand(30, generator=g)] + [torch.rand(30, generator=g) + 2] * 4),
             torch.cat([c0] * 5))]
    fewest = int(torch.bincount(c0, minlength=5).min())
    assert fewest >= 1
    assert both(many, gt_b[:1], gt[:1], max_dets=4 * fewest)["AP"] == 0.0
    r = both(many, gt_b[:1], gt[:1])
    assert r["AP"] > 0.0 and r["dets"] == 150
    # shifted and clipped rectangles: IoUs strictly between 0 and 1, equal to the boxes'
    def moved(b):
        xy = (b[:, :2] + torch.randint(-2, 3, (len(b), 2), generator=g)).clamp_min(0)
        return torch.cat([xy, xy + (b[:, 2:] - b[:, :2])], 1)
    r = both([(moved(b), s, c) for b, s, c in det_b])
    assert 0.0 < r["AP"] < 1.0 and r["AP50"] > r["AP75"]


def test_empty_masks_have_iou_zero_and_never_match(host_masks):
    import ape_amd.ops as ops
    from ape_amd.evaluation import mask_ap
    empty = torch.zeros((2, 5, 13), dtype=torch.uint8)
    iou, inter, area_a, area_b = ops.mask_pair_iou(empty, empty)
    assert iou.dtype == torch.float64 and iou.tolist() == [[0.0, 0.0], [0.0, 0.0]] and int(inter.sum()) == 0
    gt = draw([[1, 1, 4, 4]], 5, 13)
    det = torch.cat([torch.zeros_like(gt), gt])                                      # an empty detection in front of the right one
    r = mask_ap([(det, torch.tensor([0.9, 0.5]), torch.tensor([1, 1]))], [(gt, torch.tensor([1]))])
    assert abs(r["AP"] - 0.5) < 1e-12 and r["dets"] == 2                             # the empty one is a false positive, at every threshold
    r = mask_ap([(det[:1], torch.tensor([0.9]), torch.tensor([1]))], [(torch.zeros_like(gt), torch.tensor([1]))])
    assert r["AP"] == 0.0                                                            # empty against empty: no match either
    r = mask_ap([(det[:0], torch.zeros(0), torch.zeros(0, dtype=torch.long))], [(gt, torch.tensor([1]))])
    assert r["AP"] == 0.0 and r["gt"] == 1 and r["dets"] == 0                        # an image without detections


def _mask_case():
    gt_b, g = _images(seed=3, count=4, per=12)
    gt = [(draw(b, H, W), c) for b, c in gt_b]
    det = []
    for b, c in gt_b:
        moved = b + torch.randint(-2, 3, (len(b), 1), generator=g).clamp_min(-int(b.min()))
        both = torch.cat([moved, _shift(b[:3])])
        det.append((draw(both, H, W), torch.rand(len(both), generator=g), torch.cat([c, c[:3]])))
    return det, gt


def _close(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k] == pytest.approx(b[k], rel=1e-12, abs=1e-12), (k, a[k], b[k])


def test_rle_inputs_bool_inputs_and_the_accumulator_equal_tensor_inputs(host_masks):
    from ape_amd.evaluation import MaskAPAccumulator, decode_masks, mask_ap
    from ape_amd.structures import Instances
    det, gt = _mask_case()
    want = mask_ap(det, gt)
    assert 0.0 < want["AP"] < 1.0
    for form in ("bytes", "str", "list"):
        m = det[0][0]
        assert torch.equal(decode_masks(to_rles(m, form)), m), form
        got = mask_ap([(to_rles(m, form), s, c) for m, s, c in det], [(to_rles(m, form), c) for m, c in gt])
        _close(got, want)
    _close(mask_ap([(m.bool(), s, c) for m, s, c in det], [(m * 255, c) for m, c in gt]), want)     # bool, and any non-zero value
    acc = MaskAPAccumulator()
    for i, ((m, s, c), (gm, gc)) in enumerate(zip(det, gt)):
        if i % 2 == 0:
            acc.update(m, s, c, gm, gc)
        else:                                                 # an Instances carrying pred_masks, or only the runtime's pred_masks_rle
            inst = Instances((H, W))
            inst.scores, inst.pred_classes = s, c
            if i == 1:
                inst.pred_masks = m
            else:
                inst.pred_masks_rle = to_rles(m)
            acc.update(inst, gt_masks=gm, gt_classes=gc)
    acc.reduce()                                              # no process group: a no-op
    assert len(acc.records) == len(det) and all(r[3].dtype == torch.float64 and not r[3].is_cuda for r in acc.records)
    _close(acc.compute(), want)
    with pytest.raises(ValueError):
        acc.update(det[0][0], det[0][1], det[0][2], gt[0][0][:, :-1], gt[0][1])          # sizes differ
    with pytest.raises(ValueError):
        acc.update(det[0][0], det[0][1][:-1], det[0][2], gt[0][0], gt[0][1])             # a score short
    with pytest.raises(ValueError):
        decode_masks(to_rles(det[0][0][:1]) + [{"size": [H, W + 1], "counts": b"0"}])


# ------------------------------------------------------------------------------------------------ reduce over two ranks
def _worker(rank, world, port, ret):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    import ape_amd.ops as ops
    from ape_amd.evaluation import MaskAPAccumulator
    _patch(ops, setattr)
    det, gt = _mask_case()
    acc = MaskAPAccumulator()
    for (m, s, c), (gm, gc) in list(zip(det, gt))[rank::world]:
        acc.update(m, s, c, gm, gc)
    acc.reduce()
    ret[rank] = (len(acc.records), acc.compute())
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_reduce_equals_the_single_process_result(host_masks):
    import torch.multiprocessing as mp
    from ape_amd.evaluation import mask_ap
    world = 2
    port = 33500 + (os.getpid() % 2000)
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    det, gt = _mask_case()
    want = mask_ap(det, gt)
    for rank in range(world):
        count, got = ret[rank]
        assert count == len(det)
        _close(got, want)


# ------------------------------------------------------------------------------------------------ the real library, no GPU
def test_rle_from_string_round_trips_with_rle_to_string():
    from ape_amd import _lib, build, ops
    build.build(verbose=False)
    assert ops.rle_from_string(b"527O").tolist() == [5, 2, 7, 1]                      # 4th count stored as 1 - 2 = -1 -> 'O'
    assert ops.rle_from_string("X1").tolist() == [40] and ops.rle_from_string(b"13").tolist() == [1, 3]
    cases = [[5, 2, 7, 1], [0, 4], [1, 3], [6], [40000, 3, 70000, 100000, 2, 99999, 1, 32768, 32767, 1],           # >= 2^15: multi-character,
             [9, 100000, 9, 1, 100000, 1, 5, 40000], [1 << 20, 1, 1, 1 << 20, (1 << 31) + 5, 1, 7]]                # and negative deltas
    g = torch.Generator().manual_seed(0)
    cases.append(torch.randint(0, 1 << 17, (500,), generator=g).tolist())
    for runs in cases:
        t = torch.tensor(runs, dtype=torch.int64).to(torch.int32)
        s = ops.rle_to_string(t)
        back = ops.rle_from_string(s)
        assert back.dtype == torch.int32 and not back.is_cuda and torch.equal(back, t), runs
        assert torch.equal(ops.rle_from_string(s.decode()), t)
    assert ops.rle_from_string(b"").numel() == 0 and ops.rle_from_string("").dtype == torch.int32
    with pytest.raises(TypeError):
        ops.rle_from_string([1, 2])
    f = _lib.load().ape_hip_rle_from_string
    buf = (ctypes.c_uint32 * 4)(9, 9, 9, 9)
    assert f(b"527O", 4, buf, 4) == 4 and list(buf) == [5, 2, 7, 1]
    buf = (ctypes.c_uint32 * 4)(9, 9, 9, 9)
    assert f(b"527O", 4, buf, 2) == -4 and list(buf) == [5, 2, 9, 9]                  # too small: -needed, nothing past the buffer
    assert f(b"527O", 4, None, 0) == -4 and f(b"", 0, buf, 4) == 0 and f(None, 0, None, 0) == 0


def test_argument_errors_are_reported_without_a_gpu():
    from ape_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    one = ctypes.c_void_p(64)            # never dereferenced: every call below is refused, or has nothing to do, before any HIP call
    err = lib.ape_hip_last_error

    f = lib.ape_hip_mask_pack_bits       # (masks, n, npix, stride, bits, ldb, area, stream)
    assert f(None, 1, 64, 64, one, 1, one, None) != 0 and b"null" in err()
    assert f(one, 1, 64, 64, None, 1, one, None) != 0 and b"null" in err()
    assert f(one, 1, 64, 64, one, 1, None, None) != 0 and b"null" in err()
    assert f(one, -1, 64, 64, one, 1, one, None) != 0 and b"negative" in err()
    assert f(one, 1, 65, 65, one, 1, one, None) != 0 and b"ldb" in err()              # 65 pixels are two words
    assert f(one, 2, 64, 63, one, 1, one, None) != 0 and b"stride" in err()
    assert f(one, 1, 1 << 32, 1 << 32, one, 1 << 26, one, None) != 0 and b"too large" in err()
    assert f(None, 0, 64, 64, None, 1, None, None) == 0                                # n == 0: a successful no-op

    f = lib.ape_hip_bitmask_pair_counts  # (a, n, lda, b, m, ldb, words, inter, ldi, stream)
    assert f(None, 1, 4, one, 1, 4, 4, one, 1, None) != 0 and b"null" in err()
    assert f(one, 1, 4, None, 1, 4, 4, one, 1, None) != 0 and b"null" in err()
    assert f(one, 1, 4, one, 1, 4, 4, None, 1, None) != 0 and b"null" in err()
    assert f(one, -1, 4, one, 1, 4, 4, one, 1, None) != 0 and b"negative" in err()
    assert f(one, 1, 4, one, -2, 4, 4, one, 1, None) != 0 and b"negative" in err()
    assert f(one, 1, 3, one, 1, 4, 4, one, 1, None) != 0 and b"words" in err()
    assert f(one, 1, 4, one, 1, 3, 4, one, 1, None) != 0 and b"words" in err()
    assert f(one, 1, 4, one, 2, 4, 4, one, 1, None) != 0 and b"ldi" in err()
    assert f(None, 0, 4, None, 5, 4, 4, None, 5, None) == 0 and f(None, 5, 4, None, 0, 4, 4, None, 0, None) == 0

    f = lib.ape_hip_rle_decode           # (counts, nruns, n, cap, H, W, workspace, masks, stream)
    assert f(None, one, 1, 8, 4, 4, one, one, None) != 0 and b"null" in err()
    assert f(one, None, 1, 8, 4, 4, one, one, None) != 0 and b"null" in err()
    assert f(one, one, 1, 8, 4, 4, None, one, None) != 0 and b"null" in err()
    assert f(one, one, 1, 8, 4, 4, one, None, None) != 0 and b"null" in err()
    assert f(one, one, -1, 8, 4, 4, one, one, None) != 0 and b"negative" in err()
    assert f(one, one, 1, 8, 0, 4, one, one, None) != 0 and b"at least 1" in err()
    assert f(one, one, 1, 8, 65536, 65536, one, one, None) != 0 and b"too large" in err()      # H * W does not fit 32 bits
    assert f(one, one, 1, 8, 1 << 30, 4, one, one, None) != 0 and b"too large" in err()
    assert f(None, None, 0, 8, 4, 4, None, None, None) == 0
    assert lib.ape_hip_rle_decode_workspace_words(3, 100) == 300 and lib.ape_hip_rle_decode_workspace_words(1 << 20, 1 << 20) < 0
