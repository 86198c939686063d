"""Polygon ground truth on the host side: `pack_polygons`, `segmentations_to_masks` and the accumulators' `image_size`, with
`ops.poly_rasterize` replaced by the rleFrPoly restatement (tests/polygon_refs.py) and the mask kernels by torch restatements.  The kernel
itself is held to the same restatement in tests/test_polygons_gpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import coco_util as U
import polygon_refs as pr
import test_mask_ap as tm


# ------------------------------------------------------------------------------------------------ restatements of the kernels
def rasterize_ref(xy, vert_offsets, poly_offsets, H, W, out=None):
    """ops.poly_rasterize restated on tests/polygon_refs.py"""
    assert xy.dtype == torch.float64 and vert_offsets.dtype == torch.int32 and poly_offsets.dtype == torch.int32
    vo, po = vert_offsets.tolist(), poly_offsets.tolist()
    n = len(po) - 1
    masks = torch.zeros((n, H, W), dtype=torch.uint8)
    for o in range(n):
        polys = [xy[vo[p]: vo[p + 1]].reshape(-1).tolist() for p in range(po[o], po[o + 1])]
        masks[o] = torch.from_numpy(pr.segm_mask_ref(polys, H, W))
    if out is not None:
        out.copy_(masks)
        masks = out
    return masks, masks.flatten(1).sum(1, dtype=torch.int64)


def paired_counts(a, b, out=None):
    """ops.mask_paired_counts restated"""
    a, b = a.flatten(1) != 0, b.flatten(1) != 0
    res = torch.stack([(a & b).sum(1), a.sum(1), b.sum(1)], 1).long()
    if out is not None:
        out.copy_(res)
        return out
    return res


def _band(m, d):
    """the inner boundary band: the mask without its erosion by the (2 d + 1)^2 square, the outside counting as background"""
    x = F.pad((m != 0).float()[:, None], (d, d, d, d), value=0.0)
    eroded = -F.max_pool2d(-x, 2 * d + 1, stride=1)
    return ((m != 0) & (eroded[:, 0] < 0.5)).to(torch.uint8)


def boundary_pair_iou(a, b, dilation_ratio=0.02, dilation=None):
    """ops.boundary_pair_iou restated (the first two results are what the accumulators read)"""
    import ape_amd.ops as ops
    d = ops.boundary_dilation(a.shape[1], a.shape[2], dilation_ratio) if dilation is None else int(dilation)
    biou, binter, barea_a, barea_b = tm.pair_iou(_band(a, d), _band(b, d))
    iou, inter, area_a, area_b = tm.pair_iou(a.contiguous(), b.contiguous())
    return biou, iou, binter, inter, barea_a, barea_b, area_a, area_b


def coco_match(iou, det_order, det_offsets, gt_order, gt_offsets, gt_crowd, gt_area, det_area, thresholds=None, ranges=None, match=None,
               flag=None):
    return U.host_match(iou, det_order, det_offsets, gt_order, gt_offsets, gt_crowd, gt_area, det_area)


@pytest.fixture
def host_polygons(monkeypatch, fake_ops):
    import ape_amd.ops as ops
    from ape_amd import build
    build.build(verbose=False)                                # ops.rle_from_string / rle_to_string are the library's host functions
    tm._patch(ops, lambda o, name, fn: monkeypatch.setattr(o, name, fn, raising=True))
    for name, fn in (("poly_rasterize", rasterize_ref), ("mask_paired_counts", paired_counts), ("boundary_pair_iou", boundary_pair_iou),
                     ("coco_match", coco_match)):
        monkeypatch.setattr(ops, name, fn, raising=True)
    return ops


H, W = 24, 30
# one image: three objects, the second of two overlapping polygons, the third partly outside the image
GT = [[[2, 2, 12, 2, 12, 11, 2, 11]],
      [[14.5, 3.2, 27.3, 4.1, 25.0, 14.8, 15.1, 12.6], [20, 8, 29, 8, 29, 20, 20, 20]],
      [[-4, 15, 9.5, 13.25, 11, 30, 3, 22.5]]]
GT_CLASSES = [0, 1, 1]


def gt_masks():
    return torch.stack([torch.from_numpy(pr.segm_mask_ref(p, H, W)) for p in GT])


def predictions():
    """four predictions: a ground-truth mask, two shifted ones and a stray block"""
    g = gt_masks()
    p = torch.zeros((4, H, W), dtype=torch.uint8)
    p[0] = g[0]
    p[1, :, 2:] = g[1][:, :-2]
    p[2, 1:] = g[2][:-1]
    p[3, 16:22, 12:19] = 1
    return p, torch.tensor([0.9, 0.8, 0.7, 0.6]), torch.tensor([0, 1, 1, 0])


# ------------------------------------------------------------------------------------------------ pack_polygons
def test_pack_polygons_offsets():
    from ape_amd.evaluation import pack_polygons
    xy, vo, po = pack_polygons(GT + [[]])
    assert xy.dtype == torch.float64 and vo.dtype == torch.int32 and po.dtype == torch.int32
    assert tuple(xy.shape) == (16, 2) and xy.is_contiguous()
    assert vo.tolist() == [0, 4, 8, 12, 16] and po.tolist() == [0, 1, 3, 4, 4]
    assert xy[4].tolist() == [14.5, 3.2] and xy[15].tolist() == [3, 22.5]
    xy, vo, po = pack_polygons([])
    assert tuple(xy.shape) == (0, 2) and vo.tolist() == [0] and po.tolist() == [0]
    xy, vo, po = pack_polygons([[], [(0, 0, 1.5, 0, 1, 1)]])                 # tuples and an object without polygons
    assert vo.tolist() == [0, 3] and po.tolist() == [0, 0, 1]


@pytest.mark.parametrize("bad", [[[[0, 0, 1, 0, 1]]],                        # an odd length
                                 [[[0, 0, 1, 1]]],                           # fewer than 6 numbers
                                 [[[0, 0, 1, 0, float("nan"), 1]]],
                                 [[[0, 0, 1, 0, float("inf"), 1]]],
                                 [[[0, 0, 1, 0, 65536.5, 1]]],
                                 [[[0, 0, 1, 0, 1, -70000]]],
                                 [{"size": [2, 2], "counts": [4]}]])          # an RLE dict is not a polygon list
def test_pack_polygons_errors(bad):
    from ape_amd.evaluation import pack_polygons
    with pytest.raises(ValueError):
        pack_polygons(bad)


def test_pack_polygons_takes_the_bound_itself():
    from ape_amd.evaluation import pack_polygons
    assert pack_polygons([[[0, 0, 65536, 0, -65536, 1]]])[0].abs().max() == 65536


# ------------------------------------------------------------------------------------------------ segmentations_to_masks
def test_segmentations_to_masks_mixed_entries_keep_their_order(host_polygons):
    from ape_amd.evaluation import segmentations_to_masks
    g = gt_masks()
    rles = {form: tm.to_rles(g, form) for form in ("bytes", "str", "list")}
    segs = [GT[0], rles["bytes"][1], GT[2], rles["str"][0], rles["list"][2], GT[1], []]
    want = torch.cat([g[[0, 1, 2, 0, 2, 1]], torch.zeros((1, H, W), dtype=torch.uint8)])
    got, area = segmentations_to_masks(segs, H, W, device="cpu", return_area=True)
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    assert torch.equal(area, want.flatten(1).sum(1))
    assert torch.equal(segmentations_to_masks(segs, H, W, device="cpu"), want)
    only, area = segmentations_to_masks(GT, H, W, device="cpu", return_area=True)
    assert torch.equal(only, g) and torch.equal(area, g.flatten(1).sum(1))
    assert torch.equal(segmentations_to_masks(rles["bytes"], H, W, device="cpu"), g)


def test_segmentations_to_masks_calls_each_kernel_once(host_polygons, monkeypatch):
    from ape_amd.evaluation import segmentations_to_masks
    calls = {"poly": 0, "rle": 0}

    def poly(*a, **k):
        calls["poly"] += 1
        return rasterize_ref(*a, **k)

    def rle(*a, **k):
        calls["rle"] += 1
        return tm.decode_runs(*a, **k)
    monkeypatch.setattr(host_polygons, "poly_rasterize", poly)               # reaches wire only if it says `ops.poly_rasterize`
    monkeypatch.setattr(host_polygons, "rle_decode", rle)
    r = tm.to_rles(gt_masks())
    segmentations_to_masks([GT[0], r[1], GT[2], r[0], GT[1]], H, W, device="cpu")
    assert calls == {"poly": 1, "rle": 1}


def test_segmentations_to_masks_empty_and_errors(host_polygons):
    from ape_amd.evaluation import segmentations_to_masks
    out, area = segmentations_to_masks([], 5, 7, device="cpu", return_area=True)
    assert tuple(out.shape) == (0, 5, 7) and out.dtype == torch.uint8 and tuple(area.shape) == (0,) and area.dtype == torch.int64
    r = tm.to_rles(gt_masks())
    with pytest.raises(ValueError, match="size"):
        segmentations_to_masks([GT[0], r[0]], H, W + 1, device="cpu")
    with pytest.raises(ValueError):
        segmentations_to_masks([GT[0], "abc"], H, W, device="cpu")
    with pytest.raises(ValueError):
        segmentations_to_masks([[[0, 0, 1, 1]]], H, W, device="cpu")


# ------------------------------------------------------------------------------------------------ the accumulators
def test_coco_segm_with_polygon_ground_truth(host_polygons):
    from ape_amd.evaluation import COCOAccumulator
    p, s, c = predictions()
    crowd = [0, 0, 1]
    res = []
    for gt, kw in ((gt_masks(), {}), (GT, {"image_size": (H, W)}), (GT, {}), (tuple(GT), {}),
                   ([GT[0], tm.to_rles(gt_masks())[1], GT[2]], {})):
        acc = COCOAccumulator("segm", 2, device="cpu")
        acc.update(p, s, c, gt, GT_CLASSES, gt_crowd=crowd, **kw)
        acc.update(p[:0], s[:0], c[:0], gt, GT_CLASSES, **kw)             # no detections: the size comes from the [0, H, W] tensor
        res.append(acc.compute())
    assert res[0]["gt"] == 6 and res[0]["images"] == 2 and 0 < res[0]["AP"] <= 1
    for r in res[1:]:
        assert r.keys() == res[0].keys()
        for k in r:
            assert r[k] == res[0][k] or (r[k] != r[k] and res[0][k] != res[0][k]), k


@pytest.mark.parametrize("kind", ["mask", "boundary"])
def test_mask_and_boundary_ap_with_polygon_ground_truth(host_polygons, kind):
    from ape_amd.evaluation import BoundaryAPAccumulator, MaskAPAccumulator
    make = MaskAPAccumulator if kind == "mask" else BoundaryAPAccumulator
    p, s, c = predictions()
    res = []
    for gt, kw in ((gt_masks(), {}), (GT, {"image_size": (H, W)}), (GT, {}), (GT, {"image_size": [H, W]})):
        acc = make(device="cpu")
        acc.update(p, s, c, gt, GT_CLASSES, **kw)
        acc.update(tm.to_rles(p), s, c, gt, GT_CLASSES, **kw)               # the size of an RLE dict among the inputs
        res.append(acc.compute())
    assert res[0]["gt"] == 6 and 0 < res[0]["AP"] <= 1
    assert res[1] == res[0] and res[2] == res[0] and res[3] == res[0]


def test_boundary_iou_with_polygons(host_polygons):
    from ape_amd.evaluation import boundary_iou
    p, _, _ = predictions()
    want = boundary_iou(p, gt_masks(), device="cpu")
    assert torch.equal(boundary_iou(p, GT, device="cpu"), want)
    assert torch.equal(boundary_iou(p, GT, device="cpu", image_size=(H, W)), want)
    assert torch.equal(boundary_iou(GT, tm.to_rles(p), device="cpu"), boundary_iou(gt_masks(), p, device="cpu"))
    with pytest.raises(ValueError, match="image_size"):
        boundary_iou(GT, GT, device="cpu")


def test_referring_with_polygon_ground_truth(host_polygons):
    from ape_amd.evaluation import ReferringAccumulator
    p, _, _ = predictions()
    g = gt_masks()
    box = [1.0, 2.0, 20.0, 22.0]
    res = []
    for polygons in (False, True):
        acc = ReferringAccumulator(device="cpu")
        for i in range(3):
            gt = GT[i] if polygons else g[i]
            acc.update(gt_mask=gt, gt_box=box, pred_mask=p[i], pred_box=box)                         # size: the prediction's
            acc.update(gt_mask=gt, gt_box=box, pred_mask=p[i], pred_box=box, image_size=(H, W))
            acc.update(gt_mask=gt, gt_box=box, pred_mask=tm.to_rles(p[i: i + 1])[0], pred_box=box)   # size: the RLE dict's
            acc.update(gt_mask=gt, gt_box=box, image_size=(H, W))                                    # no prediction
        res.append(acc.compute())
    assert res[0]["samples"] == 12 and 0 < res[0]["mIoU"] < 100
    assert res[1] == res[0]


# ------------------------------------------------------------------------------------------------ the size and its errors
def test_size_resolution_order_and_errors(host_polygons):
    from ape_amd.evaluation import COCOAccumulator, MaskAPAccumulator, ReferringAccumulator
    from ape_amd.evaluation._common import _device_masks, mask_size
    p, s, c = predictions()
    rl = tm.to_rles(p)
    assert mask_size((3, 4), p, rl) == (3, 4)                               # image_size first
    assert mask_size(None, rl, p) == (H, W) and mask_size(None, p[:, :5], rl) == (5, W)      # then a tensor, wherever it stands
    assert mask_size(None, GT, rl) == (H, W) and mask_size(None, GT, rl[0]) == (H, W)        # then an RLE dict
    assert mask_size(None, GT, None) is None
    with pytest.raises(ValueError, match="image_size"):
        mask_size((1, 2, 3), p)
    # polygons need a size; a pure RLE list and a tensor behave as before, with or without one
    with pytest.raises(ValueError, match="image_size"):
        _device_masks(GT, "cpu")
    assert torch.equal(_device_masks(GT, "cpu", size=(H, W)), gt_masks())
    assert torch.equal(_device_masks(rl, "cpu"), p) and torch.equal(_device_masks(rl, "cpu", size=(H, W)), p)
    assert _device_masks([], "cpu", size=(H, W)) is None
    # a sample without prediction has nothing to take the size from
    with pytest.raises(ValueError, match="image_size"):
        ReferringAccumulator(device="cpu").update(gt_mask=GT[0])
    # image_size against a prediction tensor of another size: the existing size-mismatch errors
    with pytest.raises(ValueError, match="vs ground truth"):
        MaskAPAccumulator(device="cpu").update(p, s, c, GT, GT_CLASSES, image_size=(H + 1, W))
    with pytest.raises(ValueError, match="vs ground truth"):
        COCOAccumulator("segm", 2, device="cpu").update(p, s, c, GT, GT_CLASSES, image_size=(H, W + 2))
    with pytest.raises(ValueError, match="vs ground truth"):
        ReferringAccumulator(device="cpu").update(gt_mask=GT[0], pred_mask=p[0], image_size=(H + 1, W))
    # image_size wins over the prediction's size where both could serve: RLE predictions of another size are a mismatch too
    with pytest.raises(ValueError, match="vs ground truth"):
        MaskAPAccumulator(device="cpu").update(rl, s, c, GT, GT_CLASSES, image_size=(H, W + 1))


def test_existing_calls_are_unchanged(host_polygons):
    """tensor and RLE ground truth never reach the rasteriser, with or without image_size"""
    from ape_amd.evaluation import MaskAPAccumulator

    def boom(*a, **k):
        raise AssertionError("poly_rasterize was called")
    import ape_amd.ops as ops
    p, s, c = predictions()
    g = gt_masks()
    old = ops.poly_rasterize
    ops.poly_rasterize = boom
    try:
        res = []
        for gt, kw in ((g, {}), (tm.to_rles(g), {}), (g, {"image_size": (H, W)})):
            acc = MaskAPAccumulator(device="cpu")
            acc.update(p, s, c, gt, GT_CLASSES, **kw)
            res.append(acc.compute())
    finally:
        ops.poly_rasterize = old
    assert res[0] == res[1] == res[2]


def test_wrapper_refuses_host_tensors_and_wrong_types():
    from ape_amd import ops
    xy, vo, po = torch.zeros((3, 2), dtype=torch.float64), torch.tensor([0, 3], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        ops.poly_rasterize(xy, vo, po, 4, 4)


def test_polygon_kernels_join_the_last_object_of_the_link_line():
    """polygon.hip is no object of its own: boxcover.hip includes it (so it gets that file's -ffp-contract=off), and the link line keeps the
    objects it had"""
    import os

    from ape_amd import build
    names = [os.path.basename(f) for f in build._sources()]
    assert build.PART_OF == {"polygon.hip": "boxcover.hip"} and "polygon.hip" not in names and names[-1] == "boxcover.hip"
    assert os.path.exists(os.path.join(build.CSRC, "polygon.hip"))
    assert "-ffp-contract=off" in build.FILE_FLAGS["boxcover.hip"]
    with open(os.path.join(build.CSRC, "boxcover.hip")) as fh:
        assert fh.read().rstrip().endswith('#include "polygon.hip"')
    with open(os.path.join(build.CSRC, "polygon.hip")) as fh:
        text = fh.read()
    assert "fma(" not in text                                                # nothing asks for the contraction the flag forbids


def test_c_abi_argument_errors_without_a_gpu():
    """argument errors come before any HIP call: they are reported on a machine without a device"""
    import ctypes

    from ape_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.ape_hip_abi_version() == 5
    W_ = lib.ape_hip_poly_workspace_words
    assert W_(2, 3, 8, 8) == 5 and W_(1, 1, 1, 1) == 2 and W_(0, 0, 5, 13) == 0 and W_(1, 0, 65, 1) == 2
    assert W_(-1, 0, 4, 4) < 0 and W_(1, 1, 0, 4) < 0 and W_(1, 1, 65536, 65536) < 0 and W_(60000, 60000, 4096, 4096) < 0
    one = ctypes.c_void_p(4096)                                              # never dereferenced: every call below fails its checks
    R = lib.ape_hip_poly_rasterize
    assert R(one, 3, one, 1, one, 0, 4, 4, one, one, one, None) == 0         # nobj == 0: a no-op
    assert R(one, 3, one, 1, one, -1, 4, 4, one, one, one, None) == -1
    assert R(one, 3, one, 1, one, 1, 0, 4, one, one, one, None) == -1
    assert R(one, 3, one, 1, one, 1, 65536, 65536, one, one, one, None) == -1
    assert R(one, 3, one, 1, None, 1, 4, 4, one, one, one, None) == -1       # null poly_offsets
    assert R(one, 3, None, 1, one, 1, 4, 4, one, one, one, None) == -1       # null vert_offsets
    assert R(None, 3, one, 1, one, 1, 4, 4, one, one, one, None) == -1       # vertices without coordinates
    assert R(one, 3, one, 0, one, 1, 4, 4, one, one, one, None) == -1        # vertices without polygons
    assert R(one, 3, one, 1, one, 1, 4, 4, ctypes.c_void_p(4100), one, one, None) == -1          # a workspace that is not 8-byte aligned
    assert b"ape_hip_poly_rasterize" in lib.ape_hip_last_error()
