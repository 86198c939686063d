"""Evaluator wire format: `instances_to_coco_json`, the function every evaluator of the reference and its
demo call on a model's output (ape/evaluation/d3_evaluation.py:441-493, refcoco_evaluation.py:425-477, the detectron2
original used by lvis_evaluation.py:96 / multi_dataset_evaluator.py:173 / demo/demo_lazy.py:189-198): one dict per
detection with `image_id`, `category_id`, `bbox` (XYWH), `score` and `segmentation` = COCO RLE
`{"size": [h, w], "counts": str}`.

The reference encodes each full-resolution mask on the host with pycocotools after a ~1 MB-per-mask device-to-host copy.
Here the run lengths are produced on the device (`ape_hip_rle_encode`, csrc/imageio.hip) and only they travel; the string
form is the library's host function `ape_hip_rle_to_string`.  Three sources, in this order:
  * `instances.pred_masks_rle` -- already encoded by the runtime (`GraphedForward(mask_format="rle")`);
  * `instances.pred_masks` on the device -- encoded here;
  * `instances.pred_masks` on the host (the reference's output contract) -- uploaded, then encoded (there is no host
    encoder in this package).

The annotations' side of the same format: a COCO `segmentation` is an RLE dict or a list of polygons, and the reference makes a mask of
either with pycocotools' annToRLE (ape/evaluation/refcocoeval.py:127-131).  `segmentations_to_masks` does that on the device: RLE dicts
through `decode_masks`, polygons through `ops.poly_rasterize` (csrc/polygon.hip: rleFrPoly pixel for pixel, the union per object), fed by
`pack_polygons`, which only flattens the lists on the host.
"""
import numpy as np
import torch

from .. import ops
from ._common import _default_device


def encode_masks(masks, cap=4096):
    """[n, H, W] bool / uint8 masks (device, or host -> uploaded to the current device) -> list of COCO RLE dicts with
    `counts` as bytes (what pycocotools' encode returns)"""
    n = masks.shape[0]
    if n == 0:
        return []
    if not masks.is_cuda:
        masks = masks.to("cuda", non_blocking=False)
    masks = masks.contiguous()
    H, W = masks.shape[1:]
    out = [None] * n
    todo = list(range(n))
    while todo:
        sub = masks if len(todo) == n else masks[torch.tensor(todo, device=masks.device)]
        counts, nruns = ops.rle_encode(sub, cap=cap)
        nr = nruns.cpu()
        hc = counts[:, : int(min(cap, int(nr.max())))].cpu()
        again = []
        for j, i in enumerate(todo):
            r = int(nr[j])
            if r > cap:
                again.append(i)                                   # truncated: a mask with more runs than the buffer holds
                continue
            out[i] = {"size": [H, W], "counts": ops.rle_to_string(hc[j, :r])}
        todo = again
        cap *= 8
    return out


def rles_from_runs(counts, nruns, size):
    """host run-length arrays ([n, cap] int32, [n]) as produced by the runtime -> list of RLE dicts (counts as bytes)"""
    return [{"size": [int(size[0]), int(size[1])], "counts": ops.rle_to_string(counts[i, : int(nruns[i])])}
            for i in range(counts.shape[0])]


def decode_masks(rles, device=None):
    """list of COCO RLE dicts {"size": [h, w], "counts": bytes | str | list of run lengths} of ONE size -> uint8 [n, h, w] on the
    device, the inverse of `encode_masks`: the strings become run lengths on the host (`ops.rle_from_string`), only the runs
    travel, and `ops.rle_decode` writes the masks.  An uncompressed `counts` list (COCO's other form) is taken as it is."""
    rles = list(rles)
    if not rles:
        raise ValueError("decode_masks: an empty list has no size; build the [0, h, w] tensor yourself")
    size = [int(v) for v in rles[0]["size"]]
    runs = []
    for r in rles:
        if [int(v) for v in r["size"]] != size:
            raise ValueError(f"decode_masks: masks of size {list(r['size'])} and {size} in one call")
        c = r["counts"]
        if isinstance(c, (bytes, bytearray, str)):
            runs.append(ops.rle_from_string(c))
        else:
            runs.append(torch.as_tensor(c, dtype=torch.int64).reshape(-1).to(torch.int32))
    cap = max(1, max(int(c.numel()) for c in runs))
    counts = torch.zeros((len(runs), cap), dtype=torch.int32)
    for i, c in enumerate(runs):
        counts[i, : c.numel()] = c
    nruns = torch.tensor([int(c.numel()) for c in runs], dtype=torch.int32)
    device = _default_device() if device is None else torch.device(device)
    return ops.rle_decode(counts.to(device), nruns.to(device), size[0], size[1])


_POLY_COORD_MAX = 65536.0                                 # 5 * c stays far inside int32, and the boundary walk of an edge stays bounded


def _is_polygons(seg):
    """a COCO `segmentation` in polygon form: a list (possibly empty) of flat coordinate lists; the other form is an RLE dict"""
    return isinstance(seg, (list, tuple))


def pack_polygons(segmentations):
    """host: one entry per object, each a list of polygons, each polygon flat [x0, y0, x1, y1, ...] (COCO's `segmentation`) -> the three
    host tensors `ops.poly_rasterize` takes: xy float64 [V, 2], vert_offsets int32 [P + 1], poly_offsets int32 [n + 1].  ValueError for
    a polygon with an odd length or fewer than 6 numbers, a coordinate that is not finite, or |coordinate| > 65536."""
    flat, owner, vert_offsets, poly_offsets = [], [], [0], [0]
    for i, polys in enumerate(segmentations):
        if not _is_polygons(polys):
            raise ValueError(f"pack_polygons: object {i} is not a list of polygons ({type(polys).__name__})")
        for poly in polys:
            c = np.asarray(poly, dtype=np.float64).reshape(-1)
            if c.size % 2 != 0 or c.size < 6:
                raise ValueError(f"pack_polygons: a polygon of object {i} has {c.size} numbers (an even count, at least 6)")
            flat.append(c)
            owner.append(i)
            vert_offsets.append(vert_offsets[-1] + c.size // 2)
        poly_offsets.append(len(flat))
    xy = np.concatenate(flat) if flat else np.zeros(0, dtype=np.float64)
    bad = ~(np.abs(xy) <= _POLY_COORD_MAX)                    # one pass over all coordinates; a NaN fails the comparison too
    if bad.any():
        at = int(np.argmax(bad))
        i = owner[int(np.searchsorted(vert_offsets, at // 2, side="right")) - 1]
        what = "that is not finite" if not np.isfinite(xy[at]) else f"beyond +-{_POLY_COORD_MAX:.0f}"
        raise ValueError(f"pack_polygons: a polygon of object {i} has a coordinate {what}")
    return (torch.from_numpy(xy.reshape(-1, 2)), torch.tensor(vert_offsets, dtype=torch.int32),
            torch.tensor(poly_offsets, dtype=torch.int32))


def segmentations_to_masks(segmentations, height, width, device=None, return_area=False):
    """COCO `segmentation` entries of ONE image -> uint8 [n, height, width] on the device, in input order: what pycocotools' annToRLE +
    decode give (the reference's ground truth, ape/evaluation/refcocoeval.py:127-131).  An entry is a polygon list (rasterised by ONE
    `ops.poly_rasterize` call for all of them, rleFrPoly pixel for pixel) or an RLE dict in any form `decode_masks` takes (ONE
    `decode_masks` call; its size must be (height, width)).  return_area: also the foreground counts, int64 [n] on the device."""
    segmentations = list(segmentations)
    height, width = int(height), int(width)
    device = _default_device() if device is None else torch.device(device)
    n = len(segmentations)
    polys = [i for i, s in enumerate(segmentations) if _is_polygons(s)]
    rles = [i for i, s in enumerate(segmentations) if isinstance(s, dict)]
    if len(polys) + len(rles) != n:
        bad = next(s for s in segmentations if not _is_polygons(s) and not isinstance(s, dict))
        raise ValueError(f"segmentations_to_masks: an entry is a polygon list or an RLE dict, got {type(bad).__name__}")
    for i in rles:
        if [int(v) for v in segmentations[i]["size"]] != [height, width]:
            raise ValueError(f"segmentations_to_masks: an RLE of size {list(segmentations[i]['size'])} in an image of {[height, width]}")
    if n == 0:
        out = torch.zeros((0, height, width), dtype=torch.uint8, device=device)
        return (out, torch.zeros(0, dtype=torch.int64, device=device)) if return_area else out
    pm = pa = rm = None
    if polys:
        xy, vert_offsets, poly_offsets = pack_polygons([segmentations[i] for i in polys])
        pm, pa = ops.poly_rasterize(xy.to(device), vert_offsets.to(device), poly_offsets.to(device), height, width)
    if rles:
        rm = decode_masks([segmentations[i] for i in rles], device)
    if not rles:
        out, area = pm, pa
    else:
        out = torch.empty((n, height, width), dtype=torch.uint8, device=device)
        out[torch.tensor(rles, device=device)] = rm
        if polys:
            out[torch.tensor(polys, device=device)] = pm
        area = out.flatten(1).sum(1, dtype=torch.int64) if return_area else None
    return (out, area) if return_area else out


def instances_to_coco_json(instances, img_id):
    """d3_evaluation.py:441-493 with the mask encoding on the device"""
    num_instance = len(instances)
    if num_instance == 0:
        return []
    b = instances.pred_boxes.tensor.detach().cpu().clone()
    b[:, 2] -= b[:, 0]                       # BoxMode.XYXY_ABS -> XYWH_ABS
    b[:, 3] -= b[:, 1]
    boxes = b.tolist()
    scores = instances.scores.tolist()
    classes = instances.pred_classes.tolist()
    rles = None
    if instances.has("pred_masks_rle"):
        rles = [dict(r) for r in instances.pred_masks_rle]
    elif instances.has("pred_masks"):
        rles = encode_masks(instances.pred_masks)
    if rles is not None:
        for r in rles:                       # json cannot hold bytes; utf-8 is what pycocotools' _mask.pyx does too (:471-475)
            if isinstance(r["counts"], bytes):
                r["counts"] = r["counts"].decode("utf-8")
    results = []
    for k in range(num_instance):
        result = {"image_id": img_id, "category_id": classes[k], "bbox": boxes[k], "score": scores[k]}
        if rles is not None:
            result["segmentation"] = rles[k]
        results.append(result)
    return results
