"""What the metric families share: reading an `Instances`, choosing the device, the torch.distributed steps, the one-call wrappers'
loops and the float64 box IoU.  No state lives here; each accumulator keeps its own (`_state` / `_row`)."""
import torch

_AREAS = ("", "s", "m", "l")                              # all, small, medium, large: the order of ops.BOX_COVER_RANGES (= ops.COCO_RANGES)


def _default_device():
    return torch.device("cuda" if torch.cuda.is_available() else "cpu")


def pick_device(explicit, *candidates):
    """`explicit` if given, else the device of the first CUDA tensor among `candidates` (anything else is skipped), else the default
    device.  Reads `.is_cuda` and `.device` only: never a synchronisation."""
    if explicit is not None:
        return explicit
    for t in candidates:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return _default_device()


def _is_instances(x):
    return hasattr(x, "has") and hasattr(x, "get_fields")


def instance_fields(inst, kind, who):
    """(pred, scores, classes) of a detectron2-style `Instances`.  kind "masks": pred is `pred_masks`, or else `list(pred_masks_rle)`;
    kind "boxes": pred is `pred_boxes`.  `scores` / `pred_classes` are None where the instances do not carry them."""
    if kind == "boxes":
        if not inst.has("pred_boxes"):
            raise ValueError(f"{who}: the instances carry no pred_boxes")
        pred = inst.pred_boxes
    elif inst.has("pred_masks"):
        pred = inst.pred_masks
    elif inst.has("pred_masks_rle"):
        pred = list(inst.pred_masks_rle)
    else:
        raise ValueError(f"{who}: the instances carry neither pred_masks nor pred_masks_rle")
    return pred, (inst.scores if inst.has("scores") else None), (inst.pred_classes if inst.has("pred_classes") else None)


def optional_tail(t, n):
    """the first n items of `t`, with None for those it does not have"""
    return (tuple(t) + (None,) * n)[:n]


def run_pairs(acc, detections, ground_truth):
    """the one-call form of a mask accumulator: detections = per image (masks, scores, classes), ground_truth = per image (masks, classes)"""
    for (dm, ds, dc), (gm, gc) in zip(detections, ground_truth):
        acc.update(dm, ds, dc, gm, gc)
    return acc.compute()


def _all_reduce_sum(t, group):
    """in-place sum of `t` over `group`; a device tensor travels through the host when the group's backend is gloo"""
    import torch.distributed as dist
    if t.is_cuda and dist.get_backend(group) == "gloo":
        h = t.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
        t.copy_(h)
    else:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)


def _distributed():
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized()


def gather_objects(obj, group=None):
    """torch.distributed.all_gather_object: every rank's `obj`, as a list in rank order, on every rank"""
    import torch.distributed as dist
    parts = [None] * dist.get_world_size(group)
    dist.all_gather_object(parts, obj, group=group)
    return parts


def _label_map(t, device):
    """an integer label map on `device` (a host map is uploaded, as `encode_masks` does), flattened"""
    if t.device != device:
        t = t.to(device)
    return t.contiguous().reshape(-1)


def _has_polygons(masks):
    """a list of COCO `segmentation` entries of which at least one is in polygon form (a list of flat coordinate lists)"""
    return isinstance(masks, (list, tuple)) and any(isinstance(s, (list, tuple)) for s in masks)


def mask_size(image_size, *sources):
    """(H, W) of an image's masks: `image_size` if given, else the size of the first tensor among `sources` ([.., H, W]), else the `size`
    of the first RLE dict in or among them, else None.  Shapes and host dicts only: never a synchronisation."""
    if image_size is not None:
        if len(image_size) != 2:
            raise ValueError(f"image_size is (H, W), got {image_size!r}")
        return int(image_size[0]), int(image_size[1])
    for s in sources:
        if torch.is_tensor(s) and s.dim() >= 2:
            return int(s.shape[-2]), int(s.shape[-1])
    for s in sources:
        for r in ([s] if isinstance(s, dict) else s if isinstance(s, (list, tuple)) else ()):
            if isinstance(r, dict) and "size" in r:
                return int(r["size"][0]), int(r["size"][1])
    return None


def _device_masks(masks, device=None, size=None):
    """[n, H, W] masks on the device from a device tensor, a host tensor (uploaded), a list of RLE dicts (decoded) or a list of COCO
    `segmentation` entries holding polygons (rasterised at `size` = (H, W), `segmentations_to_masks`); None for an empty list, which
    has no size"""
    if isinstance(masks, (list, tuple)):
        from .wire import decode_masks, segmentations_to_masks    # here, not at the top: wire imports this module
        if _has_polygons(masks):
            if size is None:
                raise ValueError("polygon ground truth has no size of its own: pass image_size=(H, W)")
            return segmentations_to_masks(masks, size[0], size[1], device)
        return decode_masks(masks, device) if len(masks) > 0 else None
    if masks.dim() != 3:
        raise ValueError(f"masks must be [n, H, W], got {tuple(masks.shape)}")
    if not masks.is_cuda:
        masks = masks.to(pick_device(device))
    return masks.contiguous()


def _coco_box_iou(db, gb, crowd=None):
    """XYXY boxes db [n, 4], gb [m, 4] float64 on one device -> (iou [n, m], area_det [n], area_gt [m]), the areas w * h with negative
    sides taken as 0, one rounding per operation.  With crowd bool [m], a crowd column holds inter / area_det."""
    area_d = (db[:, 2] - db[:, 0]).clamp_min(0) * (db[:, 3] - db[:, 1]).clamp_min(0)
    area_g = (gb[:, 2] - gb[:, 0]).clamp_min(0) * (gb[:, 3] - gb[:, 1]).clamp_min(0)
    lt = torch.maximum(db[:, None, :2], gb[None, :, :2])
    rb = torch.minimum(db[:, None, 2:], gb[None, :, 2:])
    inter = (rb - lt).clamp_min(0).prod(-1)
    iou = inter / (area_d[:, None] + area_g[None, :] - inter).clamp_min(1e-300)
    if crowd is not None:
        iou = torch.where(crowd[None, :], inter / area_d[:, None].clamp_min(1e-300), iou)
    return iou, area_d, area_g
