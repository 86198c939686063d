"""COCO-style AP with the area range "all" and no crowd regions: `_coco_ap`, the protocol, and what feeds it an IoU matrix per
image -- boxes (`box_ap`, the benchmark's score), masks (`MaskAPAccumulator`) and min(mask, boundary) IoU (`BoundaryAPAccumulator`)."""
import torch

from .. import ops
from ._common import (_coco_box_iou, _device_masks, _distributed, _is_instances, gather_objects, instance_fields, mask_size,
                      run_pairs)


def _iou_matrix(a, b):
    """pairwise IoU of XYXY boxes a [n, 4], b [m, 4] (float64)"""
    return _coco_box_iou(a.double(), b.double())[0]


# `_coco_ap` and `coco.coco_metrics` both turn matches into precision at 101 recall points, and stay two functions on purpose: this one
# is torch (`torch.linspace` recall points, a 1e-300 clamp, the FIRST ground truth on an IoU tie), that one numpy as COCOeval has it
# (`numpy.linspace`, `numpy.spacing(1)`, the LAST ground truth).  Merging them would change bits of one; tests pin both.
def _coco_ap(records, iou_thresholds=None, max_dets=100):
    """The protocol part of `box_ap` and `mask_ap`: records is a list (one entry per image) of (scores [n], classes [n],
    gt_classes [m], iou [n, m] float64) on the host, detections in any order.  Greedy matching per (image, class) in score order,
    the monotone precision envelope and its 101 recall points, averaged over thresholds and over the classes with ground truth."""
    if iou_thresholds is None:
        iou_thresholds = [0.5 + 0.05 * i for i in range(10)]
    T = len(iou_thresholds)
    thr = torch.tensor(iou_thresholds, dtype=torch.float64)
    per_class = {}                      # class -> list of (scores [n], matched [T, n]) per image, and the GT count
    n_gt = {}
    for ds, dc, gc, full in records:
        order = torch.argsort(ds, descending=True, stable=True)
        ds, dc, full = ds[order], dc[order], full[order]
        for c in set(dc.tolist()) | set(gc.tolist()):
            d_idx, g_idx = (dc == c).nonzero().flatten()[:max_dets], (gc == c).nonzero().flatten()
            n_gt[c] = n_gt.get(c, 0) + int(g_idx.numel())
            if d_idx.numel() == 0:
                continue
            matched = torch.zeros((T, d_idx.numel()), dtype=torch.bool)
            if g_idx.numel() > 0:
                iou = full[d_idx][:, g_idx]
                for t in range(T):
                    taken = torch.zeros(g_idx.numel(), dtype=torch.bool)
                    for i in range(d_idx.numel()):                       # detections are in descending score order
                        cand = iou[i].clone()
                        cand[taken] = -1.0
                        j = int(cand.argmax())
                        if cand[j] >= min(float(thr[t]), 1 - 1e-10):
                            taken[j] = True
                            matched[t, i] = True
            per_class.setdefault(c, []).append((ds[d_idx], matched))
    rec_thrs = torch.linspace(0.0, 1.0, 101, dtype=torch.float64)
    aps = []
    for c, total in n_gt.items():
        if total == 0:
            continue
        entries = per_class.get(c, [])
        if not entries:
            aps.append(torch.zeros(T, dtype=torch.float64))
            continue
        scores = torch.cat([e[0] for e in entries])
        matched = torch.cat([e[1] for e in entries], dim=1)
        order = torch.argsort(scores, descending=True, stable=True)
        tp = matched[:, order].double().cumsum(1)
        fp = (~matched[:, order]).double().cumsum(1)
        recall = tp / total
        precision = tp / (tp + fp).clamp_min(1e-300)
        ap_t = torch.zeros(T, dtype=torch.float64)
        for t in range(T):
            pr = torch.flip(torch.cummax(torch.flip(precision[t], [0]), 0)[0], [0])        # monotone non-increasing envelope
            idx = torch.searchsorted(recall[t].contiguous(), rec_thrs, right=False)
            q = torch.where(idx < pr.numel(), pr[idx.clamp_max(pr.numel() - 1)], torch.zeros_like(rec_thrs))
            ap_t[t] = q.mean()
        aps.append(ap_t)
    if not aps:
        return {"AP": float("nan"), "AP50": float("nan"), "AP75": float("nan"), "classes": 0, "gt": 0, "dets": 0}
    A = torch.stack(aps)                                                                    # [classes, T]
    pick = lambda v: float(A[:, min(range(T), key=lambda i: abs(iou_thresholds[i] - v))].mean())   # noqa: E731
    return {"AP": float(A.mean()), "AP50": pick(0.5), "AP75": pick(0.75), "classes": int(A.shape[0]),
            "gt": int(sum(n_gt.values())), "dets": int(sum(e[0].numel() for es in per_class.values() for e in es))}


def box_ap(detections, ground_truth, iou_thresholds=None, max_dets=100):
    """COCO-style box AP of `detections` against `ground_truth` (the protocol of pycocotools' COCOeval that the reference's
    evaluators run -- ape/evaluation/lvis_evaluation.py / detectron2's COCOEvaluator -- restated: area range "all", no crowd
    regions, at most `max_dets` detections per (image, CATEGORY) -- COCOeval applies maxDets inside its per-category evaluateImg, so a
    model top-k of 300 / 500 loses nothing to the default 100 --, IoU thresholds 0.50:0.05:0.95, greedy matching in score order to the
    unmatched ground truth of the same class with the highest IoU, precision made monotone and sampled at 101 recall points,
    averaged over thresholds and over the classes that have ground truth).  pycocotools is not installable here: unpinned.

    detections: list (one entry per image) of (boxes [n, 4] XYXY, scores [n], classes [n]);
    ground_truth: list of (boxes [m, 4] XYXY, classes [m]).  -> dict(AP, AP50, AP75, classes, gt, dets)."""
    records = []
    for (db, ds, dc), (gb, gc) in zip(detections, ground_truth):
        db, ds, dc = db.detach().cpu().double(), ds.detach().cpu().double(), dc.detach().cpu().long()
        gb, gc = gb.detach().cpu().double(), gc.detach().cpu().long()
        if ds.numel() > 0 and gc.numel() > 0:
            iou = _iou_matrix(db, gb)
        else:
            iou = torch.zeros((ds.numel(), gc.numel()), dtype=torch.float64)
        records.append((ds, dc, gc, iou))
    return _coco_ap(records, iou_thresholds, max_dets)


# ------------------------------------------------------------------------------------------------------------------
# Instance masks.  The IoU matrix of an image's detections against its ground truth is counted on the device by
# `ops.mask_pair_iou` (csrc/maskiou.hip: one bit pack per side, one popcount contraction); only the [n, m] matrix travels.
# The protocol that follows is `_coco_ap`, the same code `box_ap` runs.
# ------------------------------------------------------------------------------------------------------------------
class MaskAPAccumulator:
    """COCO-style mask AP of a dataset: the protocol `box_ap` documents, with mask IoU in place of box IoU.  `update` packs each side
    of an image once, counts the whole n x m intersection matrix in one launch (`ops.mask_pair_iou`) and keeps only the image's small
    host record -- scores, classes and the IoU matrix; the per-class greedy matching stays on the host, in `compute`.
    Ground-truth masks may be COCO polygons (rasterised on the device as pycocotools' annToRLE does: `update`'s `image_size`).
    Out of scope, as for `box_ap`: crowd regions, area ranges (APs / APm / APl) and the LVIS federated protocol.  pycocotools is not a dependency of this package: unpinned."""

    def __init__(self, iou_thresholds=None, max_dets=100, device=None):
        self.iou_thresholds = None if iou_thresholds is None else [float(t) for t in iou_thresholds]
        self.max_dets = int(max_dets)
        self.device = None if device is None else torch.device(device)
        self.records = []

    def update(self, pred, scores=None, classes=None, gt_masks=None, gt_classes=None, image_size=None):
        """pred: masks [n, H, W] (uint8 / bool; device tensor, host tensor or list of RLE dicts) with `scores` [n] and `classes` [n],
        or an `Instances` carrying `pred_masks` or `pred_masks_rle` next to `scores` and `pred_classes`;
        gt_masks: [m, H, W] in any of the three forms, or a list of COCO `segmentation` entries with polygon lists among them, which
        are rasterised at image_size = (H, W) -- by default the prediction masks' size, else the size of an RLE dict among the inputs;
        gt_classes [m]"""
        if _is_instances(pred):
            pred, inst_scores, inst_classes = instance_fields(pred, "masks", "MaskAPAccumulator.update")
            scores = inst_scores if scores is None else scores
            classes = inst_classes if classes is None else classes
        if scores is None or classes is None or gt_masks is None or gt_classes is None:
            raise ValueError("MaskAPAccumulator.update: scores, classes, gt_masks and gt_classes are all needed")
        ds = torch.as_tensor(scores).detach().cpu().double().reshape(-1)
        dc = torch.as_tensor(classes).detach().cpu().long().reshape(-1)
        gc = torch.as_tensor(gt_classes).detach().cpu().long().reshape(-1)
        n, m = len(pred), len(gt_masks)
        if ds.numel() != n or dc.numel() != n or gc.numel() != m:
            raise ValueError(f"MaskAPAccumulator.update: {n} masks with {ds.numel()} scores and {dc.numel()} classes; "
                             f"{m} ground-truth masks with {gc.numel()} classes")
        if n == 0 or m == 0:
            iou = torch.zeros((n, m), dtype=torch.float64)
        else:
            a = _device_masks(pred, self.device)
            b = _device_masks(gt_masks, a.device, mask_size(image_size, a, pred, gt_masks))
            if tuple(a.shape[1:]) != tuple(b.shape[1:]):
                raise ValueError(f"MaskAPAccumulator.update: prediction masks {tuple(a.shape[1:])} vs ground truth {tuple(b.shape[1:])}")
            iou = self._pair_iou(a, b)
        self.records.append((ds, dc, gc, iou))

    def _pair_iou(self, a, b):
        """the matching IoU of two non-empty mask sets on one device, a [n, H, W] and b [m, H, W] -> float64 [n, m] on the host"""
        return ops.mask_pair_iou(a, b)[0].cpu()

    def reduce(self, group=None):
        """gather every rank's records (torch.distributed.all_gather_object; every rank ends with all of them, in rank order); a
        no-op in a process without a process group"""
        if _distributed():
            self.records = [r for part in gather_objects(self.records, group) for r in part]

    def compute(self):
        """dict(AP, AP50, AP75, classes, gt, dets), the keys of `box_ap`"""
        return _coco_ap(self.records, self.iou_thresholds, self.max_dets)


def mask_ap(detections, ground_truth, iou_thresholds=None, max_dets=100):
    """COCO-style mask AP (see `MaskAPAccumulator`, which implements it; the protocol is `box_ap`'s).
    detections: list (one entry per image) of (masks, scores [n], classes [n]); ground_truth: list of (masks, classes [m]); masks is a
    [n, H, W] uint8 / bool tensor on the device, a host tensor (uploaded) or a list of RLE dicts (decoded on the device).
    -> dict(AP, AP50, AP75, classes, gt, dets)."""
    return run_pairs(MaskAPAccumulator(iou_thresholds, max_dets), detections, ground_truth)


# ------------------------------------------------------------------------------------------------------------------
# Mask boundaries.  Boundary IoU (Cheng et al., CVPR 2021) is the IoU of the two masks' inner boundary bands, d = 2 % of the image
# diagonal wide; Boundary AP matches on min(mask IoU, boundary IoU).  The bands are made on the device from row-packed bits
# (`ops.boundary_pair_iou`, csrc/boundary.hip) and contracted by the same popcount kernel as the masks; only the [n, m] matrix travels.
# ------------------------------------------------------------------------------------------------------------------
def boundary_iou(a, b, dilation_ratio=0.02, dilation=None, device=None, image_size=None):
    """Boundary IoU matrix of two mask sets of one size, float64 [n, m] on the device: the IoU of the inner boundary bands, each
    `dilation` pixels wide (default: `dilation_ratio` of the image diagonal, `ops.boundary_dilation`), 0 where both bands are empty.
    The published `boundary_iou` package restated (not installable here: unpinned, like `box_ap`).  a, b: [n, H, W] uint8 / bool on
    the device, host tensors (uploaded), lists of RLE dicts (decoded on the device) or lists of COCO `segmentation` entries with
    polygon lists among them (rasterised at image_size = (H, W); default: the size of a tensor or an RLE dict among the inputs)."""
    size = mask_size(image_size, a, b)
    a = _device_masks(a, device, size)
    if a is None:
        raise ValueError("boundary_iou: an empty list has no size; build the [0, h, w] tensor yourself")
    b = _device_masks(b, a.device, size)
    if b is None:
        raise ValueError("boundary_iou: an empty list has no size; build the [0, h, w] tensor yourself")
    return ops.boundary_pair_iou(a, b, dilation_ratio, dilation)[0]


class BoundaryAPAccumulator(MaskAPAccumulator):
    """COCO-style Boundary AP of a dataset (the second segmentation metric of the LVIS challenge): `MaskAPAccumulator` with the matching
    IoU min(mask IoU, boundary IoU), both counted on the device in `ops.boundary_pair_iou` -- one row pack and one erosion per side,
    two popcount contractions.  Inputs, `update` / `reduce` / `compute` and the result keys are `MaskAPAccumulator`'s.
    Out of scope, like its siblings: crowd regions, area ranges (APs / APm / APl), the LVIS federated protocol and boundary PQ.  The `boundary_iou` package is not a dependency of this package: unpinned."""

    def __init__(self, iou_thresholds=None, max_dets=100, device=None, dilation_ratio=0.02):
        super().__init__(iou_thresholds, max_dets, device)
        self.dilation_ratio = float(dilation_ratio)

    def _pair_iou(self, a, b):
        biou, iou = ops.boundary_pair_iou(a, b, self.dilation_ratio)[:2]
        return torch.minimum(iou, biou).cpu()


def boundary_ap(detections, ground_truth, iou_thresholds=None, max_dets=100, dilation_ratio=0.02):
    """COCO-style Boundary AP (see `BoundaryAPAccumulator`, which implements it): `mask_ap` with min(mask IoU, boundary IoU) as the
    matching IoU.  detections / ground_truth as for `mask_ap`.  -> dict(AP, AP50, AP75, classes, gt, dets)."""
    return run_pairs(BoundaryAPAccumulator(iou_thresholds, max_dets, dilation_ratio=dilation_ratio), detections, ground_truth)
