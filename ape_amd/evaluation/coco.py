"""COCO's full detection protocol (pycocotools' COCOeval, what the reference's instance_evaluation.py / d3_evaluation.py and detectron2's
COCOEvaluator run): crowd regions, the four area ranges, AP / AP50 / AP75 / APs / APm / APl and AR@1 / @10 / @100 / ARs / ARm / ARl.
`box_ap` / `mask_ap` (ap.py) stay what they are (no crowd, area range all, first-of-a-tie); this is a separate route.  The matching of
`evaluateImg` runs on the device for all classes x area ranges x thresholds of an image in one launch (`ops.coco_match`,
coco_match_kernel in csrc/boxcover.hip); `accumulate` and `summarize` are `coco_metrics`, host arithmetic on the small per-image records.
pycocotools is not a dependency of this package: unpinned."""
import numpy as np
import torch

from .. import ops
from ._common import (_AREAS, _coco_box_iou, _device_masks, _distributed, _is_instances, gather_objects, instance_fields,
                      mask_size, optional_tail, pick_device)


def coco_recall_points():
    """COCOeval's recThrs: numpy.linspace(0, 1, 101) as numpy gives them (torch.linspace differs in last bits)"""
    return np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)


def _host_array(x, dtype):
    return np.ascontiguousarray(torch.as_tensor(x).detach().cpu().numpy()).astype(dtype, copy=False)


# Not merged with `ap._coco_ap`, on purpose: this is numpy as COCOeval has it (`numpy.linspace` recall points, `numpy.spacing(1)`, the
# LAST ground truth on an IoU tie), that one torch (`torch.linspace`, a 1e-300 clamp, the FIRST).  One function for both would change
# bits of one of them; tests pin both.
def coco_metrics(records, num_classes, class_names=None, max_dets=(1, 10, 100), iou_thresholds=None):
    """COCOeval's `accumulate` and `summarize` on per-image matching results.  A pure host function.
    records: one entry per image, in update order, of (scores [n'], classes [n'], flag [A, T, n'], gt_classes [m], gt_ignore [A, m]):
    the detections grouped by class with descending score inside a class (the order of `ops.coco_match`'s det_order), their flags
    (1 true positive, 0 false positive, 2 ignored) for the A = 4 area ranges all / small / medium / large and T thresholds
    (`iou_thresholds`, default COCO's ten -- only used to find the columns of AP50 and AP75), and per range which ground truth is ignored.
    For each class k, range a and limit M: every image's first M detections of k, concatenated in image order and put in descending
    score order by a stable sort; tp / fp = running counts of flags 1 / 0; npig = the not-ignored ground truth of k under a; recall =
    tp / npig, precision = tp / (fp + tp + numpy.spacing(1)) made monotone from the right and sampled at the 101 recall points with
    searchsorted(side="left"), 0 past the end.  npig == 0 leaves the entry out of every mean (COCOeval's -1).
    -> dict of fractions (NaN where COCOeval reports -1): AP, AP50, AP75, APs, APm, APl at the last limit, AR@M for every limit, ARs,
    ARm, ARl at the last, `AP-<name>` per class when `class_names` is given, and the counts images, gt (all ground truth, ignored or
    not), dets (inside the largest limit) and classes (those with ground truth that counts under "all")."""
    K = int(num_classes)
    max_dets = tuple(int(v) for v in max_dets)
    thr = list(ops.COCO_THRESHOLDS if iou_thresholds is None else [float(v) for v in iou_thresholds])
    if K <= 0 or not max_dets or any(v <= 0 for v in max_dets) or not thr:
        raise ValueError("coco_metrics: num_classes and max_dets must be positive, and there must be thresholds")
    if class_names is not None and len(class_names) != K:
        raise ValueError(f"coco_metrics: {len(class_names)} class names for {K} classes")
    A, T, M = len(_AREAS), len(thr), len(max_dets)
    rec_thrs = coco_recall_points()
    R = rec_thrs.size
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    npig = np.zeros((K, A), dtype=np.int64)
    scores, classes, ranks, flags = [], [], [], []
    n_gt = 0
    for i, rec in enumerate(records):
        ds, dc, fl = _host_array(rec[0], np.float64).reshape(-1), _host_array(rec[1], np.int64).reshape(-1), _host_array(rec[2], np.uint8)
        gc, gi = _host_array(rec[3], np.int64).reshape(-1), _host_array(rec[4], np.uint8)
        n, m = ds.size, gc.size
        if dc.size != n or fl.shape != (A, T, n) or gi.shape != (A, m):
            raise ValueError(f"coco_metrics: image {i}: {n} scores, {dc.size} classes, flag {fl.shape} (want {(A, T, n)}), "
                             f"{m} gt classes, gt_ignore {gi.shape} (want {(A, m)})")
        if (n and (dc.min() < 0 or dc.max() >= K)) or (m and (gc.min() < 0 or gc.max() >= K)):
            raise ValueError(f"coco_metrics: image {i}: a class outside 0 .. {K - 1}")
        n_gt += m
        for a in range(A):
            npig[:, a] += np.bincount(gc[gi[a] == 0], minlength=K)
        order = np.argsort(dc, kind="stable")
        first = np.searchsorted(dc[order], dc[order], side="left")
        rank = np.empty(n, dtype=np.int64)
        rank[order] = np.arange(n) - first                               # position among the image's detections of the same class
        scores.append(ds)
        classes.append(dc)
        ranks.append(rank)
        flags.append(fl)
    S = np.concatenate(scores) if scores else np.zeros(0)
    C = np.concatenate(classes) if classes else np.zeros(0, dtype=np.int64)
    RK = np.concatenate(ranks) if ranks else np.zeros(0, dtype=np.int64)
    F = np.concatenate(flags, axis=2) if flags else np.zeros((A, T, 0), dtype=np.uint8)
    by_class = np.argsort(C, kind="stable")                              # image order, then record order, inside a class
    bounds = np.searchsorted(C[by_class], np.arange(K + 1), side="left")
    eps = np.spacing(1)
    for k in range(K):
        if not npig[k].any():
            continue
        idx = by_class[bounds[k]: bounds[k + 1]]
        for mi, limit in enumerate(max_dets):
            sel = idx[RK[idx] < limit]
            sel = sel[np.argsort(-S[sel], kind="mergesort")]
            nd = sel.size
            f = F[:, :, sel]
            tps = np.cumsum(f == 1, axis=2).astype(np.float64)
            fps = np.cumsum(f == 0, axis=2).astype(np.float64)
            for a in range(A):
                if npig[k, a] == 0:
                    continue
                if nd == 0:
                    recall[:, k, a, mi] = 0.0
                    precision[:, :, k, a, mi] = 0.0
                    continue
                for t in range(T):
                    tp, fp = tps[a, t], fps[a, t]
                    rc = tp / npig[k, a]
                    pr = tp / (fp + tp + eps)
                    recall[t, k, a, mi] = rc[-1]
                    pr = np.maximum.accumulate(pr[::-1])[::-1]
                    inds = np.searchsorted(rc, rec_thrs, side="left")
                    q = np.zeros(R)
                    inside = inds < nd
                    q[inside] = pr[inds[inside]]
                    precision[t, :, k, a, mi] = q

    def mean(v):
        v = v[v > -1]
        return float(v.mean()) if v.size else float("nan")

    def at(value):
        return min(range(T), key=lambda i: abs(thr[i] - value))
    res = {"AP": mean(precision[:, :, :, 0, -1]), "AP50": mean(precision[at(0.5), :, :, 0, -1]), "AP75": mean(precision[at(0.75), :, :, 0, -1])}
    for a in range(1, A):
        res[f"AP{_AREAS[a]}"] = mean(precision[:, :, :, a, -1])
    for mi, limit in enumerate(max_dets):
        res[f"AR@{limit}"] = mean(recall[:, :, 0, mi])
    for a in range(1, A):
        res[f"AR{_AREAS[a]}"] = mean(recall[:, :, a, -1])
    if class_names is not None:
        for k, name in enumerate(class_names):
            res[f"AP-{name}"] = mean(precision[:, :, k, 0, -1])
    res.update(images=len(scores), gt=int(n_gt), dets=int((RK < max(max_dets)).sum()), classes=int((npig[:, 0] > 0).sum()))
    return res


def _coco_groups(scores, classes, gt_classes, K, limit):
    """The grouping `ops.coco_match` takes, made on the device without a read-back: scores [n], classes int64 [n], gt_classes int64 [m]
    -> (det_order int32 [n], det_offsets int32 [K + 1], gt_order int32 [m], gt_offsets int32 [K + 1], bad int64 scalar).
    Detections: descending score (stable), then class (stable), then each class cut to its first `limit`.  Shapes stay the inputs'
    -- a size that depends on data would need a read-back --: what is cut away, or has a class outside 0 .. K - 1, moves behind the
    groups, where det_offsets[K] ends what counts.  Ground truth: by class, in input order.  bad = the classes outside 0 .. K - 1."""
    dev = scores.device
    bounds = torch.arange(K + 1, device=dev)
    order = torch.sort(scores, descending=True, stable=True)[1]
    order = order[torch.sort(classes[order], stable=True)[1]]
    cls = classes[order]
    first = torch.searchsorted(cls, bounds)
    valid = (cls >= 0) & (cls < K)
    keep = valid & (torch.arange(cls.shape[0], device=dev) - first[cls.clamp(0, K - 1)] < limit)
    order = order[torch.sort((~keep).to(torch.uint8), stable=True)[1]]
    det_offsets = torch.cat([first[:1] * 0, (first[1:] - first[:-1]).clamp_max(limit).cumsum(0)]).to(torch.int32)
    gt_sorted, gt_order = torch.sort(gt_classes, stable=True)
    gt_offsets = torch.searchsorted(gt_sorted, bounds).to(torch.int32)
    bad = (~valid).sum() + ((gt_classes < 0) | (gt_classes >= K)).sum()
    return order.to(torch.int32), det_offsets, gt_order.to(torch.int32), gt_offsets, bad


class COCOAccumulator:
    """COCO box ("bbox") or mask ("segm") scores of a dataset by COCOeval's protocol: crowd regions, the four area ranges, ties to the
    last ground truth, thresholds numpy.linspace(.5, .95, 10) -- see `coco_metrics` for the keys.  `update` takes one image: it builds
    the IoU matrix on the device (boxes: `_iou_matrix`'s float64 arithmetic; masks: the integer counts of `ops.mask_pack_bits` /
    `ops.bitmask_pair_counts`; a crowd column holds inter / area_det), groups detections and ground truth by class with stable device sorts,
    cuts each class to max(max_dets) detections and runs `ops.coco_match` -- one launch for all classes x area ranges x thresholds.
    With device inputs it enqueues and never synchronises; `compute` (and `reduce`) read the small per-image results back.
    gt_areas: COCO scores with the annotation's `area`; the default is the box area ("bbox") or the mask area ("segm").  The area of a
    detection is its box w * h or its mask area.  Classes are 0 .. num_classes - 1; one outside raises ValueError, at the latest in
    `compute`.  At most 4096 ground truths and 65535 detections per image.
    Ground-truth masks may be COCO polygons (`segmentation` lists, rasterised on the device as pycocotools' annToRLE does: `update`'s
    `image_size`).  Out of scope: the LVIS federated rules, OpenImages, keypoints."""

    def __init__(self, iou_type, num_classes, max_dets=(1, 10, 100), device=None, class_names=None):
        if iou_type not in ("bbox", "segm"):
            raise ValueError(f"COCOAccumulator: iou_type is 'bbox' or 'segm', got {iou_type!r}")
        self.iou_type = iou_type
        self.num_classes = int(num_classes)
        self.max_dets = tuple(int(v) for v in max_dets)
        if self.num_classes <= 0 or not self.max_dets or any(v <= 0 for v in self.max_dets):
            raise ValueError("COCOAccumulator: num_classes and max_dets must be positive")
        if class_names is not None and len(class_names) != self.num_classes:
            raise ValueError(f"COCOAccumulator: {len(class_names)} class names for {self.num_classes} classes")
        self.class_names = None if class_names is None else list(class_names)
        self.device = None if device is None else torch.device(device)
        self.records = []                                     # host: what `coco_metrics` takes
        self._pending = []                                    # device: enqueued, not read back yet

    def update(self, pred, scores=None, classes=None, gt=None, gt_classes=None, gt_crowd=None, gt_areas=None, image_size=None):
        """One image.  pred: boxes [n, 4] XYXY ("bbox") or masks [n, H, W] as a device tensor, a host tensor or a list of RLE dicts
        ("segm"), with `scores` [n] and `classes` [n]; or an `Instances` carrying `pred_boxes` / `pred_masks` / `pred_masks_rle` next to
        `scores` and `pred_classes`.  gt: boxes [m, 4] (a tensor or a `Boxes`) or masks in any of the three forms, gt_classes [m],
        gt_crowd [m] (non-zero = a crowd region; default none), gt_areas [m] (see the class).  Host inputs are uploaded.
        "segm" ground truth may also be a list of COCO `segmentation` entries, polygon lists among them: they are rasterised at
        image_size = (H, W), by default the prediction masks' size, else the size of an RLE dict among the inputs."""
        who = "COCOAccumulator.update"
        segm = self.iou_type == "segm"
        if _is_instances(pred):
            pred, inst_scores, inst_classes = instance_fields(pred, "masks" if segm else "boxes", who)
            scores = inst_scores if scores is None else scores
            classes = inst_classes if classes is None else classes
        if scores is None or classes is None or gt is None or gt_classes is None:
            raise ValueError(f"{who}: scores, classes, gt and gt_classes are all needed")
        pred, gt = getattr(pred, "tensor", pred), getattr(gt, "tensor", gt)
        scores, classes, gt_classes = torch.as_tensor(scores).detach(), torch.as_tensor(classes).detach(), torch.as_tensor(gt_classes).detach()
        if not segm:
            pred, gt = torch.as_tensor(pred).detach(), torch.as_tensor(gt).detach()
            if pred.dim() != 2 or pred.shape[1] != 4 or gt.dim() != 2 or gt.shape[1] != 4:
                raise ValueError(f"{who}: boxes must be [n, 4] and [m, 4], got {tuple(pred.shape)} and {tuple(gt.shape)}")
        n, m = len(pred), len(gt)
        if tuple(scores.shape) != (n,) or tuple(classes.shape) != (n,) or tuple(gt_classes.shape) != (m,):
            raise ValueError(f"{who}: {n} detections with scores {tuple(scores.shape)} and classes {tuple(classes.shape)}; "
                             f"{m} ground truths with classes {tuple(gt_classes.shape)}")
        if gt_crowd is not None:
            gt_crowd = torch.as_tensor(gt_crowd).detach()
        if gt_areas is not None:
            gt_areas = torch.as_tensor(gt_areas).detach()
        for t, name in ((gt_crowd, "gt_crowd"), (gt_areas, "gt_areas")):
            if t is not None and tuple(t.shape) != (m,):
                raise ValueError(f"{who}: {name} must be [{m}], got {tuple(t.shape)}")
        if m > ops.COCO_MAX_GT or n > ops.COCO_MAX_DET:
            raise ValueError(f"{who}: {n} detections against {m} ground truths (at most {ops.COCO_MAX_DET} against {ops.COCO_MAX_GT} per image)")
        K = self.num_classes
        for t in (classes, gt_classes):                           # what lies on the host is checked now, the rest in `compute`
            if not t.is_cuda and t.numel() > 0 and (int(t.min()) < 0 or int(t.max()) >= K):
                raise ValueError(f"{who}: a class outside 0 .. {K - 1}")
        dev = self.device = pick_device(self.device, pred, gt, scores)
        crowd = torch.zeros(m, dtype=torch.bool, device=dev) if gt_crowd is None else gt_crowd.to(dev) != 0
        if not segm:
            iou, det_area, gt_area = _coco_box_iou(pred.to(dev, torch.float64), gt.to(dev, torch.float64), crowd)
        else:
            a = _device_masks(pred, dev) if n > 0 else None
            b = _device_masks(gt, dev, mask_size(image_size, pred, gt)) if m > 0 else None
            if a is not None and b is not None and tuple(a.shape[1:]) != tuple(b.shape[1:]):
                raise ValueError(f"{who}: prediction masks {tuple(a.shape[1:])} vs ground truth {tuple(b.shape[1:])}")
            a_bits, area_a = ops.mask_pack_bits(a) if n > 0 else (None, torch.zeros(0, dtype=torch.int64, device=dev))
            b_bits, area_b = ops.mask_pack_bits(b) if m > 0 else (None, torch.zeros(0, dtype=torch.int64, device=dev))
            if n > 0 and m > 0:
                iou = ops.count_iou(ops.bitmask_pair_counts(a_bits, b_bits), area_a, area_b, crowd)
            else:
                iou = torch.zeros((n, m), dtype=torch.float64, device=dev)
            det_area, gt_area = area_a.double(), area_b.double()
        if gt_areas is not None:
            gt_area = gt_areas.to(dev, torch.float64)
        scores, classes, gt_classes = scores.to(dev, torch.float64), classes.to(dev, torch.int64), gt_classes.to(dev, torch.int64)

        order, det_offsets, gt_order, gt_offsets, bad = _coco_groups(scores, classes, gt_classes, K, max(self.max_dets))
        _, ranges = ops.coco_match_tables(dev)
        gt_ignore = (crowd[None, :] | (gt_area[None, :] < ranges[:, :1]) | (gt_area[None, :] > ranges[:, 1:])).to(torch.uint8)
        _, flag = ops.coco_match(iou, order, det_offsets, gt_order, gt_offsets, crowd.to(torch.uint8), gt_area.contiguous(),
                                 det_area.contiguous())
        order = order.long()
        self._pending.append((scores[order], classes[order], flag, gt_classes, gt_ignore, det_offsets[-1:], bad.reshape(1)))

    def _flush(self):
        """read back what `update` enqueued: one host record per image, cut to the detections inside the groups"""
        for ds, dc, flag, gc, gi, kept, bad in self._pending:
            if int(bad.cpu()[0]) != 0:
                raise ValueError(f"COCOAccumulator: {int(bad.cpu()[0])} classes outside 0 .. {self.num_classes - 1} in image "
                                 f"{len(self.records)}")
            k = int(kept.cpu()[0])
            self.records.append((ds[:k].cpu(), dc[:k].cpu(), flag[:, :, :k].cpu(), gc.cpu(), gi.cpu()))
        self._pending = []

    def reduce(self, group=None):
        """gather every rank's records (torch.distributed.all_gather_object; every rank ends with all of them, in rank order); a
        no-op in a process without a process group"""
        if not _distributed():
            return
        self._flush()
        self.records = [r for part in gather_objects(self.records, group) for r in part]

    def compute(self):
        """`coco_metrics` of everything added so far"""
        self._flush()
        return coco_metrics(self.records, self.num_classes, self.class_names, self.max_dets)


def coco_eval(detections, ground_truth, iou_type="bbox", num_classes=None, class_names=None, max_dets=(1, 10, 100), device=None):
    """COCO scores of a list of images in one call (see `COCOAccumulator`, which implements it).  detections: per image an `Instances`
    or (boxes or masks, scores, classes); ground_truth: per image (boxes or masks, classes), optionally followed by crowd flags and by
    areas.  num_classes defaults to len(class_names)."""
    if num_classes is None:
        if class_names is None:
            raise ValueError("coco_eval: num_classes or class_names is needed")
        num_classes = len(class_names)
    acc = COCOAccumulator(iou_type, num_classes, max_dets, device, class_names)
    for det, gt in zip(detections, ground_truth):
        g, gc, crowd, areas = optional_tail(gt, 4)
        if _is_instances(det):
            acc.update(det, gt=g, gt_classes=gc, gt_crowd=crowd, gt_areas=areas)
        else:
            acc.update(det[0], det[1], det[2], g, gc, crowd, areas)
    return acc.compute()
