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
"""
import numpy as np
import torch

from . import ops


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


def _default_device():
    return torch.device("cuda" if torch.cuda.is_available() else "cpu")


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


def _iou_matrix(a, b):
    """pairwise IoU of XYXY boxes a [n, 4], b [m, 4] (float64)"""
    a, b = a.double(), b.double()
    area_a = (a[:, 2] - a[:, 0]).clamp_min(0) * (a[:, 3] - a[:, 1]).clamp_min(0)
    area_b = (b[:, 2] - b[:, 0]).clamp_min(0) * (b[:, 3] - b[:, 1]).clamp_min(0)
    lt = torch.maximum(a[:, None, :2], b[None, :, :2])
    rb = torch.minimum(a[:, None, 2:], b[None, :, 2:])
    inter = (rb - lt).clamp_min(0).prod(-1)
    return inter / (area_a[:, None] + area_b[None, :] - inter).clamp_min(1e-300)


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
# Semantic and panoptic scores.  Both reduce to the joint histogram of two label maps, counted on the device by
# `ops.label_pair_hist` (csrc/labelhist.hip): the semantic confusion matrix is hist[pred class, gt class], the panoptic segment
# intersections are hist[gt segment, pred segment].  What follows the histogram is host arithmetic on small integer matrices.
# ------------------------------------------------------------------------------------------------------------------
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


def semantic_metrics(conf, class_names=None):
    """mIoU / fwIoU / mACC / pACC (and per-class IoU-<name> / ACC-<name>), all x 100, from a confusion matrix `conf` [N + 1, N + 1]
    indexed [pred, gt] whose last row and column hold the ignore bin -- the protocol of detectron2's SemSegEvaluator.evaluate that
    the reference's semantic configurations run, restated from its published definition: a class counts in the means iff it has
    ground-truth pixels (and, for the IoU, a non-empty union).  float64 on the host from the integer matrix.  detectron2 is not a
    dependency of this package: unpinned, like `box_ap`."""
    conf = torch.as_tensor(conf).detach().cpu()
    if conf.dim() != 2 or conf.shape[0] != conf.shape[1] or conf.shape[0] < 2:
        raise ValueError(f"semantic_metrics: conf must be [N + 1, N + 1], got {tuple(conf.shape)}")
    n = conf.shape[0] - 1
    if class_names is not None and len(class_names) != n:
        raise ValueError(f"semantic_metrics: {len(class_names)} class names for {n} classes")
    inner = conf[:-1, :-1].double()
    tp = inner.diagonal()
    pos_gt, pos_pred = inner.sum(0), inner.sum(1)
    acc_valid = pos_gt > 0
    union = pos_gt + pos_pred - tp
    iou_valid = acc_valid & (union > 0)
    nan = torch.full((n,), float("nan"), dtype=torch.float64)
    acc = torch.where(acc_valid, tp / pos_gt.clamp_min(1), nan)
    iou = torch.where(iou_valid, tp / union.clamp_min(1), nan)
    total = float(pos_gt.sum())
    weights = pos_gt / total if total > 0 else nan

    def mean(v, valid):
        return float(v[valid].sum() / valid.sum()) if bool(valid.any()) else float("nan")
    res = {"mIoU": 100 * mean(iou, iou_valid),
           "fwIoU": 100 * float((iou[iou_valid] * weights[iou_valid]).sum()) if bool(iou_valid.any()) else float("nan"),
           "mACC": 100 * mean(acc, acc_valid),
           "pACC": 100 * float(tp.sum()) / total if total > 0 else float("nan")}
    names = class_names if class_names is not None else [str(i) for i in range(n)]
    for i, name in enumerate(names):
        res[f"IoU-{name}"] = 100 * float(iou[i])
    for i, name in enumerate(names):
        res[f"ACC-{name}"] = 100 * float(acc[i])
    return res


def _label_map(t, device):
    """an integer label map on `device` (a host map is uploaded, as `encode_masks` does), flattened"""
    if t.device != device:
        t = t.to(device)
    return t.contiguous().reshape(-1)


class SemSegAccumulator:
    """The confusion matrix of a dataset, resident on the device: `update` is one `ops.label_pair_hist` launch per image and never
    synchronises with the host; `compute` reads the matrix once and hands it to `semantic_metrics` (detectron2's SemSegEvaluator,
    restated; unpinned).  Ground-truth pixels equal to `ignore_label` land in the last column, which no score reads."""

    def __init__(self, num_classes, ignore_label=255, device=None, class_names=None):
        self.num_classes = int(num_classes)
        self.ignore_label = None if ignore_label is None else int(ignore_label)
        if self.num_classes < 1:
            raise ValueError("SemSegAccumulator: num_classes must be at least 1")
        if self.ignore_label is not None and 0 <= self.ignore_label < self.num_classes:
            raise ValueError(f"SemSegAccumulator: ignore_label {self.ignore_label} is one of the {self.num_classes} classes")
        self.class_names = class_names
        self.device = None if device is None else torch.device(device)
        self.conf = self.rejected = None

    def _state(self, device):
        if self.conf is None:
            self.device = self.device if self.device is not None else device
            self.conf = torch.zeros((self.num_classes + 1, self.num_classes + 1), dtype=torch.int64, device=self.device)
            self.rejected = torch.zeros((1,), dtype=torch.int64, device=self.device)
        return self.device

    def update(self, pred_labels, gt_labels):
        """pred_labels: the semantic branch's int16 [H, W] label map (uint8 / int32 work too), or its [C, H, W] float32 scores, which
        `ops.argmax_labels` reduces; gt_labels: integer [H, W] (uint8 / int16 / int32), on the device or on the host"""
        dev = self._state(pred_labels.device)
        if pred_labels.device != dev:
            pred_labels = pred_labels.to(dev)
        if pred_labels.is_floating_point():
            if pred_labels.dim() != 3 or pred_labels.shape[0] != self.num_classes:
                raise ValueError(f"SemSegAccumulator.update: scores must be [{self.num_classes}, H, W], got {tuple(pred_labels.shape)}")
            pred_labels = ops.argmax_labels(pred_labels.float().contiguous())
        if tuple(pred_labels.shape) != tuple(gt_labels.shape):
            raise ValueError(f"SemSegAccumulator.update: prediction {tuple(pred_labels.shape)} vs ground truth {tuple(gt_labels.shape)}")
        ops.label_pair_hist(_label_map(pred_labels, dev), _label_map(gt_labels, dev), self.num_classes + 1, self.num_classes + 1,
                            b_ignore=self.ignore_label, out=self.conf, rejected=self.rejected)

    def reduce(self, group=None):
        """sum the matrix and the rejected counter over a torch.distributed group (every rank ends with the totals); a no-op in a
        process without one"""
        if not _distributed():
            return
        self._state(torch.device("cuda" if torch.cuda.is_available() else "cpu"))     # a rank without images adds zeros
        _all_reduce_sum(self.conf, group)
        _all_reduce_sum(self.rejected, group)

    def compute(self):
        if self.conf is None:
            raise RuntimeError("SemSegAccumulator.compute: no image was added")
        rejected = int(self.rejected.cpu()[0])
        if rejected != 0:
            raise ValueError(f"SemSegAccumulator: {rejected} pixels carried a label outside [0, {self.num_classes}] "
                             f"(ignore label {self.ignore_label}); the scores would silently leave them out")
        return semantic_metrics(self.conf.cpu(), self.class_names)


def panoptic_quality(per_class, isthing):
    """PQ / SQ / RQ (x 100) and the class count n for "All", "Things" and "Stuff" from per-class sums -- panopticapi's PQStat.pq_average
    (the scorer behind detectron2's COCOPanopticEvaluator, which the reference's panoptic configurations name), restated from its
    published definition; unpinned, like `box_ap`.
    per_class: {category_id: {"tp", "fp", "fn", "iou"}}, isthing: {category_id: bool}; a class counts iff tp + fp + fn > 0:
    PQ = iou / (tp + fp / 2 + fn / 2), SQ = iou / tp (0 without a match), RQ = tp / (tp + fp / 2 + fn / 2), averaged over classes."""
    res = {}
    for name, want in (("All", None), ("Things", True), ("Stuff", False)):
        pq = sq = rq = 0.0
        n = 0
        for cat, thing in isthing.items():
            if want is not None and bool(thing) != want:
                continue
            s = per_class.get(cat)
            if s is None:
                continue
            tp, fp, fn, iou = int(s["tp"]), int(s["fp"]), int(s["fn"]), float(s["iou"])
            if tp + fp + fn == 0:
                continue
            n += 1
            pq += iou / (tp + 0.5 * fp + 0.5 * fn)
            sq += iou / tp if tp != 0 else 0.0
            rq += tp / (tp + 0.5 * fp + 0.5 * fn)
        nan = float("nan")
        res[name] = {"PQ": 100 * pq / n if n else nan, "SQ": 100 * sq / n if n else nan, "RQ": 100 * rq / n if n else nan, "n": n}
    return res


class PanopticAccumulator:
    """Per-class tp / fp / fn / iou sums of a dataset.  Per image the segment intersections are ONE `ops.label_pair_hist` launch
    (hist[gt segment, pred segment]; the segment areas are its row and column sums) and one small read-back; the matching that
    follows is panopticapi's pq_compute_single_core, restated from its published definition (unpinned, like `box_ap`).
    categories: {category_id: isthing}, or panopticapi's list of {"id", "isthing"}."""

    VOID = 0

    def __init__(self, categories):
        if not isinstance(categories, dict):
            categories = {int(c["id"]): bool(c["isthing"]) for c in categories}
        self.isthing = {int(k): bool(v) for k, v in sorted(categories.items())}
        self._index = {c: i for i, c in enumerate(self.isthing)}
        n = len(self.isthing)
        self.tp, self.fp, self.fn = (torch.zeros(n, dtype=torch.int64) for _ in range(3))
        self.iou = torch.zeros(n, dtype=torch.float64)

    def _cat(self, cat, who):
        try:
            return self._index[int(cat)]
        except KeyError:
            raise KeyError(f"PanopticAccumulator: {who} segment has category {cat}, which is not one of the accumulator's categories")

    def update(self, pred_seg, pred_info, gt_seg, gt_info):
        """pred_seg: int32 [H, W], ids 0 .. count with 0 = void, pred_info: [{"id", "isthing", "category_id"}] (what `segments_info`
        returns); gt_seg: integer [H, W] with arbitrary ids (COCO packs RGB), 0 = VOID, on the device or the host,
        gt_info: [{"id", "category_id", "iscrowd"}]"""
        if pred_seg.dtype != torch.int32 or pred_seg.dim() != 2:
            raise TypeError(f"PanopticAccumulator.update: pred_seg must be int32 [H, W], got {pred_seg.dtype} {tuple(pred_seg.shape)}")
        if tuple(gt_seg.shape) != tuple(pred_seg.shape):
            raise ValueError(f"PanopticAccumulator.update: prediction {tuple(pred_seg.shape)} vs ground truth {tuple(gt_seg.shape)}")
        if gt_seg.is_floating_point() or gt_seg.dtype == torch.bool:
            raise TypeError(f"PanopticAccumulator.update: gt_seg must be an integer map, got {gt_seg.dtype}")
        dev = pred_seg.device
        gt_ids = [int(g["id"]) for g in gt_info]
        pred_ids = [int(p["id"]) for p in pred_info]
        if len(set(gt_ids)) != len(gt_ids) or len(set(pred_ids)) != len(pred_ids) or self.VOID in gt_ids or any(i <= 0 for i in pred_ids):
            raise ValueError("PanopticAccumulator.update: segment ids must be unique and positive (0 is VOID)")
        G, P = len(gt_ids), max(pred_ids, default=0)
        # compact the ground truth's ids to 0 .. G (0 = VOID, then gt_info's order); an id the table does not know becomes G + 1, which
        # the histogram rejects
        table = torch.tensor([self.VOID] + gt_ids, dtype=torch.int64)
        order = torch.argsort(table)
        keys, rank = table[order].to(dev), order.to(dev)
        flat = _label_map(gt_seg, dev).long()
        pos = torch.searchsorted(keys, flat).clamp_max(G)
        compact = torch.where(keys[pos] == flat, rank[pos], torch.full_like(pos, G + 1)).to(torch.int32)
        hist, rejected = ops.label_pair_hist(compact, _label_map(pred_seg, dev), G + 1, P + 1)
        inter = hist.cpu()
        if int(rejected.cpu()[0]) != 0:
            known = torch.tensor([self.VOID] + gt_ids, dtype=torch.int64)
            seen = torch.unique(flat.cpu())
            unknown = seen[~torch.isin(seen, known)].tolist()
            if unknown:
                raise KeyError(f"PanopticAccumulator.update: the ground-truth map holds ids {unknown[:8]} that gt_info does not list")
            raise KeyError(f"PanopticAccumulator.update: pred_seg holds ids outside 0 .. {P}, the largest id of pred_info")
        area_gt, area_pred = inter.sum(1), inter.sum(0)
        listed = torch.zeros(P + 1, dtype=torch.bool)
        listed[self.VOID] = True
        listed[torch.tensor(pred_ids, dtype=torch.int64)] = True
        if bool((area_pred[~listed] != 0).any()):
            raise KeyError(f"PanopticAccumulator.update: pred_seg holds ids {(~listed & (area_pred != 0)).nonzero().flatten().tolist()[:8]} "
                           "that pred_info does not list")
        for p in pred_info:
            if int(area_pred[int(p["id"])]) == 0:
                raise KeyError(f"PanopticAccumulator.update: predicted segment {p['id']} has no pixel in pred_seg")
        pred_cat = {int(p["id"]): self._cat(p["category_id"], "a predicted") for p in pred_info}
        gt_cat = [self._cat(g["category_id"], "a ground-truth") for g in gt_info]
        crowd = [int(g.get("iscrowd", 0)) == 1 for g in gt_info]
        gt_matched, pred_matched = set(), set()
        for gi in range(G):
            if crowd[gi]:
                continue
            row = inter[gi + 1]
            for pid in row.nonzero().flatten().tolist():
                if pid == self.VOID or pred_cat[pid] != gt_cat[gi]:
                    continue
                i = int(row[pid])
                union = int(area_pred[pid]) + int(area_gt[gi + 1]) - i - int(inter[self.VOID, pid])
                iou = i / union
                if iou > 0.5:
                    self.tp[gt_cat[gi]] += 1
                    self.iou[gt_cat[gi]] += iou
                    gt_matched.add(gi)
                    pred_matched.add(pid)
        crowd_of = {}                          # category -> its crowd segment (the last one listed, as panopticapi's dict keeps)
        for gi in range(G):
            if gi in gt_matched:
                continue
            if crowd[gi]:
                crowd_of[gt_cat[gi]] = gi
                continue
            self.fn[gt_cat[gi]] += 1
        for pid, cat in pred_cat.items():
            if pid in pred_matched:
                continue
            covered = int(inter[self.VOID, pid])
            if cat in crowd_of:
                covered += int(inter[crowd_of[cat] + 1, pid])
            if covered / int(area_pred[pid]) > 0.5:
                continue
            self.fp[cat] += 1

    def reduce(self, group=None):
        """sum the per-class tp / fp / fn / iou arrays over a torch.distributed group; a no-op in a process without one"""
        if not _distributed():
            return
        import torch.distributed as dist
        dev = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
        for name in ("tp", "fp", "fn", "iou"):
            t = getattr(self, name).to(dev)
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
            setattr(self, name, t.cpu())

    def per_class(self):
        return {c: {"tp": int(self.tp[i]), "fp": int(self.fp[i]), "fn": int(self.fn[i]), "iou": float(self.iou[i])} for c, i in self._index.items()}

    def compute(self):
        """{"All" | "Things" | "Stuff": {"PQ", "SQ", "RQ" (x 100), "n"}} over the classes with tp + fp + fn > 0"""
        return panoptic_quality(self.per_class(), self.isthing)


# ------------------------------------------------------------------------------------------------------------------
# Instance masks.  The IoU matrix of an image's detections against its ground truth is counted on the device by
# `ops.mask_pair_iou` (csrc/maskiou.hip: one bit pack per side, one popcount contraction); only the [n, m] matrix travels.
# The protocol that follows is `_coco_ap`, the same code `box_ap` runs.
# ------------------------------------------------------------------------------------------------------------------
def _device_masks(masks, device=None):
    """[n, H, W] masks on the device from a device tensor, a host tensor (uploaded) or a list of RLE dicts (decoded); None for an
    empty list, which has no size"""
    if isinstance(masks, (list, tuple)):
        return decode_masks(masks, device) if len(masks) > 0 else None
    if masks.dim() != 3:
        raise ValueError(f"masks must be [n, H, W], got {tuple(masks.shape)}")
    if not masks.is_cuda:
        masks = masks.to(_default_device() if device is None else device)
    return masks.contiguous()


class MaskAPAccumulator:
    """COCO-style mask AP of a dataset: the protocol `box_ap` documents, with mask IoU in place of box IoU.  `update` packs each side
    of an image once, counts the whole n x m intersection matrix in one launch (`ops.mask_pair_iou`) and keeps only the image's small
    host record -- scores, classes and the IoU matrix; the per-class greedy matching stays on the host, in `compute`.
    Out of scope, as for `box_ap`: crowd regions, area ranges (APs / APm / APl), polygon ground truth (there is no rasteriser here)
    and the LVIS federated protocol.  pycocotools is not a dependency of this package: unpinned."""

    def __init__(self, iou_thresholds=None, max_dets=100, device=None):
        self.iou_thresholds = None if iou_thresholds is None else [float(t) for t in iou_thresholds]
        self.max_dets = int(max_dets)
        self.device = None if device is None else torch.device(device)
        self.records = []

    def update(self, pred, scores=None, classes=None, gt_masks=None, gt_classes=None):
        """pred: masks [n, H, W] (uint8 / bool; device tensor, host tensor or list of RLE dicts) with `scores` [n] and `classes` [n],
        or an `Instances` carrying `pred_masks` or `pred_masks_rle` next to `scores` and `pred_classes`;
        gt_masks: [m, H, W] in any of the three forms, gt_classes [m]"""
        if hasattr(pred, "has") and hasattr(pred, "get_fields"):
            inst = pred
            if inst.has("pred_masks"):
                pred = inst.pred_masks
            elif inst.has("pred_masks_rle"):
                pred = list(inst.pred_masks_rle)
            else:
                raise ValueError("MaskAPAccumulator.update: the instances carry neither pred_masks nor pred_masks_rle")
            scores = inst.scores if scores is None else scores
            classes = inst.pred_classes if classes is None else classes
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
            b = _device_masks(gt_masks, a.device)
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
        if not _distributed():
            return
        import torch.distributed as dist
        parts = [None] * dist.get_world_size(group)
        dist.all_gather_object(parts, self.records, group=group)
        self.records = [r for part in parts for r in part]

    def compute(self):
        """dict(AP, AP50, AP75, classes, gt, dets), the keys of `box_ap`"""
        return _coco_ap(self.records, self.iou_thresholds, self.max_dets)


def mask_ap(detections, ground_truth, iou_thresholds=None, max_dets=100):
    """COCO-style mask AP (see `MaskAPAccumulator`, which implements it; the protocol is `box_ap`'s).
    detections: list (one entry per image) of (masks, scores [n], classes [n]); ground_truth: list of (masks, classes [m]); masks is a
    [n, H, W] uint8 / bool tensor on the device, a host tensor (uploaded) or a list of RLE dicts (decoded on the device).
    -> dict(AP, AP50, AP75, classes, gt, dets)."""
    acc = MaskAPAccumulator(iou_thresholds, max_dets)
    for (dm, ds, dc), (gm, gc) in zip(detections, ground_truth):
        acc.update(dm, ds, dc, gm, gc)
    return acc.compute()


# ------------------------------------------------------------------------------------------------------------------
# Mask boundaries.  Boundary IoU (Cheng et al., CVPR 2021) is the IoU of the two masks' inner boundary bands, d = 2 % of the image
# diagonal wide; Boundary AP matches on min(mask IoU, boundary IoU).  The bands are made on the device from row-packed bits
# (`ops.boundary_pair_iou`, csrc/boundary.hip) and contracted by the same popcount kernel as the masks; only the [n, m] matrix travels.
# ------------------------------------------------------------------------------------------------------------------
def boundary_iou(a, b, dilation_ratio=0.02, dilation=None, device=None):
    """Boundary IoU matrix of two mask sets of one size, float64 [n, m] on the device: the IoU of the inner boundary bands, each
    `dilation` pixels wide (default: `dilation_ratio` of the image diagonal, `ops.boundary_dilation`), 0 where both bands are empty.
    The published `boundary_iou` package restated (not installable here: unpinned, like `box_ap`).  a, b: [n, H, W] uint8 / bool on
    the device, host tensors (uploaded) or lists of RLE dicts (decoded on the device)."""
    a = _device_masks(a, device)
    if a is None:
        raise ValueError("boundary_iou: an empty list has no size; build the [0, h, w] tensor yourself")
    b = _device_masks(b, a.device)
    if b is None:
        raise ValueError("boundary_iou: an empty list has no size; build the [0, h, w] tensor yourself")
    return ops.boundary_pair_iou(a, b, dilation_ratio, dilation)[0]


class BoundaryAPAccumulator(MaskAPAccumulator):
    """COCO-style Boundary AP of a dataset (the second segmentation metric of the LVIS challenge): `MaskAPAccumulator` with the matching
    IoU min(mask IoU, boundary IoU), both counted on the device in `ops.boundary_pair_iou` -- one row pack and one erosion per side,
    two popcount contractions.  Inputs, `update` / `reduce` / `compute` and the result keys are `MaskAPAccumulator`'s.
    Out of scope, like its siblings: crowd regions, area ranges (APs / APm / APl), polygon ground truth, the LVIS federated protocol
    and boundary PQ.  The `boundary_iou` package is not a dependency of this package: unpinned."""

    def __init__(self, iou_thresholds=None, max_dets=100, device=None, dilation_ratio=0.02):
        super().__init__(iou_thresholds, max_dets, device)
        self.dilation_ratio = float(dilation_ratio)

    def _pair_iou(self, a, b):
        biou, iou = ops.boundary_pair_iou(a, b, self.dilation_ratio)[:2]
        return torch.minimum(iou, biou).cpu()


def boundary_ap(detections, ground_truth, iou_thresholds=None, max_dets=100, dilation_ratio=0.02):
    """COCO-style Boundary AP (see `BoundaryAPAccumulator`, which implements it): `mask_ap` with min(mask IoU, boundary IoU) as the
    matching IoU.  detections / ground_truth as for `mask_ap`.  -> dict(AP, AP50, AP75, classes, gt, dets)."""
    acc = BoundaryAPAccumulator(iou_thresholds, max_dets, dilation_ratio=dilation_ratio)
    for (dm, ds, dc), (gm, gc) in zip(detections, ground_truth):
        acc.update(dm, ds, dc, gm, gc)
    return acc.compute()


# ------------------------------------------------------------------------------------------------------------------
# Referring expressions (RefCOCO / RefCOCO+ / RefCOCOg; ape/evaluation/refcoco_evaluation.py:377-421, refcocoeval.py:17-39,201-250).
# Expression mode returns ONE detection per expression, so the scores are PAIRED: sample i needs |pred_i & gt_i|, |pred_i| and |gt_i|,
# which `ops.mask_paired_counts` (csrc/maskiou.hip) counts in one pass over the two byte masks, straight into a row of a device table.
# ------------------------------------------------------------------------------------------------------------------
_REFER_THRESHOLDS = (5, 6, 7, 8, 9)                       # tenths: P@0.5 .. P@0.9


def referring_metrics(counts, boxes=None):
    """The referring-expression scores of N samples, all x 100, from counts int64 [N, 3] = (inter, area_pred, area_gt) per sample (what
    `ops.mask_paired_counts` returns) and, optionally, boxes float64 [N, 8] = prediction XYXY followed by ground-truth XYXY.  A pure host
    function.  The reference's keys with the reference's meanings:
      oIoU   sum(inter) / sum(union), union = area_pred + area_gt - inter: integer sums, ONE float64 division; 0.0 if no union at all;
      mIoU   the float64 mean of the per-sample IoUs, each with the reference's arithmetic (refcocoeval.py:36-38 as torch evaluates it,
             in float32): (inter.float() + 1e-6) / (union.float() + 1e-6).  Empty against empty scores 1 (the reference's convention).
             The counts convert to float32 exactly up to 2^24 pixels per mask (4096 x 4096); beyond that the reference's own float32
             sums round as well, in their own way;
      P@0.5 .. P@0.9 (only with `boxes`)  the share of samples whose BOX IoU exceeds the threshold (strictly), box IoU in float64 as
             inter / (area_p + area_g - inter), 0 for an empty union -- the pycocotools formula behind the reference's `coco_eval.ious`;
             pycocotools is not a dependency of this package: unpinned, like `box_ap`.
    And extras:
      mask_P@0.5 .. mask_P@0.9  the share of samples whose MASK IoU exceeds the threshold, in exact integers (10 inter > k union); an
             empty union counts as a hit, in line with its IoU of 1;
      samples  N."""
    counts = torch.as_tensor(counts).detach().cpu()
    if counts.dim() != 2 or counts.shape[1] != 3 or counts.is_floating_point() or counts.dtype == torch.bool:
        raise ValueError(f"referring_metrics: counts must be an integer [N, 3], got {counts.dtype} {tuple(counts.shape)}")
    N = int(counts.shape[0])
    if N == 0:
        raise ValueError("referring_metrics: no samples")
    counts = counts.long()
    inter, union = counts[:, 0], counts[:, 1] + counts[:, 2] - counts[:, 0]
    if bool((counts < 0).any()) or bool((inter > torch.minimum(counts[:, 1], counts[:, 2])).any()):
        raise ValueError("referring_metrics: counts are (inter, area_pred, area_gt) with 0 <= inter <= either area")
    total_union = int(union.sum())
    iou32 = (inter.float() + 1e-6) / (union.float() + 1e-6)
    res = {"oIoU": 100.0 * int(inter.sum()) / total_union if total_union > 0 else 0.0,
           "mIoU": 100.0 * float(iou32.double().mean())}
    if boxes is not None:
        boxes = torch.as_tensor(boxes).detach().cpu().double()
        if tuple(boxes.shape) != (N, 8):
            raise ValueError(f"referring_metrics: boxes must be [{N}, 8] (prediction XYXY, ground-truth XYXY), got {tuple(boxes.shape)}")
        p, g = boxes[:, :4], boxes[:, 4:]
        wh = (torch.minimum(p[:, 2:], g[:, 2:]) - torch.maximum(p[:, :2], g[:, :2])).clamp_min(0)
        binter = wh[:, 0] * wh[:, 1]
        bunion = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]) + (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]) - binter
        biou = torch.where(bunion > 0, binter / torch.where(bunion > 0, bunion, torch.ones_like(bunion)), torch.zeros_like(bunion))
        for k in _REFER_THRESHOLDS:
            res[f"P@0.{k}"] = 100.0 * int((biou > k / 10).sum()) / N
    for k in _REFER_THRESHOLDS:
        res[f"mask_P@0.{k}"] = 100.0 * int((10 * inter > k * union).sum() + (union == 0).sum()) / N
    res["samples"] = N
    return res


def _is_instances(x):
    return hasattr(x, "has") and hasattr(x, "get_fields")


class ReferringAccumulator:
    """The referring-expression scores of a dataset (`referring_metrics`: oIoU, mIoU, P@k, mask_P@k).  The state is a device table,
    int64 [capacity, 3] with a float64 [capacity, 8] companion for the boxes: `update` has `ops.mask_paired_counts` write the sample's
    row directly (`out=` a one-row view) and, when the masks are on the device already, issues no device-to-host copy and no
    synchronisation; the tables grow by doubling with a device-to-device copy, and `compute` reads them back once.
    Out of scope: the COCO-style AP the reference also prints for these datasets (that is `box_ap` / `mask_ap`), gRefCOCO's N-acc / T-acc,
    polygon ground truth."""

    def __init__(self, device=None, capacity=256):
        self.device = None if device is None else torch.device(device)
        self.capacity = max(1, int(capacity))
        self.counts = self.boxes = None
        self.n = 0
        self.with_boxes = None                            # decided by the first sample

    def _row(self, device):
        """the index of the next sample's row, after making room for it"""
        if self.counts is None:
            self.device = self.device if self.device is not None else device
            self.counts = torch.zeros((self.capacity, 3), dtype=torch.int64, device=self.device)
            self.boxes = torch.zeros((self.capacity, 8), dtype=torch.float64, device=self.device)
        elif self.n == self.capacity:
            self.capacity *= 2
            for name in ("counts", "boxes"):
                old = getattr(self, name)
                new = torch.zeros((self.capacity, old.shape[1]), dtype=old.dtype, device=old.device)
                new[: self.n].copy_(old[: self.n])
                setattr(self, name, new)
        return self.n

    @staticmethod
    def _one_mask(mask, device, who):
        """[1, H, W] on the device from a [H, W] / [1, H, W] tensor (device or host) or one RLE dict"""
        if isinstance(mask, dict):
            return _device_masks([mask], device)
        if mask.dim() == 2:
            mask = mask[None]
        if mask.dim() != 3 or mask.shape[0] != 1:
            raise ValueError(f"ReferringAccumulator.update: {who} must be one mask, [H, W] or [1, H, W], got {tuple(mask.shape)}")
        return _device_masks(mask, device)

    def update(self, pred=None, gt_mask=None, gt_box=None, pred_mask=None, pred_box=None):
        """One sample.  The prediction is either `pred`, an `Instances` as expression mode returns it (`pred_masks` or `pred_masks_rle`,
        `pred_boxes`, `scores`; the highest-scoring instance is taken, on a tie the first, as the reference's stable sort does), or
        `pred_mask` ([H, W] / [1, H, W] uint8 / bool on the device or the host, or one RLE dict) with an optional `pred_box` (XYXY).
        Neither, or an `Instances` of length 0, is a sample without prediction: it scores as an empty mask, (0, 0, area_gt), and is a
        box miss.  gt_mask: a device tensor, a host tensor or one RLE dict; gt_box: optional XYXY -- with it the sample takes part in
        P@k, and then every sample of the dataset must."""
        if gt_mask is None:
            raise ValueError("ReferringAccumulator.update: gt_mask is needed")
        if pred is not None and pred_mask is not None:
            raise ValueError("ReferringAccumulator.update: give the prediction as `pred` or as `pred_mask`, not both")
        if pred is not None and not _is_instances(pred):
            raise TypeError("ReferringAccumulator.update: `pred` is an Instances; a bare mask goes in as `pred_mask`")
        with_boxes = gt_box is not None
        if self.with_boxes is not None and with_boxes != self.with_boxes:
            raise ValueError("ReferringAccumulator.update: some samples have boxes and some do not; P@k needs a box for every sample")
        if pred is not None and len(pred) > 0:
            masks = pred.pred_masks if pred.has("pred_masks") else None
            if masks is None and not pred.has("pred_masks_rle"):
                raise ValueError("ReferringAccumulator.update: the instances carry neither pred_masks nor pred_masks_rle")
            pb = pred.pred_boxes.tensor if with_boxes else None
            scores = torch.as_tensor(pred.scores).reshape(-1)
            if len(pred) == 1:
                first = slice(0, 1)
            else:
                order = torch.argsort(scores, descending=True, stable=True)[:1]
                if scores.is_cuda and masks is not None and masks.device == scores.device and (pb is None or pb.device == scores.device):
                    first = order                                 # everything is on the device: the choice stays there, no read-back
                else:
                    first = slice(int(order), int(order) + 1)
            pred_mask = masks[first] if masks is not None else pred.pred_masks_rle[first.start]
            pred_box = pb[first] if with_boxes else None
        on_device = [m.device for m in (gt_mask, pred_mask) if torch.is_tensor(m) and m.is_cuda]
        dev = self.device if self.device is not None else (on_device[0] if on_device else _default_device())
        gt = self._one_mask(gt_mask, dev, "gt_mask").to(dev)
        if pred_mask is None:
            pm = torch.zeros_like(gt)                             # no prediction: the empty mask, (0, 0, area_gt)
        else:
            pm = self._one_mask(pred_mask, dev, "the predicted mask").to(dev)
            if with_boxes and pred_box is None:
                raise ValueError("ReferringAccumulator.update: gt_box without a box for the prediction")
        if tuple(pm.shape) != tuple(gt.shape):
            raise ValueError(f"ReferringAccumulator.update: prediction {tuple(pm.shape[1:])} vs ground truth {tuple(gt.shape[1:])}")
        i = self._row(dev)
        ops.mask_paired_counts(pm, gt, out=self.counts[i: i + 1])
        if with_boxes:
            self._put_box(i, 4, gt_box)
            if pred_mask is None:
                self.boxes[i, :4].zero_()                         # an empty box: IoU 0, a miss at every threshold
            else:
                self._put_box(i, 0, pred_box)
        self.with_boxes = with_boxes
        self.n += 1

    def _put_box(self, i, col, box):
        """box (XYXY; tensor, list or tuple) -> self.boxes[i, col: col + 4].  A device box is copied on the device; a host box travels as
        four scalar launch arguments, not as a host-to-device copy, which would wait for the stream"""
        if torch.is_tensor(box) and box.is_cuda:
            self.boxes[i, col: col + 4].copy_(box.detach().reshape(4))
            return
        values = [float(v) for v in (box.reshape(-1).tolist() if torch.is_tensor(box) else box)]
        if len(values) != 4:
            raise ValueError(f"ReferringAccumulator.update: a box is XYXY, got {len(values)} values")
        for j, v in enumerate(values):
            self.boxes[i, col + j].fill_(v)

    def _host_rows(self):
        if self.n == 0:
            return torch.zeros((0, 3), dtype=torch.int64), None
        return self.counts[: self.n].cpu(), (self.boxes[: self.n].cpu() if self.with_boxes else None)

    def reduce(self, group=None):
        """gather every rank's rows (torch.distributed.all_gather_object of the host copies; every rank ends with all of them, in rank
        order); a no-op in a process without a process group"""
        if not _distributed():
            return
        import torch.distributed as dist
        parts = [None] * dist.get_world_size(group)
        dist.all_gather_object(parts, self._host_rows(), group=group)
        parts = [p for p in parts if p[0].shape[0] > 0]
        if not parts:
            return
        if len({p[1] is None for p in parts}) != 1:
            raise ValueError("ReferringAccumulator.reduce: some ranks have boxes and some do not")
        counts = torch.cat([p[0] for p in parts])
        self.with_boxes = parts[0][1] is not None
        dev = self.device if self.device is not None else _default_device()
        self.n = 0
        self.counts = None
        self.capacity = max(self.capacity, int(counts.shape[0]))
        self._row(dev)
        self.counts[: counts.shape[0]] = counts.to(self.device)
        if self.with_boxes:
            self.boxes[: counts.shape[0]] = torch.cat([p[1] for p in parts]).to(self.device)
        self.n = int(counts.shape[0])

    def compute(self):
        """`referring_metrics` of the samples: oIoU, mIoU, mask_P@k, samples, and P@k if the samples came with boxes"""
        if self.n == 0:
            raise RuntimeError("ReferringAccumulator.compute: no sample was added")
        return referring_metrics(*self._host_rows())


def referring_scores(samples, device=None):
    """The referring-expression scores of a list in one call (see `ReferringAccumulator`, which implements it, and `referring_metrics`
    for the keys).  samples: a list of (pred, gt_mask) or (pred, gt_mask, gt_box); pred is an `Instances`, None (no prediction), one
    mask (tensor or RLE dict) or (mask, box); gt_mask a device tensor, a host tensor or an RLE dict; boxes XYXY."""
    acc = ReferringAccumulator(device)
    for s in samples:
        pred, gt_mask, gt_box = (tuple(s) + (None,))[:3]
        if pred is None or _is_instances(pred):
            acc.update(pred, gt_mask, gt_box)
        elif isinstance(pred, (tuple, list)):
            acc.update(None, gt_mask, gt_box, pred_mask=pred[0], pred_box=pred[1])
        else:
            acc.update(None, gt_mask, gt_box, pred_mask=pred)
    return acc.compute()


# ------------------------------------------------------------------------------------------------------------------
# Box proposals (ape/evaluation/lvis_evaluation.py:293-399, the same function in refcoco_evaluation.py and d3_evaluation.py; reported by
# `_eval_box_proposals` as AR@100 .. ARl@1000).  Recall of the class-agnostic boxes: how a two-stage detector's proposal selection is
# judged apart from its classification.  The greedy coverage loop runs on the device (`ops.box_cover_overlaps`, csrc/boxcover.hip), all
# eight (area range, limit) combinations of an image in one launch; what is kept per dataset is two small integer tables.
# ------------------------------------------------------------------------------------------------------------------
_PROPOSAL_AREAS = ("", "s", "m", "l")                     # all, small, medium, large: the order of ops.BOX_COVER_RANGES


def proposal_recall_thresholds():
    """the reference's IoU thresholds 0.5, 0.55 .. 0.95 as the float32 values its `torch.arange` gives"""
    return torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)


def proposal_recall_names(limits=(100, 1000)):
    """AR@100, ARs@100, ARm@100, ARl@100, AR@1000, ... : the rows of the tables, limit outer, area inner"""
    return [f"AR{a}@{int(k)}" for k in limits for a in _PROPOSAL_AREAS]


def proposal_recall_metrics(counts, num_pos, names=None, images=None, thresholds=None):
    """Box-proposal recall from its tables.  A pure host function.
    counts int64 [C, T]: per (area range, limit) combination and IoU threshold, the in-range ground-truth boxes whose recorded overlap
    is at or above the threshold; num_pos int64 [C]: the in-range ground-truth boxes; names: the C keys (default
    `proposal_recall_names()`, C = 8).  The reference's arithmetic (lvis_evaluation.py:387-392): recalls[t] = float32(counts[c, t]) /
    float(num_pos[c]) -- a float32 tensor divided by a Python float --, ar = recalls.mean() in float32, and the reported value is
    float(ar.item() * 100); num_pos == 0 gives nan, as there.  Tables of two parts of a dataset merge by addition.
    Returns the C keys plus `gt` = num_pos[0] (with the default names: the ground-truth boxes of all areas) and, when given, `images`
    (an int the tables do not hold) and `thresholds` (the T IoU thresholds, listed as floats)."""
    counts, num_pos = torch.as_tensor(counts).detach().cpu(), torch.as_tensor(num_pos).detach().cpu()
    for t, name in ((counts, "counts"), (num_pos, "num_pos")):
        if t.is_floating_point() or t.dtype == torch.bool:
            raise ValueError(f"proposal_recall_metrics: {name} must be an integer tensor, got {t.dtype}")
    if counts.dim() != 2 or counts.shape[1] == 0 or tuple(num_pos.shape) != (counts.shape[0],):
        raise ValueError(f"proposal_recall_metrics: counts must be [C, T] and num_pos [C], got {tuple(counts.shape)} and {tuple(num_pos.shape)}")
    names = proposal_recall_names() if names is None else list(names)
    if len(names) != counts.shape[0]:
        raise ValueError(f"proposal_recall_metrics: {len(names)} names for {counts.shape[0]} rows")
    counts, num_pos = counts.long(), num_pos.long()
    if bool((counts < 0).any()) or bool((counts > num_pos[:, None]).any()):
        raise ValueError("proposal_recall_metrics: 0 <= counts[c, t] <= num_pos[c]")
    res = {}
    for c, name in enumerate(names):
        recalls = counts[c].float() / float(int(num_pos[c]))      # x / 0.0 is nan or inf in torch, never an exception
        res[name] = float(recalls.mean().item() * 100)
    res["gt"] = int(num_pos[0])
    if images is not None:
        res["images"] = int(images)
    if thresholds is not None:
        thresholds = torch.as_tensor(thresholds, dtype=torch.float32).reshape(-1)
        if thresholds.numel() != counts.shape[1]:
            raise ValueError(f"proposal_recall_metrics: {thresholds.numel()} thresholds for {counts.shape[1]} columns")
        res["thresholds"] = thresholds.tolist()
    return res


class ProposalRecallAccumulator:
    """Box-proposal recall of a dataset: AR@100, ARs@100, ARm@100, ARl@100, AR@1000, ... (`proposal_recall_metrics`) plus `images`, `gt`
    (the ground-truth boxes of the first row, i.e. of all areas) and `thresholds`.  The state is two device tables, counts int64 [C, T]
    and num_pos int64 [C]; `update` sorts the proposals on the device, runs `ops.box_cover_overlaps` (one launch for all C combinations)
    and adds to the tables with tensor ops: with device inputs it never synchronises.  `compute` reads the tables back once.
    gt_areas: COCO and LVIS score with the annotations' `area` field, the SEGMENT's area, not the box area; pass it when there is one
    (the default is the box area, right for box-only ground truth).
    Order among equal scores: the reference sorts with an unstable sort, which leaves it unspecified; here the sort is stable --
    proposals of equal score keep their input order."""

    def __init__(self, device=None, limits=(100, 1000), thresholds=None):
        self.device = None if device is None else torch.device(device)
        self.limits = tuple(int(k) for k in limits)
        self.names = proposal_recall_names(self.limits)
        thr = proposal_recall_thresholds() if thresholds is None else torch.as_tensor(thresholds, dtype=torch.float32).reshape(-1).cpu()
        if thr.numel() == 0:
            raise ValueError("ProposalRecallAccumulator: no thresholds")
        self.thresholds = thr
        self.counts = self.num_pos = self._thr = None
        self.images = 0

    def _state(self, device):
        if self.counts is None:
            self.device = self.device if self.device is not None else device
            C = len(self.names)
            self.counts = torch.zeros((C, self.thresholds.numel()), dtype=torch.int64, device=self.device)
            self.num_pos = torch.zeros((C,), dtype=torch.int64, device=self.device)
            self._thr = self.thresholds.to(self.device)
        return self.device

    def update(self, proposals, gt_boxes, gt_areas=None, boxes=None, logits=None):
        """One image.  proposals: an `Instances` with `proposal_boxes` + `objectness_logits` (a proposal generator's output) or with
        `pred_boxes` + `scores` (a detector's), or None with `boxes` [n, 4] XYXY and `logits` [n] as tensors; gt_boxes [m, 4] XYXY (a
        tensor or a `Boxes`); gt_areas [m] optional (see the class).  Host inputs are uploaded.  The proposals are put in descending
        score order by a stable sort.  An image without proposals or without ground truth adds nothing to the tables (the reference's
        rule, lvis_evaluation.py:343-344, decided from the shapes alone) but counts in `images`."""
        who = "ProposalRecallAccumulator.update"
        if proposals is not None:
            if boxes is not None or logits is not None:
                raise ValueError(f"{who}: give the proposals as an Instances or as boxes= / logits=, not both")
            if not _is_instances(proposals):
                raise TypeError(f"{who}: `proposals` is an Instances; bare tensors go in as boxes= and logits=")
            if proposals.has("proposal_boxes") and proposals.has("objectness_logits"):
                boxes, logits = proposals.proposal_boxes, proposals.objectness_logits
            elif proposals.has("pred_boxes") and proposals.has("scores"):
                boxes, logits = proposals.pred_boxes, proposals.scores
            else:
                raise ValueError(f"{who}: the instances carry neither proposal_boxes + objectness_logits nor pred_boxes + scores")
        if boxes is None or logits is None:
            raise ValueError(f"{who}: boxes and logits are both needed")
        boxes, gt_boxes = getattr(boxes, "tensor", boxes), getattr(gt_boxes, "tensor", gt_boxes)
        boxes, logits, gt_boxes = torch.as_tensor(boxes), torch.as_tensor(logits), torch.as_tensor(gt_boxes)
        if boxes.dim() != 2 or boxes.shape[1] != 4 or tuple(logits.shape) != (boxes.shape[0],):
            raise ValueError(f"{who}: boxes must be [n, 4] and logits [n], got {tuple(boxes.shape)} and {tuple(logits.shape)}")
        if gt_boxes.dim() != 2 or gt_boxes.shape[1] != 4:
            raise ValueError(f"{who}: gt_boxes must be [m, 4], got {tuple(gt_boxes.shape)}")
        n, m = boxes.shape[0], gt_boxes.shape[0]
        if gt_areas is not None:
            gt_areas = torch.as_tensor(gt_areas)
            if tuple(gt_areas.shape) != (m,):
                raise ValueError(f"{who}: gt_areas must be [{m}], got {tuple(gt_areas.shape)}")
        on_device = [t.device for t in (boxes, gt_boxes, logits) if t.is_cuda]
        dev = self._state(on_device[0] if on_device else _default_device())
        self.images += 1
        if n == 0 or m == 0:
            return
        boxes, logits = boxes.detach().to(dev, torch.float32), logits.detach().to(dev)
        gt_boxes = gt_boxes.detach().to(dev, torch.float32).contiguous()
        if gt_areas is not None:
            gt_areas = gt_areas.detach().to(dev, torch.float32).contiguous()
        order = torch.sort(logits, descending=True, stable=True)[1]
        ov, _ = ops.box_cover_overlaps(boxes[order], gt_boxes, gt_areas, limits=self.limits)
        self.counts += (ov[:, :, None] >= self._thr).sum(1)
        self.num_pos += (ov >= 0).sum(1)

    def reduce(self, group=None):
        """sum both tables (and the image count) over a torch.distributed group: every rank ends with the totals; a no-op in a process
        without one"""
        if not _distributed():
            return
        self._state(_default_device())                            # a rank without images adds zeros
        _all_reduce_sum(self.counts, group)
        _all_reduce_sum(self.num_pos, group)
        images = torch.tensor([self.images], dtype=torch.int64, device=self.device)
        _all_reduce_sum(images, group)
        self.images = int(images.cpu()[0])

    def compute(self):
        if self.counts is None:
            raise RuntimeError("ProposalRecallAccumulator.compute: no image was added")
        both = torch.cat([self.counts, self.num_pos[:, None]], 1).cpu()       # one read-back
        return proposal_recall_metrics(both[:, :-1], both[:, -1], self.names, images=self.images, thresholds=self.thresholds)


def proposal_recall(samples, device=None, **kw):
    """Box-proposal recall of a list in one call (see `ProposalRecallAccumulator`, which implements it).  samples: a list of
    (proposals, gt_boxes) or (proposals, gt_boxes, gt_areas); proposals is an `Instances` or a (boxes, logits) pair of tensors;
    keywords go to the accumulator (limits, thresholds)."""
    acc = ProposalRecallAccumulator(device, **kw)
    for s in samples:
        proposals, gt_boxes, gt_areas = (tuple(s) + (None,))[:3]
        if _is_instances(proposals):
            acc.update(proposals, gt_boxes, gt_areas)
        else:
            acc.update(None, gt_boxes, gt_areas, boxes=proposals[0], logits=proposals[1])
    return acc.compute()


# ------------------------------------------------------------------------------------------------------------------
# COCO's full detection protocol (pycocotools' COCOeval, what the reference's instance_evaluation.py / d3_evaluation.py and detectron2's
# COCOEvaluator run): crowd regions, the four area ranges, AP / AP50 / AP75 / APs / APm / APl and AR@1 / @10 / @100 / ARs / ARm / ARl.
# `box_ap` / `mask_ap` above stay what they are (no crowd, area range all, first-of-a-tie); this is a separate route.  The matching of
# `evaluateImg` runs on the device for all classes x area ranges x thresholds of an image in one launch (`ops.coco_match`,
# coco_match_kernel in csrc/boxcover.hip); `accumulate` and `summarize` are `coco_metrics`, host arithmetic on the small per-image records.
# pycocotools is not a dependency of this package: unpinned.
# ------------------------------------------------------------------------------------------------------------------
_COCO_AREAS = ("", "s", "m", "l")                         # all, small, medium, large: the order of ops.COCO_RANGES


def coco_recall_points():
    """COCOeval's recThrs: numpy.linspace(0, 1, 101) as numpy gives them (torch.linspace differs in last bits)"""
    return np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)


def _host_array(x, dtype):
    return np.ascontiguousarray(torch.as_tensor(x).detach().cpu().numpy()).astype(dtype, copy=False)


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
    A, T, M = len(_COCO_AREAS), len(thr), len(max_dets)
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
        res[f"AP{_COCO_AREAS[a]}"] = mean(precision[:, :, :, a, -1])
    for mi, limit in enumerate(max_dets):
        res[f"AR@{limit}"] = mean(recall[:, :, 0, mi])
    for a in range(1, A):
        res[f"AR{_COCO_AREAS[a]}"] = mean(recall[:, :, a, -1])
    if class_names is not None:
        for k, name in enumerate(class_names):
            res[f"AP-{name}"] = mean(precision[:, :, k, 0, -1])
    res.update(images=len(scores), gt=int(n_gt), dets=int((RK < max(max_dets)).sum()), classes=int((npig[:, 0] > 0).sum()))
    return res


def _coco_box_iou(db, gb, crowd):
    """XYXY boxes db [n, 4], gb [m, 4] float64 and crowd bool [m] on one device -> (iou [n, m] with `_iou_matrix`'s arithmetic, a crowd
    column holding inter / area_det; area_det [n]; area_gt [m]), the areas w * h with negative sides taken as 0"""
    area_d = (db[:, 2] - db[:, 0]).clamp_min(0) * (db[:, 3] - db[:, 1]).clamp_min(0)
    area_g = (gb[:, 2] - gb[:, 0]).clamp_min(0) * (gb[:, 3] - gb[:, 1]).clamp_min(0)
    lt = torch.maximum(db[:, None, :2], gb[None, :, :2])
    rb = torch.minimum(db[:, None, 2:], gb[None, :, 2:])
    inter = (rb - lt).clamp_min(0).prod(-1)
    iou = inter / (area_d[:, None] + area_g[None, :] - inter).clamp_min(1e-300)
    return torch.where(crowd[None, :], inter / area_d[:, None].clamp_min(1e-300), iou), area_d, area_g


def _coco_count_iou(inter, area_a, area_b, crowd):
    """integer counts inter [n, m], area_a [n], area_b [m] and crowd bool [m] -> float64 [n, m]: inter / union, a crowd column
    inter / area_a, 0 where the denominator is 0"""
    union = area_a[:, None] + area_b[None, :] - inter
    den = torch.where(crowd[None, :], area_a[:, None].expand_as(union), union)
    return torch.where(den > 0, inter.double() / den.clamp_min(1).double(), torch.zeros((), dtype=torch.float64, device=inter.device))


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
    Out of scope: polygon ground truth (rasterise it first), the LVIS federated rules, OpenImages, keypoints."""

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

    def update(self, pred, scores=None, classes=None, gt=None, gt_classes=None, gt_crowd=None, gt_areas=None):
        """One image.  pred: boxes [n, 4] XYXY ("bbox") or masks [n, H, W] as a device tensor, a host tensor or a list of RLE dicts
        ("segm"), with `scores` [n] and `classes` [n]; or an `Instances` carrying `pred_boxes` / `pred_masks` / `pred_masks_rle` next to
        `scores` and `pred_classes`.  gt: boxes [m, 4] (a tensor or a `Boxes`) or masks in any of the three forms, gt_classes [m],
        gt_crowd [m] (non-zero = a crowd region; default none), gt_areas [m] (see the class).  Host inputs are uploaded."""
        who = "COCOAccumulator.update"
        segm = self.iou_type == "segm"
        if _is_instances(pred):
            inst = pred
            if not segm:
                if not inst.has("pred_boxes"):
                    raise ValueError(f"{who}: the instances carry no pred_boxes")
                pred = inst.pred_boxes
            elif inst.has("pred_masks"):
                pred = inst.pred_masks
            elif inst.has("pred_masks_rle"):
                pred = list(inst.pred_masks_rle)
            else:
                raise ValueError(f"{who}: the instances carry neither pred_masks nor pred_masks_rle")
            scores = inst.scores if scores is None else scores
            classes = inst.pred_classes if classes is None else classes
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
        if self.device is None:
            on_device = [t.device for t in (pred, gt, scores) if torch.is_tensor(t) and t.is_cuda]
            self.device = on_device[0] if on_device else _default_device()
        dev = self.device
        crowd = torch.zeros(m, dtype=torch.bool, device=dev) if gt_crowd is None else gt_crowd.to(dev) != 0
        if not segm:
            iou, det_area, gt_area = _coco_box_iou(pred.to(dev, torch.float64), gt.to(dev, torch.float64), crowd)
        else:
            a = _device_masks(pred, dev) if n > 0 else None
            b = _device_masks(gt, dev) if m > 0 else None
            if a is not None and b is not None and tuple(a.shape[1:]) != tuple(b.shape[1:]):
                raise ValueError(f"{who}: prediction masks {tuple(a.shape[1:])} vs ground truth {tuple(b.shape[1:])}")
            a_bits, area_a = ops.mask_pack_bits(a) if n > 0 else (None, torch.zeros(0, dtype=torch.int64, device=dev))
            b_bits, area_b = ops.mask_pack_bits(b) if m > 0 else (None, torch.zeros(0, dtype=torch.int64, device=dev))
            if n > 0 and m > 0:
                iou = _coco_count_iou(ops.bitmask_pair_counts(a_bits, b_bits), area_a, area_b, crowd)
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
        import torch.distributed as dist
        self._flush()
        parts = [None] * dist.get_world_size(group)
        dist.all_gather_object(parts, self.records, group=group)
        self.records = [r for part in parts for r in part]

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
        g, gc, crowd, areas = (tuple(gt) + (None, None))[:4]
        if _is_instances(det):
            acc.update(det, gt=g, gt_classes=gc, gt_crowd=crowd, gt_areas=areas)
        else:
            acc.update(det[0], det[1], det[2], g, gc, crowd, areas)
    return acc.compute()
