"""Semantic and panoptic scores.  Both reduce to the joint histogram of two label maps, counted on the device by
`ops.label_pair_hist` (csrc/labelhist.hip): the semantic confusion matrix is hist[pred class, gt class], the panoptic segment
intersections are hist[gt segment, pred segment].  What follows the histogram is host arithmetic on small integer matrices."""
import torch

from .. import ops
from ._common import _all_reduce_sum, _distributed, _label_map, pick_device


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
        self._state(pick_device(self.device))                     # a rank without images adds zeros
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

    # long, and left in one piece on purpose: it is ONE protocol (pq_compute_single_core), top to bottom, and repeats nothing of the
    # other families.  `reduce` below is on its own too: it moves HOST tensors to the device only under nccl, not `_all_reduce_sum`'s rule.
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
