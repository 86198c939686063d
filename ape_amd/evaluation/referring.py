"""Referring expressions (RefCOCO / RefCOCO+ / RefCOCOg; ape/evaluation/refcoco_evaluation.py:377-421, refcocoeval.py:17-39,201-250).
Expression mode returns ONE detection per expression, so the scores are PAIRED: sample i needs |pred_i & gt_i|, |pred_i| and |gt_i|,
which `ops.mask_paired_counts` (csrc/maskiou.hip) counts in one pass over the two byte masks, straight into a row of a device table."""
import torch

from .. import ops
from ._common import (_device_masks, _distributed, _is_instances, gather_objects, instance_fields, mask_size, optional_tail,
                      pick_device)

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


class ReferringAccumulator:
    """The referring-expression scores of a dataset (`referring_metrics`: oIoU, mIoU, P@k, mask_P@k).  The state is a device table,
    int64 [capacity, 3] with a float64 [capacity, 8] companion for the boxes: `update` has `ops.mask_paired_counts` write the sample's
    row directly (`out=` a one-row view) and, when the masks are on the device already, issues no device-to-host copy and no
    synchronisation; the tables grow by doubling with a device-to-device copy, and `compute` reads them back once.
    The ground truth may be the annotation's COCO polygons (rasterised on the device as the reference's annToRLE does: `update`'s
    `image_size`).  Out of scope: the COCO-style AP the reference also prints for these datasets (that is `box_ap` / `mask_ap`), gRefCOCO's
    N-acc / T-acc."""

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
    def _one_mask(mask, device, who, size=None):
        """[1, H, W] on the device from a [H, W] / [1, H, W] tensor (device or host), one RLE dict or one object's polygon list (rasterised
        at `size`)"""
        if isinstance(mask, (dict, list, tuple)):
            return _device_masks([mask], device, size)
        if mask.dim() == 2:
            mask = mask[None]
        if mask.dim() != 3 or mask.shape[0] != 1:
            raise ValueError(f"ReferringAccumulator.update: {who} must be one mask, [H, W] or [1, H, W], got {tuple(mask.shape)}")
        return _device_masks(mask, device)

    def update(self, pred=None, gt_mask=None, gt_box=None, pred_mask=None, pred_box=None, image_size=None):
        """One sample.  The prediction is either `pred`, an `Instances` as expression mode returns it (`pred_masks` or `pred_masks_rle`,
        `pred_boxes`, `scores`; the highest-scoring instance is taken, on a tie the first, as the reference's stable sort does), or
        `pred_mask` ([H, W] / [1, H, W] uint8 / bool on the device or the host, or one RLE dict) with an optional `pred_box` (XYXY).
        Neither, or an `Instances` of length 0, is a sample without prediction: it scores as an empty mask, (0, 0, area_gt), and is a
        box miss.  gt_mask: a device tensor, a host tensor, one RLE dict or the annotation's polygon list (ONE object: a list of flat
        [x0, y0, x1, y1, ...] lists), which is rasterised at image_size = (H, W) -- by default the predicted mask's size; gt_box:
        optional XYXY -- with it the sample takes part in P@k, and then every sample of the dataset must."""
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
            masks, scores, _ = instance_fields(pred, "masks", "ReferringAccumulator.update")
            rles, masks = (masks, None) if isinstance(masks, list) else (None, masks)
            pb = pred.pred_boxes.tensor if with_boxes else None
            scores = torch.as_tensor(scores).reshape(-1)
            if len(pred) == 1:
                first = slice(0, 1)
            else:
                order = torch.argsort(scores, descending=True, stable=True)[:1]
                if scores.is_cuda and masks is not None and masks.device == scores.device and (pb is None or pb.device == scores.device):
                    first = order                                 # everything is on the device: the choice stays there, no read-back
                else:
                    first = slice(int(order), int(order) + 1)
            pred_mask = masks[first] if masks is not None else rles[first.start]
            pred_box = pb[first] if with_boxes else None
        dev = pick_device(self.device, gt_mask, pred_mask)
        gt = self._one_mask(gt_mask, dev, "gt_mask", mask_size(image_size, pred_mask, gt_mask)).to(dev)
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
        parts = [p for p in gather_objects(self._host_rows(), group) if p[0].shape[0] > 0]
        if not parts:
            return
        if len({p[1] is None for p in parts}) != 1:
            raise ValueError("ReferringAccumulator.reduce: some ranks have boxes and some do not")
        counts = torch.cat([p[0] for p in parts])
        self.with_boxes = parts[0][1] is not None
        dev = pick_device(self.device)
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
        pred, gt_mask, gt_box = optional_tail(s, 3)
        if pred is None or _is_instances(pred):
            acc.update(pred, gt_mask, gt_box)
        elif isinstance(pred, (tuple, list)):
            acc.update(None, gt_mask, gt_box, pred_mask=pred[0], pred_box=pred[1])
        else:
            acc.update(None, gt_mask, gt_box, pred_mask=pred)
    return acc.compute()
