"""Box proposals (ape/evaluation/lvis_evaluation.py:293-399, the same function in refcoco_evaluation.py and d3_evaluation.py; reported by
`_eval_box_proposals` as AR@100 .. ARl@1000).  Recall of the class-agnostic boxes: how a two-stage detector's proposal selection is
judged apart from its classification.  The greedy coverage loop runs on the device (`ops.box_cover_overlaps`, csrc/boxcover.hip), all
eight (area range, limit) combinations of an image in one launch; what is kept per dataset is two small integer tables."""
import torch

from .. import ops
from ._common import _AREAS, _all_reduce_sum, _distributed, _is_instances, optional_tail, pick_device


def proposal_recall_thresholds():
    """the reference's IoU thresholds 0.5, 0.55 .. 0.95 as the float32 values its `torch.arange` gives"""
    return torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)


def proposal_recall_names(limits=(100, 1000)):
    """AR@100, ARs@100, ARm@100, ARl@100, AR@1000, ... : the rows of the tables, limit outer, area inner"""
    return [f"AR{a}@{int(k)}" for k in limits for a in _AREAS]


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
        dev = self._state(pick_device(self.device, boxes, gt_boxes, logits))
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
        self._state(pick_device(self.device))                     # a rank without images adds zeros
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
        proposals, gt_boxes, gt_areas = optional_tail(s, 3)
        if _is_instances(proposals):
            acc.update(proposals, gt_boxes, gt_areas)
        else:
            acc.update(None, gt_boxes, gt_areas, boxes=proposals[0], logits=proposals[1])
    return acc.compute()
