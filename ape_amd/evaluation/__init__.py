"""Scoring a model's output, with the counting on the device (`ape_amd.ops`) and the protocol arithmetic on the host.  Everything is
imported from here; the modules:
  wire          the evaluators' wire format: `instances_to_coco_json`, `encode_masks` / `decode_masks` (COCO RLE, run lengths made on the device),
                and the annotations' side of it: `segmentations_to_masks` / `pack_polygons` (COCO polygons rasterised on the device as annToRLE does)
  ap            COCO-style AP, area range "all", no crowd: `box_ap` (the benchmark's score), `mask_ap`, `boundary_ap` and their accumulators
  coco          COCOeval's full protocol -- crowd, area ranges, AP / AR: `COCOAccumulator`, `coco_eval`, `coco_metrics`
  segmentation  `SemSegAccumulator` (mIoU, fwIoU, mACC, pACC) and `PanopticAccumulator` (PQ, SQ, RQ) on the label-pair histogram
  referring     `ReferringAccumulator`, `referring_scores`: oIoU, mIoU, P@k of one prediction per expression
  proposals     `ProposalRecallAccumulator`, `proposal_recall`: AR@100 / AR@1000 by area of class-agnostic boxes
  _common       what they share: reading an `Instances`, choosing the device, gathering over ranks, the float64 box IoU
A new protocol is a matching rule plus a summary on top of `_common`.  Every module reaches the kernels as `ops.<name>` (`from .. import
ops`), never through a name imported from `ape_amd.ops`, so that replacing an attribute of `ape_amd.ops` reaches all of them."""
from .. import ops
from ._common import _coco_box_iou                                                                      # noqa: F401
from .ap import BoundaryAPAccumulator, MaskAPAccumulator, _coco_ap, _iou_matrix, boundary_ap, boundary_iou, box_ap, mask_ap   # noqa: F401
from .coco import COCOAccumulator, _coco_groups, coco_eval, coco_metrics, coco_recall_points            # noqa: F401
from .proposals import (ProposalRecallAccumulator, proposal_recall, proposal_recall_metrics, proposal_recall_names,    # noqa: F401
                        proposal_recall_thresholds)
from .referring import ReferringAccumulator, referring_metrics, referring_scores                        # noqa: F401
from .segmentation import PanopticAccumulator, SemSegAccumulator, panoptic_quality, semantic_metrics    # noqa: F401
from .wire import (decode_masks, encode_masks, instances_to_coco_json, pack_polygons, rles_from_runs,    # noqa: F401
                   segmentations_to_masks)

_coco_count_iou = ops.count_iou                           # its name before it moved to ops; tests import it from here
