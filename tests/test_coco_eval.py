"""COCO's full protocol without a GPU: the default thresholds and recall points bit for bit, `coco_metrics` on a hand-computed dataset,
its agreement with `box_ap` where the two protocols coincide (the literal host matcher of coco_util feeds it), the rejections of
`ops.coco_match` that need no device, and the link line."""
import math
import os

import numpy as np
import pytest
import torch

import coco_util as U


def test_default_thresholds_and_recall_points_are_numpys():
    from ape_amd import ops
    from ape_amd.evaluation import coco_recall_points
    want = np.linspace(0.5, 0.95, 10)
    assert len(ops.COCO_THRESHOLDS) == 10 and all(type(v) is float for v in ops.COCO_THRESHOLDS)
    assert np.array(ops.COCO_THRESHOLDS).tobytes() == want.tobytes()
    naive = [0.5 + 0.05 * i for i in range(10)]
    assert [i for i in range(10) if naive[i] != ops.COCO_THRESHOLDS[i]] == [7, 8]       # 0.85 and 0.90 differ in the last bit
    assert 17 / 20 >= ops.COCO_THRESHOLDS[7] and not 17 / 20 >= naive[7]
    points = coco_recall_points()
    assert points.dtype == np.float64 and points.tobytes() == np.linspace(0, 1, 101).tobytes()
    assert points.tobytes() != torch.linspace(0, 1, 101, dtype=torch.float64).numpy().tobytes()
    assert ops.COCO_RANGES == ((0.0, 1e10), (0.0, 1024.0), (1024.0, 9216.0), (9216.0, 1e10))


def _hand_records():
    """Three classes (cat, dog, bird), two images, flags written by hand; thresholds 0 .. 4 ("low") and 5 .. 9 ("high") differ in one flag.
    Image 0: ground truth g0 cat of area 500 (small), g1 cat crowd, g2 dog of area 2000 (medium).  Cat detections in score order:
      d1 .97 on the crowd           -> ignored (2) under every range
      d2 .92 unmatched, area 20000  -> false positive (0) under all and large, ignored under small and medium (outside the range)
      d0 .90 on g0                  -> true positive (1) under all and small, ignored under medium and large (g0 is outside them)
    Image 1: two small cats; e0 .95 and e1 .85 are true positives under all and small -- e1 only at the low thresholds, a false
    positive at the high ones -- and ignored under medium and large.  No dog is ever detected; there is no bird at all."""
    A, T = 4, 10
    f0 = torch.zeros((A, T, 3), dtype=torch.uint8)
    f0[0, :] = torch.tensor([2, 0, 1], dtype=torch.uint8)
    f0[1, :] = torch.tensor([2, 2, 1], dtype=torch.uint8)
    f0[2, :] = torch.tensor([2, 2, 2], dtype=torch.uint8)
    f0[3, :] = torch.tensor([2, 0, 2], dtype=torch.uint8)
    ig0 = torch.tensor([[0, 1, 0], [0, 1, 1], [1, 1, 0], [1, 1, 1]], dtype=torch.uint8)
    f1 = torch.full((A, T, 2), 2, dtype=torch.uint8)
    f1[:2, :5] = torch.tensor([1, 1], dtype=torch.uint8)
    f1[:2, 5:] = torch.tensor([1, 0], dtype=torch.uint8)
    ig1 = torch.tensor([[0, 0], [0, 0], [1, 1], [1, 1]], dtype=torch.uint8)
    return [(torch.tensor([0.97, 0.92, 0.90], dtype=torch.float64), torch.tensor([0, 0, 0]), f0, torch.tensor([0, 0, 1]), ig0),
            (torch.tensor([0.95, 0.85], dtype=torch.float64), torch.tensor([0, 0]), f1, torch.tensor([0, 0]), ig1)]


def test_coco_metrics_on_a_hand_computed_dataset():
    """Cats under "all", limit 100, in score order d1 e0 d2 d0 e1; 3 cats count (the crowd does not).  With e = numpy.spacing(1) and
    p1 = 1 / (1 + e) (2 + e and 4 + e round to 2 and 4; 2 / (3 + e) rounds to the float 2 / 3):
      low thresholds:  flags 2 1 0 1 1 -> tp 0 1 1 2 3, fp 0 0 1 1 1, recall 0 1/3 1/3 2/3 1, precision 0 p1 1/2 2/3 3/4, from the right
                       p1 p1 3/4 3/4 3/4.  Recall points 0 .. 0.33 (34 of them) find index 0 or 1 -> p1; 0.34 .. 1 (67) find 3 or 4 -> 3/4.
                       Had the crowd match d1 counted as a false positive, the first value would be 1/2.
      high thresholds: flags 2 1 0 1 0 -> tp 0 1 1 2 2, fp 0 0 1 1 2, recall .. 2/3 2/3, precision 0 p1 1/2 2/3 1/2, from the right
                       p1 p1 2/3 2/3 1/2: 34 points p1, 0.34 .. 0.66 (33) -> 2/3, 0.67 .. 1 (34) lie past the end -> 0.
    Cats under "small": d2 is ignored, so there is no false positive at the low thresholds (AP 1, recall 1); at the high ones flags
    2 1 2 1 0 give precision 1 up to recall 2/3 (67 points) and 0 beyond.
    Dogs: one medium ground truth, no detection: precision 0 and recall 0 under all and medium.  Birds: nothing, left out everywhere.
    Small has no dog and medium no cat that counts: APs and ARs are the cats' alone, APm and ARm the dogs' alone (0); large has nothing.
    Limit 1 keeps d1 (ignored) and e0 (true positive): cat recall 1/3 at every threshold."""
    from ape_amd.evaluation import coco_metrics
    e = np.spacing(1)
    p1 = 1 / (1 + e)
    assert p1 < 1.0 and 2 / (2 + e) == 1.0 and 2 / (3 + e) == 2 / 3 and 3 / (4 + e) == 0.75
    cat_low, cat_high = (34 * p1 + 67 * 0.75) / 101, (34 * p1 + 33 * (2 / 3)) / 101
    want = {"AP": (cat_low + cat_high) / 2 / 2, "AP50": cat_low / 2, "AP75": cat_high / 2,
            "APs": (1.0 + 67 / 101) / 2, "APm": 0.0, "APl": float("nan"),
            "AR@1": (1 / 3) / 2, "AR@10": (1.0 + 2 / 3) / 2 / 2, "AR@100": (1.0 + 2 / 3) / 2 / 2,
            "ARs": (1.0 + 2 / 3) / 2, "ARm": 0.0, "ARl": float("nan"),
            "AP-cat": (cat_low + cat_high) / 2, "AP-dog": 0.0, "AP-bird": float("nan")}
    got = coco_metrics(_hand_records(), 3, class_names=["cat", "dog", "bird"])
    assert set(got) == set(want) | {"images", "gt", "dets", "classes"}
    assert (got["images"], got["gt"], got["dets"], got["classes"]) == (2, 5, 5, 2)
    for k, v in want.items():
        # a mean of at most 10 x 101 x 3 doubles in [0, 1]: its rounding error stays below 3030 x 2^-53 < 4e-13 however it is summed
        assert (math.isnan(got[k]) and math.isnan(v)) or abs(got[k] - v) < 4e-13, (k, got[k], v)
    assert got["AR@1"] < got["AR@10"] and got["AP75"] < got["AP50"] and got["APs"] > got["AP"]
    plain = coco_metrics(_hand_records(), 3)
    assert not any(k.startswith("AP-") for k in plain) and plain["AP"] == got["AP"]
    # the order of the images decides nothing here (no equal scores across images)
    assert coco_metrics(_hand_records()[::-1], 3)["AP"] == got["AP"]


def test_coco_metrics_of_nothing_is_nan():
    from ape_amd.evaluation import coco_metrics
    got = coco_metrics([], 3, class_names=["a", "b", "c"])
    keys = ["AP", "AP50", "AP75", "APs", "APm", "APl", "AR@1", "AR@10", "AR@100", "ARs", "ARm", "ARl", "AP-a", "AP-b", "AP-c"]
    assert set(got) == set(keys) | {"images", "gt", "dets", "classes"}
    assert all(math.isnan(got[k]) for k in keys)
    assert (got["images"], got["gt"], got["dets"], got["classes"]) == (0, 0, 0, 0)
    # detections without any ground truth: still nothing to average
    empty = (torch.tensor([0.5]), torch.tensor([1]), torch.zeros((4, 10, 1), dtype=torch.uint8), torch.zeros(0, dtype=torch.int64),
             torch.zeros((4, 0), dtype=torch.uint8))
    got = coco_metrics([empty], 3)
    assert math.isnan(got["AP"]) and math.isnan(got["AR@100"]) and got["dets"] == 1 and got["images"] == 1


def test_coco_metrics_rejects_malformed_records():
    from ape_amd.evaluation import coco_metrics
    ok = _hand_records()
    with pytest.raises(ValueError):
        coco_metrics(ok, 3, class_names=["a", "b"])
    with pytest.raises(ValueError):
        coco_metrics(ok, 1)                                                  # the dog is class 1
    with pytest.raises(ValueError):
        coco_metrics([(ok[0][0], ok[0][1], ok[0][2][:, :, :2], ok[0][3], ok[0][4])], 3)
    with pytest.raises(ValueError):
        coco_metrics([(ok[0][0], ok[0][1], ok[0][2], ok[0][3], ok[0][4][:3])], 3)
    with pytest.raises(ValueError):
        coco_metrics(ok, 3, max_dets=())


def _generic_boxes(k, g):
    xy = torch.rand((k, 2), generator=g, dtype=torch.float64) * 400
    wh = torch.rand((k, 2), generator=g, dtype=torch.float64) * 150 + 10
    return torch.cat([xy, xy + wh], 1)


def test_agrees_with_box_ap_where_the_protocols_coincide():
    """generic float64 boxes (no two IoUs or scores tie), no crowd, range "all", the thresholds 0.5 + 0.05 i given to both sides: the
    literal matcher + `coco_metrics` and `box_ap` differ only in `+ spacing(1)` against `clamp_min(1e-300)` in a precision <= 1 -- a
    relative 2.3e-16 per value, before a mean.  The classes have 7, 11 and 13 ground truths in all: tp / 7, tp / 11 and tp / 13 meet a
    recall point k / 100 only at 0 and 1, which numpy's and torch's linspace both hold exactly."""
    from ape_amd.evaluation import box_ap, coco_metrics
    thr = [0.5 + 0.05 * i for i in range(10)]
    g = torch.Generator().manual_seed(17)
    gt_classes = [[0, 0, 1, 1, 2, 2, 2, 1], [0, 0, 0, 1, 1, 2, 2, 2, 2], [0, 1, 1, 1, 2, 2, 2], [0, 1, 1, 1, 2, 2, 2]]
    assert [sum(c.count(k) for c in gt_classes) for k in range(3)] == [7, 11, 13]
    dets, gts, records = [], [], []
    for classes in gt_classes:
        gc = torch.tensor(classes)
        gb = _generic_boxes(len(classes), g)
        near = gb.repeat(3, 1) + (torch.rand((3 * len(classes), 4), generator=g, dtype=torch.float64) - 0.5) * 30
        db = torch.cat([near, _generic_boxes(10, g)])
        dc = torch.cat([gc.repeat(3), torch.randint(0, 3, (10,), generator=g)])
        ds = torch.rand(db.shape[0], generator=g, dtype=torch.float64)
        dets.append((db, ds, dc))
        gts.append((gb, gc))
        iou, det_area, gt_area = U.box_iou(db, gb, torch.zeros(len(classes)))
        records.append(U.host_record(iou.numpy(), ds.numpy(), dc.numpy(), gc.numpy(), np.zeros(len(classes), dtype=bool), gt_area.numpy(),
                                     det_area.numpy(), 3, thresholds=thr))
    old = box_ap(dets, gts, iou_thresholds=thr)
    new = coco_metrics(records, 3, iou_thresholds=thr)
    assert 0.05 < old["AP"] < 0.95 and old["AP75"] < old["AP50"]
    for k in ("AP", "AP50", "AP75"):
        assert abs(new[k] - old[k]) <= 1e-12, (k, new[k], old[k])
    assert (new["classes"], new["gt"], new["dets"]) == (old["classes"], old["gt"], old["dets"])


def test_literal_matcher_on_the_named_rules():
    """the test's own reference, checked by hand on the cases the kernel tests name: the last of equal IoUs, a not-ignored ground truth
    over a crowd of higher IoU, two detections on one crowd, an area-ignored ground truth only once"""
    one = [(0.0, 1e10)]
    mt, fl = U.literal_match([[0.6, 0.6, 0.6]], [0, 0, 0], [100.0] * 3, [100.0], [0.5], one)
    assert mt[0, 0].tolist() == [2] and fl[0, 0].tolist() == [1]
    mt, fl = U.literal_match([[0.6, 0.9]], [0, 1], [100.0] * 2, [100.0], [0.5], one)
    assert mt[0, 0].tolist() == [0] and fl[0, 0].tolist() == [1]
    mt, fl = U.literal_match([[0.8], [0.7]], [1], [100.0], [100.0] * 2, [0.5], one)
    assert mt[0, 0].tolist() == [0, 0] and fl[0, 0].tolist() == [2, 2]
    mt, fl = U.literal_match([[0.8], [0.7]], [0], [5000.0], [100.0] * 2, [0.5], [(0.0, 1024.0)])
    assert mt[0, 0].tolist() == [0, -1] and fl[0, 0].tolist() == [2, 0]


def test_coco_match_rejections_that_need_no_device():
    from ape_amd import ops
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)                         # noqa: E731
    args = dict(iou=torch.rand(3, 2, dtype=torch.float64), det_order=i32([0, 1, 2]), det_offsets=i32([0, 3]), gt_order=i32([0, 1]),
                gt_offsets=i32([0, 2]), gt_crowd=torch.zeros(2, dtype=torch.uint8), gt_area=torch.rand(2, dtype=torch.float64),
                det_area=torch.rand(3, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        ops.coco_match(**args)                                                 # host tensors: there is no CPU path
    with pytest.raises(RuntimeError):
        ops.coco_match(**args, thresholds=torch.tensor([0.5], dtype=torch.float64))
    for name, bad in (("iou", args["iou"].float()), ("det_order", args["det_order"].long()), ("gt_offsets", args["gt_offsets"].long()),
                      ("gt_crowd", args["gt_crowd"].bool()), ("gt_area", args["gt_area"].float()), ("det_area", [0.0, 1.0, 2.0])):
        with pytest.raises(TypeError):
            ops.coco_match(**{**args, name: bad})
    with pytest.raises(TypeError):
        ops.coco_match(**args, thresholds=torch.tensor([0.5]))                 # float32 thresholds
    for name, bad in (("iou", torch.rand(2, 3, dtype=torch.float64).t()),      # [3, 2] with the inner stride 3
                      ("iou", torch.rand(6, dtype=torch.float64)), ("gt_offsets", i32([0, 1, 2])),      # K + 1 = 3 against 2
                      ("det_offsets", i32([[0, 3]])), ("gt_crowd", torch.zeros(3, dtype=torch.uint8)),
                      ("gt_area", torch.rand(3, dtype=torch.float64)), ("det_area", torch.rand(2, dtype=torch.float64)),
                      ("det_order", i32([0, 9, 1, 9, 2, 9])[::2]), ("gt_order", torch.zeros(4097, dtype=torch.int32)),
                      ("det_order", torch.zeros(65536, dtype=torch.int32))):
        with pytest.raises(ValueError):
            ops.coco_match(**{**args, name: bad})
    with pytest.raises(ValueError):
        ops.coco_match(**args, ranges=torch.zeros((2, 3), dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.coco_match(**{**args, "det_offsets": i32([0]), "gt_offsets": i32([0])})          # detections, but K = 0


def test_accumulator_rejections_that_need_no_device():
    from ape_amd.evaluation import COCOAccumulator, coco_eval
    with pytest.raises(ValueError):
        COCOAccumulator("keypoints", 3)
    with pytest.raises(ValueError):
        COCOAccumulator("bbox", 0)
    with pytest.raises(ValueError):
        COCOAccumulator("bbox", 3, class_names=["a"])
    acc = COCOAccumulator("bbox", 3, device="cpu")
    boxes = torch.tensor([[0.0, 0.0, 10.0, 10.0]])
    with pytest.raises(ValueError):
        acc.update(boxes, torch.tensor([0.5]), torch.tensor([0]))                              # no ground truth given at all
    with pytest.raises(ValueError):
        acc.update(boxes, torch.tensor([0.5, 0.4]), torch.tensor([0]), boxes, torch.tensor([0]))
    with pytest.raises(ValueError):
        acc.update(boxes, torch.tensor([0.5]), torch.tensor([3]), boxes, torch.tensor([0]))    # class 3 of 3
    with pytest.raises(ValueError):
        acc.update(boxes, torch.tensor([0.5]), torch.tensor([0]), boxes, torch.tensor([0]), gt_crowd=torch.tensor([0, 1]))
    with pytest.raises(RuntimeError):
        acc.update(boxes, torch.tensor([0.5]), torch.tensor([0]), boxes, torch.tensor([0]))    # a host device: there is no CPU path
    with pytest.raises(ValueError):
        coco_eval([], [], "bbox")
    assert math.isnan(coco_eval([], [], "bbox", num_classes=2)["AP"])


def test_link_line_is_the_parents():
    """no new object: the kernel lives in boxcover.hip, which stays last behind the alphabetical rest"""
    from ape_amd import build
    names = [os.path.basename(f) for f in build._sources()]
    assert names == ["attention.hip", "boundary.hip", "boxes.hip", "error.cpp", "ffn_fused.hip", "gemm.hip", "gemm_p8.hip", "geometry.hip",
                     "hostcopy.cpp", "imageio.hip", "labelhist.hip", "maskiou.hip", "masks.hip", "meter.cpp", "msda.hip", "norm.hip",
                     "relpos.hip", "select.hip", "softmax.hip", "spatial.hip", "topk.hip", "vlpool.hip", "boxcover.hip"]
