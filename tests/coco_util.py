"""The host's word on COCO matching, shared by test_coco_eval.py and test_coco_eval_gpu.py: COCOeval.evaluateImg's scan written out
literally (NOT the two-phase form the kernel uses), the grouping that precedes it, and the IoU of boxes and masks with crowd columns."""
import numpy as np
import torch

THRESHOLDS = np.linspace(0.5, 0.95, 10)
RANGES = [(0.0, 1e5 ** 2), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e5 ** 2)]         # all, small, medium, large


def literal_match(iou, crowd, gt_area, det_area, thresholds=THRESHOLDS, ranges=RANGES):
    """ONE class of one image.  iou [D, G] (detections in descending score order, ground truth in annotation order; a crowd column holds
    inter / area_det), crowd [G], gt_area [G], det_area [D] -> (match int [A, T, D]: the ground truth's index or -1, flag uint8
    [A, T, D]: 1 true positive, 0 false positive, 2 ignored).  COCOeval's loop: the ground truth sorted by the ignore flag with a stable
    sort; per detection a scan that skips what is taken unless it is a crowd, stops when a kept match meets an ignored ground truth,
    skips what lies below the best so far and else replaces the best -- `>=` in effect, so the last of equals wins"""
    iou = np.asarray(iou, dtype=np.float64)
    D, G = iou.shape
    A, T = len(ranges), len(thresholds)
    match = np.full((A, T, D), -1, dtype=np.int64)
    flag = np.zeros((A, T, D), dtype=np.uint8)
    for a, (lo, hi) in enumerate(ranges):
        gt_ig = np.array([1 if (crowd[g] or gt_area[g] < lo or gt_area[g] > hi) else 0 for g in range(G)], dtype=np.int64)
        gtind = np.argsort(gt_ig, kind="mergesort")
        for t, thr in enumerate(thresholds):
            taken = [False] * G
            for d in range(D):
                best = min(float(thr), 1 - 1e-10)
                m = -1
                for g in gtind:
                    if taken[g] and not crowd[g]:
                        continue
                    if m > -1 and gt_ig[m] == 0 and gt_ig[g] == 1:
                        break
                    if iou[d, g] < best:
                        continue
                    best = iou[d, g]
                    m = int(g)
                if m == -1:
                    flag[a, t, d] = 2 if (det_area[d] < lo or det_area[d] > hi) else 0
                    continue
                taken[m] = True
                match[a, t, d] = m
                flag[a, t, d] = 2 if gt_ig[m] else 1
    return match, flag


def group(scores, classes, gt_classes, K, limit=100):
    """(det_order [n'], det_offsets [K + 1], gt_order [m], gt_offsets [K + 1]) as int32 tensors: the detections of each class in descending
    score order (stable: equal scores keep their input order), at most `limit` of them; the ground truth of each class in input order"""
    scores, classes, gt_classes = np.asarray(scores, dtype=np.float64), np.asarray(classes), np.asarray(gt_classes)
    by_score = np.argsort(-scores, kind="stable")
    det_order, det_offsets, gt_order, gt_offsets = [], [0], [], [0]
    for k in range(K):
        det_order += [int(i) for i in by_score if classes[i] == k][:limit]
        det_offsets.append(len(det_order))
        gt_order += [int(j) for j in range(len(gt_classes)) if gt_classes[j] == k]
        gt_offsets.append(len(gt_order))
    as_i32 = lambda v: torch.tensor(v, dtype=torch.int32)                                            # noqa: E731
    return as_i32(det_order), as_i32(det_offsets), as_i32(gt_order), as_i32(gt_offsets)


def host_match(iou, det_order, det_offsets, gt_order, gt_offsets, crowd, gt_area, det_area, thresholds=THRESHOLDS, ranges=RANGES):
    """what `ops.coco_match` is to return, from the literal loop class by class: (match int32 [A, T, n'], flag uint8 [A, T, n'])"""
    iou = np.asarray(iou, dtype=np.float64)
    crowd, gt_area, det_area = np.asarray(crowd), np.asarray(gt_area, dtype=np.float64), np.asarray(det_area, dtype=np.float64)
    do, go = np.asarray(det_order, dtype=np.int64), np.asarray(gt_order, dtype=np.int64)
    A, T = len(ranges), len(thresholds)
    match = np.full((A, T, do.size), -1, dtype=np.int32)
    flag = np.zeros((A, T, do.size), dtype=np.uint8)
    for k in range(len(det_offsets) - 1):
        d0, d1, g0, g1 = int(det_offsets[k]), int(det_offsets[k + 1]), int(gt_offsets[k]), int(gt_offsets[k + 1])
        if d1 == d0:
            continue
        rows, cols = do[d0:d1], go[g0:g1]
        mt, fl = literal_match(iou[np.ix_(rows, cols)].reshape(rows.size, cols.size), crowd[cols], gt_area[cols], det_area[rows],
                               thresholds, ranges)
        match[:, :, d0:d1] = np.where(mt >= 0, cols[np.clip(mt, 0, None)] if cols.size else -1, -1)
        flag[:, :, d0:d1] = fl
    return torch.from_numpy(match), torch.from_numpy(flag)


def gt_ignore(crowd, gt_area, ranges=RANGES):
    crowd, gt_area = np.asarray(crowd).astype(bool), np.asarray(gt_area, dtype=np.float64)
    return torch.from_numpy(np.stack([crowd | (gt_area < lo) | (gt_area > hi) for lo, hi in ranges]).astype(np.uint8).reshape(len(ranges), -1))


def host_record(iou, scores, classes, gt_classes, crowd, gt_area, det_area, K, limit=100, thresholds=THRESHOLDS):
    """one image's record for `coco_metrics` from the literal matcher: (scores, classes, flag, gt_classes, gt_ignore)"""
    do, doff, go, goff = group(scores, classes, gt_classes, K, limit)
    _, flag = host_match(iou, do, doff, go, goff, crowd, gt_area, det_area, thresholds)
    idx = do.long()
    return (torch.as_tensor(scores, dtype=torch.float64)[idx], torch.as_tensor(classes, dtype=torch.int64)[idx], flag,
            torch.as_tensor(gt_classes, dtype=torch.int64), gt_ignore(crowd, gt_area))


def box_iou(db, gb, crowd):
    """float64 on the host: (iou [n, m] with a crowd column = inter / area_det, det_area [n], gt_area [m]); the arithmetic of
    `evaluation._iou_matrix`, one rounding per operation"""
    db, gb = torch.as_tensor(db).double().cpu(), torch.as_tensor(gb).double().cpu()
    crowd = torch.as_tensor(crowd).cpu() != 0
    area_d = (db[:, 2] - db[:, 0]).clamp_min(0) * (db[:, 3] - db[:, 1]).clamp_min(0)
    area_g = (gb[:, 2] - gb[:, 0]).clamp_min(0) * (gb[:, 3] - gb[:, 1]).clamp_min(0)
    w = (torch.minimum(db[:, None, 2], gb[None, :, 2]) - torch.maximum(db[:, None, 0], gb[None, :, 0])).clamp_min(0)
    h = (torch.minimum(db[:, None, 3], gb[None, :, 3]) - torch.maximum(db[:, None, 1], gb[None, :, 1])).clamp_min(0)
    inter = w * h
    iou = inter / (area_d[:, None] + area_g[None, :] - inter).clamp_min(1e-300)
    return torch.where(crowd[None, :], inter / area_d[:, None].clamp_min(1e-300), iou), area_d, area_g


def mask_iou(a, b, crowd):
    """uint8 masks a [n, H, W], b [m, H, W] on the host -> (iou float64 [n, m] from integer counts: inter / union, a crowd column
    inter / area_det, 0 where the denominator is 0; det_area [n]; gt_area [m])"""
    a, b = torch.as_tensor(a).cpu().flatten(1).long(), torch.as_tensor(b).cpu().flatten(1).long()
    crowd = torch.as_tensor(crowd).cpu() != 0
    inter = (a != 0).long() @ (b != 0).long().t()
    area_a, area_b = (a != 0).sum(1), (b != 0).sum(1)
    den = torch.where(crowd[None, :], area_a[:, None].expand_as(inter), area_a[:, None] + area_b[None, :] - inter)
    iou = torch.where(den > 0, inter.double() / den.clamp_min(1).double(), torch.zeros((), dtype=torch.float64))
    return iou, area_a.double(), area_b.double()
