"""Time COCO matching of ONE image -- COCOeval.evaluateImg for all classes x 4 area ranges x 10 IoU thresholds -- on the device against
the same rule as a host loop:
    (a) ops.coco_match(iou, groups...)            one launch, the IoU matrix and the grouping given
    (b) COCOAccumulator("bbox").update(...)       what an evaluation pays per image: box IoU, three sorts, (a), nothing read back
    (c) the host: the IoU matrix read back, then COCOeval's scan as a Python loop per class, range and threshold (what pycocotools'
        evaluateImg is)
at 100 detections x 20 ground truths over 80 classes (COCO) and 300 x 60 over 1203 (LVIS' vocabulary), boxes in a 1333 x 800 image: two
thirds of the detections are jittered ground truth with its class, a tenth of the ground truth is crowd.  (a) is first compared for
equality -- matches and flags -- with (c).  (a) and (b) are timed eagerly with device events around one call and a synchronise before
it, (c) with the host's clock including its read-back; the routes are sampled in alternation; the median and the spread (max - min over
the samples) of each are printed.  The parent of this route has no full-protocol matcher to compare with.

    python tools/gpu_probe_cocomatch.py [--out profiles/cocomatch_timing.txt] [--samples 7]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def scene(n, m, K, seed):
    """(boxes [n, 4], scores [n], classes [n], gt [m, 4], gt_classes [m], gt_crowd [m]) on the host, float64 boxes"""
    g = torch.Generator().manual_seed(seed)
    wh = 12 + 388 * torch.rand((m, 2), generator=g, dtype=torch.float64) ** 2
    xy = torch.rand((m, 2), generator=g, dtype=torch.float64) * (torch.tensor([1333.0, 800.0], dtype=torch.float64) - wh)
    gt = torch.cat([xy, xy + wh], 1)
    gc = torch.randint(0, K, (m,), generator=g)
    pick = torch.randint(0, m, (n,), generator=g)
    src = gt[pick]
    size = torch.cat([src[:, 2:] - src[:, :2]] * 2, 1)
    near = src + (torch.rand((n, 4), generator=g, dtype=torch.float64) - 0.5) * 0.4 * size
    rwh = 12 + 388 * torch.rand((n, 2), generator=g, dtype=torch.float64)
    rxy = torch.rand((n, 2), generator=g, dtype=torch.float64) * (torch.tensor([1333.0, 800.0], dtype=torch.float64) - rwh).clamp_min(1)
    far = torch.cat([rxy, rxy + rwh], 1)
    hit = torch.rand(n, generator=g) < 2 / 3
    boxes = torch.where(hit[:, None], near, far)
    classes = torch.where(hit, gc[pick], torch.randint(0, K, (n,), generator=g))
    scores = torch.rand(n, generator=g, dtype=torch.float64)
    crowd = (torch.rand(m, generator=g) < 0.1).to(torch.uint8)
    return boxes, scores, classes, gt, gc, crowd


def host_loop(iou, det_order, det_offsets, gt_order, gt_offsets, crowd, gt_area, det_area, thresholds, ranges):
    """COCOeval's scan, class by class: ground truth sorted by the ignore flag (stable); per detection skip what is taken unless crowd,
    stop when a kept match meets an ignored ground truth, skip what lies below the best so far, else replace the best"""
    A, T = len(ranges), len(thresholds)
    match = np.full((A, T, len(det_order)), -1, dtype=np.int32)
    flag = np.zeros((A, T, len(det_order)), dtype=np.uint8)
    for k in range(len(det_offsets) - 1):
        d0, d1, g0, g1 = det_offsets[k], det_offsets[k + 1], gt_offsets[k], gt_offsets[k + 1]
        if d1 == d0:
            continue
        cols = [int(c) for c in gt_order[g0:g1]]
        for a, (lo, hi) in enumerate(ranges):
            ig = [1 if (crowd[c] or gt_area[c] < lo or gt_area[c] > hi) else 0 for c in cols]
            scan = sorted(range(len(cols)), key=lambda j: ig[j])
            for t, thr in enumerate(thresholds):
                taken = [False] * len(cols)
                for pos in range(d0, d1):
                    row = int(det_order[pos])
                    best, m = min(thr, 1 - 1e-10), -1
                    for j in scan:
                        if taken[j] and not crowd[cols[j]]:
                            continue
                        if m > -1 and ig[m] == 0 and ig[j] == 1:
                            break
                        v = iou[row, cols[j]]
                        if v < best:
                            continue
                        best, m = v, j
                    if m == -1:
                        flag[a, t, pos] = 2 if (det_area[row] < lo or det_area[row] > hi) else 0
                    else:
                        taken[m] = True
                        match[a, t, pos] = cols[m]
                        flag[a, t, pos] = 2 if ig[m] else 1
    return match, flag


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3                      # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"

    from ape_amd import evaluation, ops

    thresholds, ranges = list(ops.COCO_THRESHOLDS), list(ops.COCO_RANGES)
    lines = [f"coco_match (one launch: all classes x 4 area ranges x 10 thresholds of an image) on {torch.cuda.get_device_name(0)} against the host "
             f"loop; eager calls, device events around one call (host loop: host clock, read-back included); {args.samples} samples per "
             f"route in alternation; microseconds per image",
             f"{'n x m / K':>16} {'groups':>6} | {'coco_match':>10} {'spread':>8} | {'update':>8} {'spread':>8} | {'host loop':>10} {'spread':>9} | "
             f"loop / coco_match | loop / update | equal"]
    ok = True
    for n, m, K in ((100, 20, 80), (300, 60, 1203)):
        boxes, scores, classes, gt, gc, crowd = [t.cuda() for t in scene(n, m, K, 11 * m + 1)]
        iou, det_area, gt_area = evaluation._coco_box_iou(boxes, gt, crowd != 0)
        det_order, det_offsets, gt_order, gt_offsets, _ = evaluation._coco_groups(scores, classes, gc, K, 100)
        dthr, drng = ops.coco_match_tables("cuda")
        match = torch.empty((4, 10, n), dtype=torch.int32, device="cuda")
        flag = torch.empty((4, 10, n), dtype=torch.uint8, device="cuda")
        acc = evaluation.COCOAccumulator("bbox", K, device="cuda")

        def ours():
            return ops.coco_match(iou, det_order, det_offsets, gt_order, gt_offsets, crowd, gt_area, det_area, thresholds=dthr, ranges=drng,
                                  match=match, flag=flag)

        def update():
            acc.update(boxes, scores, classes, gt, gc, gt_crowd=crowd)
            acc._pending.clear()                               # timing only: nothing is kept

        def host():
            t0 = time.perf_counter()
            r = host_loop(iou.cpu().numpy(), det_order.cpu().tolist(), det_offsets.cpu().tolist(), gt_order.cpu().tolist(),
                          gt_offsets.cpu().tolist(), crowd.cpu().tolist(), gt_area.cpu().tolist(), det_area.cpu().tolist(), thresholds, ranges)
            return (time.perf_counter() - t0) * 1e6, r
        ours()
        update()
        torch.cuda.synchronize()
        _, (hmt, hfl) = host()
        kept = int(det_offsets[-1])
        groups = int(((det_offsets[1:] - det_offsets[:-1]) > 0).sum())
        same = np.array_equal(match.cpu().numpy()[:, :, :kept], hmt[:, :, :kept]) and np.array_equal(flag.cpu().numpy()[:, :, :kept], hfl[:, :, :kept])
        verdict = "yes" if same else (f"NO: {int((match.cpu().numpy()[:, :, :kept] != hmt[:, :, :kept]).sum())} matches / "
                                      f"{int((flag.cpu().numpy()[:, :, :kept] != hfl[:, :, :kept]).sum())} flags differ")
        ok = ok and same
        times = [[], [], []]
        for _ in range(2):                                     # warm
            timed(ours)
            timed(update)
        for _ in range(args.samples):
            times[0].append(timed(ours))
            times[1].append(timed(update))
            times[2].append(host()[0])
        med = [statistics.median(t) for t in times]
        spread = [max(t) - min(t) for t in times]
        lines.append(f"{n:>4} x {m:<3}/ {K:<5} {groups:>6} | {med[0]:10.1f} {spread[0]:8.1f} | {med[1]:8.1f} {spread[1]:8.1f} | {med[2]:10.1f} "
                     f"{spread[2]:9.1f} | {med[2] / med[0]:16.1f}x | {med[2] / med[1]:12.1f}x | {verdict}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
