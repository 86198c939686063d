"""Time ops.box_cover_overlaps -- the greedy coverage of ground-truth boxes by proposals for all 8 (area range, limit) combinations of an
image in ONE launch -- against the loop it replaces, restated with torch on the same device:
    (a) ops.box_cover_overlaps(proposals, gt)
    (b) torch: per combination the n_c x m_c IoU matrix, then min(n_c, m_c) rounds of max(dim=0), max, and two index writes -- the
        reference's `_evaluate_box_proposals` loop with nothing leaving the device (the columns of each area range are picked beforehand,
        outside the timed part; the reference picks them with a boolean index, which synchronises)
at n x m = 1000 x 20 and 1000 x 300: proposals that are jittered copies of the ground truth mixed with random boxes, in a 1333 x 800 image.
(a) is first compared for equality -- overlaps and matched rows -- with (b), and (b) with the same loop on the host.  Both routes are
timed as they are called, eagerly, with device events around one call and a synchronise before it: (b)'s time is mostly the launches
of its thousands of small kernels, which is what the route costs.  The routes are sampled in alternation; the median and the spread
(max - min over the samples) of each are printed.

    python tools/gpu_probe_boxcover.py [--out profiles/boxcover_timing.txt] [--samples 7]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def scene(n, m, seed):
    """(proposals [n, 4] in descending score order, gt [m, 4]) on the host: ground truth with sides 12 .. 400 in a 1333 x 800 image; two
    thirds of the proposals are ground-truth boxes jittered by up to a fifth of their size, the rest random boxes"""
    g = torch.Generator().manual_seed(seed)
    wh = 12 + 388 * torch.rand((m, 2), generator=g) ** 2
    xy = torch.rand((m, 2), generator=g) * (torch.tensor([1333.0, 800.0]) - wh)
    gt = torch.cat([xy, xy + wh], 1).float()
    src = gt[torch.randint(0, m, (n,), generator=g)]
    size = torch.cat([src[:, 2:] - src[:, :2]] * 2, 1)
    near = src + (torch.rand((n, 4), generator=g) - 0.5) * 0.4 * size
    rwh = 12 + 388 * torch.rand((n, 2), generator=g)
    rxy = torch.rand((n, 2), generator=g) * (torch.tensor([1333.0, 800.0]) - rwh).clamp_min(1)
    far = torch.cat([rxy, rxy + rwh], 1)
    pick = torch.rand(n, generator=g) < 2 / 3
    return torch.where(pick[:, None], near, far).float().contiguous(), gt.contiguous()


def iou_matrix(p, g):
    area_p = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    area_g = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    w = (torch.minimum(p[:, None, 2], g[None, :, 2]) - torch.maximum(p[:, None, 0], g[None, :, 0])).clamp_min(0)
    h = (torch.minimum(p[:, None, 3], g[None, :, 3]) - torch.maximum(p[:, None, 1], g[None, :, 1])).clamp_min(0)
    inter = w * h
    union = (area_p[:, None] + area_g[None, :]) - inter
    hit = inter > 0
    return torch.where(hit, inter / torch.where(hit, union, torch.ones_like(union)), torch.zeros_like(inter))


def torch_loop(p, g, columns, limits, ov, mt):
    """the loop, on whatever device p and g are on, without a synchronisation; columns[c] = the in-range ground truth of combination c
    (an index tensor), picked beforehand"""
    ov.fill_(-1.0)
    mt.fill_(-1)
    for c, (cols, limit) in enumerate(zip(columns, limits)):
        if cols.numel() == 0:
            continue
        ov[c, cols] = 0.0
        rows = p[:limit] if limit > 0 else p
        table = iou_matrix(rows, g[cols])
        for _ in range(min(table.shape)):
            best, best_row = table.max(dim=0)
            value, col = best.max(dim=0)
            row = best_row[col]
            ov[c, cols[col]] = value
            mt[c, cols[col]] = row.int()
            table[row, :] = -1
            table[:, col] = -1
    return ov, mt


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

    from ape_amd import ops

    ranges = [r for _ in ops.BOX_COVER_LIMITS for r in ops.BOX_COVER_RANGES]
    limits = [k for k in ops.BOX_COVER_LIMITS for _ in ops.BOX_COVER_RANGES]
    lines = [f"box_cover_overlaps (one launch, 8 combinations) against the torch loop on {torch.cuda.get_device_name(0)}; eager calls, device "
             f"events around one call; {args.samples} samples per route in alternation; microseconds per call",
             f"{'n x m':>11} {'rounds':>6} | {'box_cover':>10} {'spread':>8} | {'torch loop':>11} {'spread':>9} | loop / box_cover | equal"]
    ok = True
    for n, m in ((1000, 20), (1000, 300)):
        hp, hg = scene(n, m, 7 * m + 1)
        areas = (hg[:, 2] - hg[:, 0]) * (hg[:, 3] - hg[:, 1])
        hcols = [((areas >= torch.tensor(lo, dtype=torch.float32)) & (areas <= torch.tensor(hi, dtype=torch.float32))).nonzero().flatten()
                 for lo, hi in ranges]
        rounds = sum(min(n if k <= 0 else min(n, k), int(c.numel())) for c, k in zip(hcols, limits))
        p, g = hp.cuda(), hg.cuda()
        dcols = [c.cuda() for c in hcols]
        out, match = torch.empty((8, m), dtype=torch.float32, device="cuda"), torch.empty((8, m), dtype=torch.int32, device="cuda")
        tov, tmt = torch.empty_like(out), torch.empty_like(match)
        garea = areas.cuda()

        def ours():
            return ops.box_cover_overlaps(p, g, gt_areas=garea, out=out, match=match)

        def loop():
            return torch_loop(p, g, dcols, limits, tov, tmt)
        ours()
        loop()
        torch.cuda.synchronize()
        hov, hmt = torch_loop(hp, hg, hcols, limits, torch.empty((8, m)), torch.empty((8, m), dtype=torch.int32))
        same = torch.equal(out, tov) and torch.equal(match, tmt)
        host_same = torch.equal(out.cpu(), hov) and torch.equal(match.cpu(), hmt)
        verdict = "yes" if same and host_same else (f"NO: {int((out != tov).sum())} overlaps / {int((match != tmt).sum())} rows differ from the "
                                                     f"device loop, {int((out.cpu() != hov).sum())} / {int((match.cpu() != hmt).sum())} from the host loop")
        ok = ok and same and host_same
        times = [[], []]
        for _ in range(2):                                     # warm
            timed(ours)
            timed(loop)
        for _ in range(args.samples):
            times[0].append(timed(ours))
            times[1].append(timed(loop))
        med = [statistics.median(t) for t in times]
        spread = [max(t) - min(t) for t in times]
        lines.append(f"{n:>5} x {m:<3} {rounds:>6} | {med[0]:10.1f} {spread[0]:8.1f} | {med[1]:11.1f} {spread[1]:9.1f} | {med[1] / med[0]:15.1f}x | {verdict}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
