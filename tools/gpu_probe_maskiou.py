"""Time ops.mask_pair_iou against the torch formulation of the same matrix on the same device:
    a.flatten(1).float() @ b.flatten(1).float().T      (and .sum(1) of each side for the areas)
at 100 x 20 masks of 1024^2 and 300 x 60 masks of 1536^2 (uint8, blobs of a few percent of the image, as detections are).  The two
routes alternate inside one process; a sample is the device-event time of `--calls` back-to-back calls divided by their number; per
case the median and the spread (max - min over the samples) of each route are printed, next to the two stages of the new route (the
bit packs of both sides, the pair counts on the packed words).  The results are compared for equality at the timed size first.

    python tools/gpu_probe_maskiou.py [--out FILE] [--samples 11] [--calls 5]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def blobs(n, S, seed):
    """n masks [S, S] uint8 on the device: an ellipse each, 1 - 12 % of the image, centres spread so that many pairs overlap"""
    g = torch.Generator().manual_seed(seed)
    cy, cx = torch.rand(n, generator=g) * S, torch.rand(n, generator=g) * S
    ry, rx = (0.06 + 0.14 * torch.rand(n, generator=g)) * S, (0.06 + 0.14 * torch.rand(n, generator=g)) * S
    y = torch.arange(S, device="cuda", dtype=torch.float32)[None, :, None]
    x = torch.arange(S, device="cuda", dtype=torch.float32)[None, None, :]
    cy, cx, ry, rx = (t.cuda()[:, None, None] for t in (cy, cx, ry, rx))
    return ((((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2) <= 1.0).to(torch.uint8)


def sample(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls          # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples", type=int, default=11)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from ape_amd import ops

    lines = [f"mask_pair_iou vs a.flatten(1).float() @ b.flatten(1).float().T on {torch.cuda.get_device_name(0)}; uint8 masks; "
             f"{args.samples} alternating samples of {args.calls} calls each, microseconds per call (device events)",
             f"{'case':>18} | {'hip median':>10} {'hip spread':>10} | {'pack':>9} {'counts':>9} | {'torch median':>12} {'torch spread':>12} | "
             f"within torch median + spread"]
    for n, m, S in ((100, 20, 1024), (300, 60, 1536)):
        a, b = blobs(n, S, 1), blobs(m, S, 2)

        def hip():
            return ops.mask_pair_iou(a, b)

        def ref():
            fa, fb = a.flatten(1).float(), b.flatten(1).float()
            return fa @ fb.T, fa.sum(1), fb.sum(1)

        iou, inter, area_a, area_b = hip()
        want, wa, wb = ref()                                 # exact in fp32 here: every count is far below 2^24
        assert torch.equal(inter, want.long()) and torch.equal(area_a, wa.long()) and torch.equal(area_b, wb.long()), "the two routes disagree"
        assert int(inter.max()) < 2 ** 24 and int((inter > 0).sum()) > 0
        a_bits, _ = ops.mask_pack_bits(a)
        b_bits, _ = ops.mask_pack_bits(b)
        out = torch.empty((n, m), dtype=torch.int64, device="cuda")

        def pack():
            ops.mask_pack_bits(a)
            ops.mask_pack_bits(b)

        def counts():
            ops.bitmask_pair_counts(a_bits, b_bits, out=out)
        for _ in range(2):                                   # warm every route at this shape
            for fn in (hip, ref, pack, counts):
                sample(fn, args.calls)
        th, tr, tp, tc = [], [], [], []
        for _ in range(args.samples):
            th.append(sample(hip, args.calls))
            tr.append(sample(ref, args.calls))
            tp.append(sample(pack, args.calls))
            tc.append(sample(counts, args.calls))
        mh, mr = statistics.median(th), statistics.median(tr)
        sh, sr = max(th) - min(th), max(tr) - min(tr)
        lines.append(f"{n:>4}x{m:<3} of {S:>4}^2 | {mh:10.1f} {sh:10.1f} | {statistics.median(tp):9.1f} {statistics.median(tc):9.1f} | "
                     f"{mr:12.1f} {sr:12.1f} | {'yes' if mh <= mr + sr else 'NO'}")
        del a, b, a_bits, b_bits
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
