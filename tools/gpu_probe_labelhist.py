"""Time ops.label_pair_hist against the torch formulation of the same histogram on the same device:
    torch.bincount(a.long() * nb + b.long(), minlength=na * nb)
One call at n = 1536 * 1536, int16 x uint8, on the 134 x 134 (LDS path) and 460 x 460 (global path) tables, for a coherent map
(constant 37 x 53 blocks) and a uniformly random one.  The two routes alternate inside one process; a sample is the device-event
time of `--calls` back-to-back calls divided by their number; per case the median and the spread (max - min over the samples) of
each route are printed, and whether the new call stays within the torch route's median + spread.  The results are compared for
equality at the timed size first.

    python tools/gpu_probe_labelhist.py [--out FILE] [--samples 15] [--calls 20]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def maps(kind, na, nb, H=1536, W=1536):
    if kind == "coherent":
        by, bx = torch.arange(H)[:, None] // 37, torch.arange(W)[None, :] // 53
        blk = by * ((W + 52) // 53) + bx
        return (blk * 7 % na).to(torch.int16).cuda(), (blk * 11 % min(nb, 256)).to(torch.uint8).cuda()
    g = torch.Generator().manual_seed(0)
    return (torch.randint(0, na, (H, W), generator=g).to(torch.int16).cuda(),
            torch.randint(0, min(nb, 256), (H, W), generator=g).to(torch.uint8).cuda())


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
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from ape_amd import ops

    lines = [f"label_pair_hist vs torch.bincount(a.long() * nb + b.long()) on {torch.cuda.get_device_name(0)}; n = 1536 * 1536, int16 x uint8; "
             f"{args.samples} alternating samples of {args.calls} calls each, microseconds per call (device events); "
             f"LDS path up to {ops.label_hist_lds_bins()} bins",
             f"{'table':>9} {'map':>9} | {'hip median':>10} {'hip spread':>10} | {'torch median':>12} {'torch spread':>12} | within torch median + spread"]
    for na, nb in ((134, 134), (460, 460)):
        for kind in ("coherent", "random"):
            a, b = maps(kind, na, nb)
            out = torch.zeros((na, nb), dtype=torch.int64, device="cuda")
            rejected = torch.zeros((1,), dtype=torch.int64, device="cuda")

            def hip():
                ops.label_pair_hist(a, b, na, nb, out=out, rejected=rejected)

            def ref():
                return torch.bincount(a.long().reshape(-1) * nb + b.long().reshape(-1), minlength=na * nb)
            hip()
            want = ref().reshape(na, nb)
            assert torch.equal(out, want) and int(rejected) == 0, "the two routes disagree"
            for _ in range(3):                               # warm both routes at this shape
                sample(hip, args.calls)
                sample(ref, args.calls)
            th, tr = [], []
            for _ in range(args.samples):
                th.append(sample(hip, args.calls))
                tr.append(sample(ref, args.calls))
            mh, mr = statistics.median(th), statistics.median(tr)
            sh, sr = max(th) - min(th), max(tr) - min(tr)
            lines.append(f"{na:>4}x{nb:<4} {kind:>9} | {mh:10.1f} {sh:10.1f} | {mr:12.1f} {sr:12.1f} | {'yes' if mh <= mr + sr else 'NO'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
