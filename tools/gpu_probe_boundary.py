"""Time ops.boundary_pair_iou against the torch formulation of the same matrices on the same device:
    eroded = 1 - max_pool2d(F.pad(1 - x, (d, d, d, d), value=1), 2 * d + 1, stride=1)        (x: the masks as float [n, 1, H, W])
    band = x * (1 - eroded);   counts = band_a.flatten(1).float() @ band_b.flatten(1).float().T   (and the same for the masks)
at 100 x 100 masks of 1024^2 (d = 29) and of 1536^2 (d = 43), uint8 ellipses of a few percent of the image, as detections are.  A sample
is the device-event time of `--calls` back-to-back calls divided by their number; per case the median and the spread (max - min over the
samples) of each route are printed, next to the stages of the new route (row packs, boundaries, the two pair counts).  The torch route
is slow, so it gets `--ref-samples` samples of one call.  The band and mask intersections of the two routes are compared for equality
at the timed size first.

    python tools/gpu_probe_boundary.py [--out profiles/boundary_timing.txt] [--samples 11] [--calls 5] [--ref-samples 3]
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
    ap.add_argument("--ref-samples", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    import torch.nn.functional as F

    from ape_amd import ops

    lines = [f"boundary_pair_iou vs the torch formulation (max_pool2d erosion, float matmul counts) on {torch.cuda.get_device_name(0)}; uint8 masks; "
             f"hip: {args.samples} samples of {args.calls} calls, torch: {args.ref_samples} samples of 1 call; microseconds per call (device events)",
             f"{'case':>20} | {'hip median':>10} {'hip spread':>10} | {'packs':>8} {'bands':>8} {'counts':>8} | {'torch median':>12} {'torch spread':>12} | "
             f"torch / hip"]
    for n, m, S in ((100, 100, 1024), (100, 100, 1536)):
        a, b = blobs(n, S, 1), blobs(m, S, 2)
        d = ops.boundary_dilation(S, S)

        def hip():
            return ops.boundary_pair_iou(a, b, dilation=d)

        def band(x):
            x = x[:, None].float()
            eroded = 1 - F.max_pool2d(F.pad(1 - x, (d, d, d, d), value=1.0), 2 * d + 1, stride=1)
            return (x * (1 - eroded)).flatten(1), x.flatten(1)

        def ref():
            ba, fa = band(a)
            bb, fb = band(b)
            return ba @ bb.T, fa @ fb.T, ba.sum(1), bb.sum(1)

        biou, iou, binter, inter, barea_a, barea_b, area_a, area_b = hip()
        torch_note = None
        try:
            want_b, want_i, wa, wb = ref()                   # exact in fp32 here: every count is far below 2^24
            assert torch.equal(binter, want_b.long()) and torch.equal(inter, want_i.long()), "the two routes disagree"
            assert torch.equal(barea_a, wa.long()) and torch.equal(barea_b, wb.long()), "the two routes disagree on the band areas"
            del want_b, want_i, wa, wb
        except (RuntimeError, torch.cuda.OutOfMemoryError) as e:          # e.g. no pooling kernel for a window this large
            torch_note = f"torch formulation failed: {str(e).splitlines()[0][:120]}"
        assert int(binter.max()) < 2 ** 24 and int((binter > 0).sum()) > 0
        a_bits, _ = ops.mask_pack_rows(a)
        b_bits, _ = ops.mask_pack_rows(b)
        a_band, _ = ops.bitmask_boundary(a_bits, S, S, d)
        b_band, _ = ops.bitmask_boundary(b_bits, S, S, d)
        out = torch.empty((n, m), dtype=torch.int64, device="cuda")

        def packs():
            ops.mask_pack_rows(a)
            ops.mask_pack_rows(b)

        def bands():
            ops.bitmask_boundary(a_bits, S, S, d)
            ops.bitmask_boundary(b_bits, S, S, d)

        def counts():
            ops.bitmask_pair_counts(a_bits, b_bits, out=out)
            ops.bitmask_pair_counts(a_band, b_band, out=out)
        for _ in range(2):                                   # warm every route at this shape
            for fn in (hip, packs, bands, counts):
                sample(fn, args.calls)
        th, tp, tb, tc, tr = [], [], [], [], []
        for _ in range(args.samples):
            th.append(sample(hip, args.calls))
            tp.append(sample(packs, args.calls))
            tb.append(sample(bands, args.calls))
            tc.append(sample(counts, args.calls))
        if torch_note is None:
            for _ in range(args.ref_samples):
                tr.append(sample(ref, 1))
        mh, sh = statistics.median(th), max(th) - min(th)
        head = (f"{n:>4}x{m:<3} {S:>4}^2 d={d:<3} | {mh:10.1f} {sh:10.1f} | {statistics.median(tp):8.1f} {statistics.median(tb):8.1f} "
                f"{statistics.median(tc):8.1f} | ")
        if tr:
            mr, sr = statistics.median(tr), max(tr) - min(tr)
            lines.append(head + f"{mr:12.1f} {sr:12.1f} | {mr / mh:8.1f}x")
        else:
            lines.append(head + torch_note)
        del a, b, a_bits, b_bits, a_band, b_band
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
