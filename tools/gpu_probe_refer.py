"""Time ops.mask_paired_counts -- the (|a & b|, |a|, |b|) of n PAIRS of byte masks in one pass -- against the two routes to the same three
numbers that exist without it, on the same device:
    (a) ops.mask_paired_counts(a, b)
    (b) ops.mask_pair_iou(a, b) with the diagonal taken: two bit packs and all n x n intersections
    (c) torch: (a & b).flatten(1).sum(1), a.flatten(1).sum(1), b.flatten(1).sum(1)                 (masks of 0 / 1)
at 1 x 480 x 640, 1 x 1024^2 and 64 x 1024^2, uint8 ellipses as detections are.  (a) is first compared for equality with host integer
arithmetic at every size.  Each route is captured into a graph of `--calls` back-to-back calls, so a sample -- the device-event time of
one replay divided by the calls -- holds no host enqueue time; the routes are sampled in alternation, and the median and the spread
(max - min over the samples) of each are printed.  The roof of (a) is the 2 n H W bytes of the masks read once, at the 6.3 TB/s a
streaming read reaches on this device; sizes that fit the 256 MiB Infinity Cache are served from it on repeated calls (as a mask that
the model has just written is), so the largest size rotates over three sets of masks, 403 MB, and reads from memory.

    python tools/gpu_probe_refer.py [--out profiles/refer_timing.txt] [--samples 11] [--calls 10]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAM_TBS = 6.3                                               # measured streaming-read rate of the MI355X, TB/s


def blobs(n, H, W, seed):
    """n masks [H, W] uint8 of 0 / 1 on the device: an ellipse each, a few percent to a quarter of the image"""
    g = torch.Generator().manual_seed(seed)
    cy, cx = (0.3 + 0.4 * torch.rand(n, generator=g)) * H, (0.3 + 0.4 * torch.rand(n, generator=g)) * W
    ry, rx = (0.1 + 0.2 * torch.rand(n, generator=g)) * H, (0.1 + 0.2 * torch.rand(n, generator=g)) * W
    y = torch.arange(H, device="cuda", dtype=torch.float32)[None, :, None]
    x = torch.arange(W, device="cuda", dtype=torch.float32)[None, None, :]
    cy, cx, ry, rx = (t.cuda()[:, None, None] for t in (cy, cx, ry, rx))
    return ((((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2) <= 1.0).to(torch.uint8)


def graph_of(fn, sets, calls):
    """a graph of `calls` back-to-back calls of fn, call k on set k % len(sets)"""
    for a, b in sets:                                          # warm every set: nothing is set up lazily inside the capture
        fn(a, b)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    keep = []
    with torch.cuda.graph(graph):
        for k in range(calls):
            keep.append(fn(*sets[k % len(sets)]))
    torch.cuda.synchronize()
    return graph, keep


def sample(graph, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    graph.replay()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls              # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples", type=int, default=11)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"

    from ape_amd import ops

    def paired(a, b):
        return ops.mask_paired_counts(a, b)

    def matrix(a, b):
        iou, inter, area_a, area_b = ops.mask_pair_iou(a, b)
        return inter.diagonal(), area_a, area_b

    def tensor_library(a, b):
        return (a & b).flatten(1).sum(1), a.flatten(1).sum(1), b.flatten(1).sum(1)

    lines = [f"mask_paired_counts against mask_pair_iou's diagonal and torch's (a & b).sum on {torch.cuda.get_device_name(0)}; uint8 masks; "
             f"{args.samples} samples of one replay of a graph of {args.calls} calls each, routes in alternation; microseconds per call "
             f"(device events); roof = 2 n H W bytes at {STREAM_TBS} TB/s",
             f"{'case':>16} {'sets':>4} {'MB':>7} {'roof':>7} | {'paired':>8} {'spread':>7} {'TB/s':>6} | {'pair_iou diag':>13} {'spread':>7} | "
             f"{'torch':>8} {'spread':>7} | diag / paired  torch / paired"]
    for n, H, W, nsets in ((1, 480, 640, 1), (1, 1024, 1024, 1), (64, 1024, 1024, 3)):
        sets = [(blobs(n, H, W, 10 * s + 1), blobs(n, H, W, 10 * s + 2)) for s in range(nsets)]
        for a, b in sets:                                      # equality with host integer arithmetic first
            ha, hb = a.cpu().flatten(1) != 0, b.cpu().flatten(1) != 0
            want = torch.stack([(ha & hb).long().sum(1), ha.long().sum(1), hb.long().sum(1)], 1)
            assert torch.equal(paired(a, b).cpu(), want), f"mask_paired_counts differs from host integer arithmetic at {n} x {H} x {W}"
            assert torch.equal(torch.stack(matrix(a, b), 1).cpu(), want) and torch.equal(torch.stack(tensor_library(a, b), 1).cpu(), want)
        routes = [graph_of(fn, sets, args.calls) for fn in (paired, matrix, tensor_library)]
        times = [[] for _ in routes]
        for _ in range(2):                                     # warm the replays
            for graph, _ in routes:
                sample(graph, args.calls)
        for _ in range(args.samples):
            for t, (graph, _) in zip(times, routes):
                t.append(sample(graph, args.calls))
        med = [statistics.median(t) for t in times]
        spread = [max(t) - min(t) for t in times]
        nbytes = 2 * n * H * W
        lines.append(f"{n:>3} x {H:>4} x {W:<4} {nsets:>4} {nbytes / 1e6:7.1f} {nbytes / (STREAM_TBS * 1e6):7.2f} | {med[0]:8.2f} {spread[0]:7.2f} "
                     f"{nbytes / med[0] / 1e6:6.2f} | {med[1]:13.2f} {spread[1]:7.2f} | {med[2]:8.2f} {spread[2]:7.2f} | "
                     f"{med[1] / med[0]:12.1f}x {med[2] / med[0]:14.1f}x")
        del routes, sets
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
