"""Time the polygon rasteriser on ONE COCO-shaped image -- 640 x 480, 20 objects of 1 .. 3 polygons with 30 .. 100 vertices each --
against what a user of this package does without it, uploading the same 20 masks rasterised on the host:
    (a) ops.poly_rasterize(xy, vert_offsets, poly_offsets, 480, 640)   the device time of its launches (toggle, fill, output), summed per call
                                                                       from the library's launch meter (the memset node is not a launch and
                                                                       not metered), and the whole call by device events, operands resident
    (b) segmentations_to_masks(polygons, 480, 640)                     what an evaluation pays per image: packing on the host, three small
                                                                       uploads, (a); host clock around the call and a synchronise
    (c) masks.to("cuda")                                               the upload of the 20 host-rasterised byte masks [20, 480, 640]
                                                                       (pageable memory, as a dataset loader hands them over); host clock
                                                                       around the copy and a synchronise.  The host rasterisation itself
                                                                       (pycocotools in the reference) is NOT in (c).
(a) is first compared for equality with the rleFrPoly restatement of tests/polygon_refs.py.  Two warm calls, then the routes are sampled in
alternation; the median and the spread (max - min over the samples) of each are printed.  There is no threshold: the cost is recorded.

    python tools/gpu_probe_polygon.py [--out profiles/polygon_timing.txt] [--samples 15]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scene(H, W, n, seed):
    """n objects, each 1 .. 3 star-shaped polygons of 30 .. 100 vertices with two decimals, some reaching over the image edge"""
    rng = np.random.default_rng(seed)
    objs = []
    for _ in range(n):
        polys = []
        for _ in range(int(rng.integers(1, 4))):
            k = int(rng.integers(30, 101))
            cx, cy = rng.uniform(0, W), rng.uniform(0, H)
            r = rng.uniform(15, 120)
            ang = np.sort(rng.uniform(0, 2 * np.pi, k))
            rad = r * (0.75 + 0.25 * np.sin(rng.integers(2, 7) * ang + rng.uniform(0, 6))) + rng.uniform(-2, 2, k)
            polys.append(np.round(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1), 2).reshape(-1).tolist())
        objs.append(polys)
    return objs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples", type=int, default=15)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"

    import polygon_refs
    from ape_amd import _lib, build, evaluation, ops

    H, W, n = 480, 640, 20
    objs = scene(H, W, n, 7)
    want = torch.from_numpy(np.stack([polygon_refs.segm_mask_ref(p, H, W) for p in objs]))
    xy, vo, po = [t.cuda() for t in evaluation.pack_polygons(objs)]
    out = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
    lib = _lib.load()

    def kernels():
        """microseconds: (sum of the call's metered launches, the call by device events)"""
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        lib.ape_hip_meter_begin()
        start.record()
        ops.poly_rasterize(xy, vo, po, H, W, out=out)
        stop.record()
        stop.synchronize()
        cnt = lib.ape_hip_meter_end()
        ms, name = ctypes.c_float(), ctypes.c_char_p()
        parts = {}
        for i in range(cnt):
            lib.ape_hip_meter_read(i, ctypes.byref(name), ctypes.byref(ms))
            parts[name.value.decode()] = parts.get(name.value.decode(), 0.0) + ms.value * 1e3
        return sum(parts.values()), start.elapsed_time(stop) * 1e3, parts

    def end_to_end():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        evaluation.segmentations_to_masks(objs, H, W, device="cuda")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    def upload():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want.to("cuda")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    masks, area = ops.poly_rasterize(xy, vo, po, H, W)
    same = torch.equal(masks.cpu(), want) and torch.equal(area.cpu(), want.flatten(1).sum(1))
    for _ in range(2):                                         # warm
        kernels()
        end_to_end()
        upload()
    t = [[], [], [], []]
    parts = {}
    for _ in range(args.samples):
        k, call, parts = kernels()
        t[0].append(k)
        t[1].append(call)
        t[2].append(end_to_end())
        t[3].append(upload())
    med = [statistics.median(v) for v in t]
    spread = [max(v) - min(v) for v in t]
    stamp = os.path.join(os.path.dirname(build.LIB), "libape_hip.sha256")
    digest = open(stamp).read().strip() if os.path.exists(stamp) else "unknown"
    lines = [f"poly_rasterize on {torch.cuda.get_device_name(0)}: one {W} x {H} image, {n} objects, {vo.numel() - 1} polygons, {xy.shape[0]} vertices, "
             f"{int(want.sum())} foreground pixels; {args.samples} samples per route in alternation after 2 warm calls; microseconds per image",
             f"library digest {digest}",
             f"equal to the rleFrPoly restatement (masks and areas): {'yes' if same else 'NO'}",
             f"{'route':<58} {'median':>10} {'spread':>10}",
             f"{'(a) poly_rasterize, metered launches summed':<58} {med[0]:10.1f} {spread[0]:10.1f}",
             f"{'(a) poly_rasterize, device events around the call':<58} {med[1]:10.1f} {spread[1]:10.1f}",
             f"{'(b) segmentations_to_masks, host clock + synchronise':<58} {med[2]:10.1f} {spread[2]:10.1f}",
             f"{'(c) upload of the 20 host-rasterised byte masks':<58} {med[3]:10.1f} {spread[3]:10.1f}",
             "last sample's launches: " + ", ".join(f"{k} {v:.1f}" for k, v in parts.items())]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
