"""cocoapi maskApi.c rleFrPoly restated in Python, statement for statement: the 5x boundary walk, the crossings, then SORT, DIFFERENCE and
MERGE of empty runs -- the C code's own form, so that it shares nothing with the device's formulation (a bit toggled per crossing and a
prefix parity).  Python floats are IEEE doubles and `int()` truncates toward zero like the C cast; every expression keeps the C code's
order of operations.  An object (`segm_mask_ref`) is the union of its polygons, pycocotools' frPyObjects + merge = annToRLE."""
import math

import numpy as np


def poly_points_ref(xy):
    """the walk: (u, v) lists of every boundary point on the 5x grid, all edges in order"""
    k = len(xy) // 2
    x = [int(5 * xy[2 * j] + .5) for j in range(k)]
    y = [int(5 * xy[2 * j + 1] + .5) for j in range(k)]
    x.append(x[0])
    y.append(y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe = xe, xs
            ys, ye = ye, ys
        if dx == 0 and dy == 0:                               # C: s = 0 / 0, one point whose v nobody reads (both neighbours share its u)
            u.append(xs)
            v.append(ys)
            continue
        s = float(ye - ys) / dx if dx >= dy else float(xe - xs) / dy
        if dx >= dy:
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(int(ys + s * t + .5))
        else:
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + .5))
    return u, v


def poly_crossing_points_ref(xy, h, w):
    """the recorded (x, y) pairs in walking order; y runs from 0 to h INCLUSIVE"""
    u, v = poly_points_ref(xy)
    a = []
    for j in range(1, len(u)):
        if u[j] != u[j - 1]:
            xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
            xd = (xd + .5) / 5 - .5
            if math.floor(xd) != xd or xd < 0 or xd > w - 1:
                continue
            yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
            yd = (yd + .5) / 5 - .5
            if yd < 0:
                yd = 0.0
            elif yd > h:
                yd = float(h)
            yd = math.ceil(yd)
            a.append((int(xd), int(yd)))
    return a


def poly_crossings_ref(xy, h, w):
    """the recorded column-major indices a = x * h + y, in walking order: y == h spills into the next column, in the last column to h * w"""
    return [x * h + y for x, y in poly_crossing_points_ref(xy, h, w)]


def poly_runs_ref(xy, h, w):
    """column-major run lengths starting with the zeros, what rleFrPoly leaves in R->cnts"""
    a = poly_crossings_ref(xy, h, w)
    a.append(h * w)
    a.sort()
    p = 0
    for j in range(len(a)):
        t = a[j]
        a[j] -= p
        p = t
    k = len(a)
    b = [a[0]]
    j = 1
    while j < k:
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < k:
                b[-1] += a[j]
                j += 1
    return b


def runs_to_mask(runs, h, w):
    """rleDecode: uint8 [h, w] of 0 / 1 from column-major runs"""
    flat = np.zeros(h * w, dtype=np.uint8)
    pos, val = 0, 0
    for r in runs:
        if val:
            flat[pos: pos + r] = 1
        pos += r
        val ^= 1
    assert pos == h * w, (pos, h, w)
    return np.ascontiguousarray(flat.reshape(w, h).T)


def poly_mask_ref(xy, h, w):
    return runs_to_mask(poly_runs_ref(xy, h, w), h, w)


def segm_mask_ref(polys, h, w):
    """one object: the union of its polygons' masks (an object without polygons is empty)"""
    m = np.zeros((h, w), dtype=np.uint8)
    for xy in polys:
        m |= poly_mask_ref(xy, h, w)
    return m


def parity_mask_ref(xy, h, w):
    """the device's formulation on the host: toggle bit a per crossing (a = h * w dropped), then the prefix parity"""
    t = np.zeros(h * w, dtype=np.uint8)
    for a in poly_crossings_ref(xy, h, w):
        if a < h * w:
            t[a] ^= 1
    return np.ascontiguousarray((np.cumsum(t) & 1).astype(np.uint8).reshape(w, h).T)
