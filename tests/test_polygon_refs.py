"""Pins tests/polygon_refs.py, the rleFrPoly restatement that the device rasteriser is held to: literal run lengths, the equivalence of the C
code's sort / difference / merge with a prefix parity of toggled bits, and areas against the shoelace formula."""
import math

import numpy as np
import pytest

import polygon_refs as pr

# (h, w, polygon, column-major runs starting with the zeros)
LITERAL = [
    (6, 6, [1, 1, 4, 1, 4, 4, 1, 4], [7, 3, 3, 3, 3, 3, 14]),                       # the 3 x 3 block at rows / cols 1 .. 3
    (6, 6, [0.5, 0.5, 3.5, 0.5, 3.5, 3.5, 0.5, 3.5], [7, 3, 3, 3, 3, 3, 14]),
    (6, 6, [0, 0, 3, 0, 3, 3, 0, 3], [0, 3, 3, 3, 3, 3, 21]),
    (6, 6, [1, 1, 5, 1, 1, 5], [7, 3, 3, 2, 4, 1, 16]),
    (6, 6, [2, 0, 4, 6, 0, 6], [4, 2, 1, 5, 1, 5, 4, 2, 12]),
    (6, 6, [0, 0, 6, 6, 6, 0, 0, 6], [0, 5, 2, 3, 4, 1, 5, 1, 4, 3, 2, 5, 1]),      # a bow-tie
    (8, 8, [4, 4, 8, 4, 8, 8, 4, 8], [36, 4, 4, 4, 4, 4, 4, 4]),                    # records an index 64 = h * w
    (8, 8, [-5, -5, 20, -5, 20, 20, -5, 20], [0, 64]),
    (1, 1, [0, 0, 1, 0, 1, 1, 0, 1], [0, 1]),
]


@pytest.mark.parametrize("h,w,xy,runs", LITERAL)
def test_literal_runs(h, w, xy, runs):
    assert pr.poly_runs_ref(xy, h, w) == runs
    assert sum(runs) == h * w


def test_literal_block_is_the_block():
    m = pr.poly_mask_ref([1, 1, 4, 1, 4, 4, 1, 4], 6, 6)
    want = np.zeros((6, 6), dtype=np.uint8)
    want[1:4, 1:4] = 1
    assert np.array_equal(m, want)


def test_index_hw_is_recorded_and_harmless():
    assert 64 in pr.poly_crossings_ref([4, 4, 8, 4, 8, 8, 4, 8], 8, 8)
    m = pr.poly_mask_ref([4, 4, 8, 4, 8, 8, 4, 8], 8, 8)
    want = np.zeros((8, 8), dtype=np.uint8)
    want[4:, 4:] = 1
    assert np.array_equal(m, want)


def random_polygon(rng, h, w):
    """a mix of the families that matter: fractional and integer coordinates, vertices inside and outside the image"""
    k = int(rng.integers(3, 9))
    kind = int(rng.integers(0, 4))
    span = 0.3 if kind < 2 else 0.0                           # how far outside the image, as a share of its size
    x = rng.uniform(-span * w, (1 + span) * w, k)
    y = rng.uniform(-span * h, (1 + span) * h, k)
    if kind % 2 == 0:
        x, y = np.round(x), np.round(y)
    else:
        x, y = np.round(x, 2), np.round(y, 2)
    return np.stack([x, y], 1).reshape(-1).tolist()


def test_parity_equals_sort_diff_merge():
    rng = np.random.default_rng(20240607)
    spills = 0
    for i in range(1200):
        h, w = int(rng.integers(1, 24)), int(rng.integers(1, 24))
        xy = random_polygon(rng, h, w)
        spills += any(y == h for _, y in pr.poly_crossing_points_ref(xy, h, w))
        assert np.array_equal(pr.parity_mask_ref(xy, h, w), pr.poly_mask_ref(xy, h, w)), (i, h, w, xy)
    assert spills > 50                                        # the yd == h spill into the next column really occurs


def test_union_not_xor():
    a, b = [1, 1, 6, 1, 6, 6, 1, 6], [3, 3, 8, 3, 8, 8, 3, 8]
    ma, mb = pr.poly_mask_ref(a, 10, 10), pr.poly_mask_ref(b, 10, 10)
    assert (ma & mb).any()
    assert np.array_equal(pr.segm_mask_ref([a, b], 10, 10), ma | mb)
    assert np.array_equal(pr.segm_mask_ref([], 4, 5), np.zeros((4, 5), dtype=np.uint8))


def test_convex_area_close_to_shoelace():
    """|area - shoelace| <= 0.5 * perimeter + 1 for convex polygons inside the image: a boundary pixel is won or lost whole, and the
    boundary crosses about `perimeter` of them.  (The restatement stays within 0.13 * perimeter on such polygons; the bound is a
    condition with margin.)"""
    rng = np.random.default_rng(5)
    for _ in range(400):
        h, w = int(rng.integers(20, 60)), int(rng.integers(20, 60))
        k = int(rng.integers(3, 12))
        ang = np.sort(rng.uniform(0, 2 * math.pi, k))
        cx, cy = w / 2, h / 2
        rx, ry = rng.uniform(3, w / 2 - 1), rng.uniform(3, h / 2 - 1)
        x, y = np.round(cx + rx * np.cos(ang), 2), np.round(cy + ry * np.sin(ang), 2)
        shoelace = 0.5 * abs(float(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))))
        perimeter = float(np.hypot(x - np.roll(x, -1), y - np.roll(y, -1)).sum())
        area = int(pr.poly_mask_ref(np.stack([x, y], 1).reshape(-1).tolist(), h, w).sum())
        assert abs(area - shoelace) <= 0.5 * perimeter + 1, (area, shoelace, perimeter)
