"""Boundary IoU / Boundary AP without a GPU: the host rule for the band width, the three new entry points of csrc/boundary.hip (declared,
exported, bound, and their argument checks, which run before any HIP call), the tile planner (a host function), and the accumulator's
record shape on empty inputs."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ape_hip_mask_pack_rows", "ape_hip_bitmask_boundary", "ape_hip_bitmask_unpack_rows")


@pytest.mark.parametrize("hw,want", [((1024, 1024), 29), ((1536, 1536), 43), ((10, 10), 1), ((75, 100), 2), ((480, 640), 16)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_boundary_dilation(hw, want):
    """2 % of the diagonal with Python's round: 0.28 rounds to 0 and is clamped to 1; (75, 100) is exactly 2.5, half to even"""
    from ape_amd import ops
    assert ops.boundary_dilation(*hw) == want
    assert isinstance(ops.boundary_dilation(*hw), int)


def test_boundary_dilation_ratio_and_errors():
    from ape_amd import ops
    assert ops.boundary_dilation(300, 400, ratio=0.01) == 5 and ops.boundary_dilation(300, 400, 0.001) == 1
    with pytest.raises(ValueError):
        ops.boundary_dilation(0, 10)


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "ape_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(ape_hip_\w+)\s*\(", text))


def test_new_symbols_are_declared_exported_and_bound():
    from ape_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    declared = _header_symbols()
    for name in NEW + ("ape_hip_bitmask_boundary_tile",):
        assert name in declared and name in _lib.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and tuple(fn.argtypes) == tuple(_lib.SIGNATURES[name][1])
    assert lib.ape_hip_abi_version() == 5


def test_argument_errors_are_reported_without_a_gpu():
    from ape_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    one = ctypes.c_void_p(64)            # never dereferenced: every call below is refused, or has nothing to do, before any HIP call
    err = lib.ape_hip_last_error

    f = lib.ape_hip_mask_pack_rows       # (masks, n, H, W, bits, ldb, area, stream)
    assert f(None, 1, 4, 65, one, 8, one, None) != 0 and b"null" in err()
    assert f(one, 1, 4, 65, None, 8, one, None) != 0 and b"null" in err()
    assert f(one, 1, 4, 65, one, 8, None, None) != 0 and b"null" in err()
    assert f(one, -1, 4, 65, one, 8, one, None) != 0 and b"negative" in err()
    assert f(one, 1, 0, 65, one, 8, one, None) != 0 and b"at least 1" in err()
    assert f(one, 1, 4, 0, one, 8, one, None) != 0 and b"at least 1" in err()
    assert f(one, 1, 4, 65, one, 7, one, None) != 0 and b"ldb" in err()              # 4 rows of 65 pixels are 4 x 2 words
    assert f(one, 1, 1 << 30, 1 << 30, one, 1 << 40, one, None) != 0 and b"too large" in err()
    assert f(None, 0, 4, 65, None, 8, None, None) == 0                                 # n == 0: a successful no-op

    f = lib.ape_hip_bitmask_boundary     # (bits, n, H, W, d, ldb, bbits, ldo, barea, stream)
    two = ctypes.c_void_p(4096)
    assert f(one, 1, 4, 65, 0, 8, two, 8, one, None) != 0 and b"d = 0" in err()
    assert f(one, 1, 4, 65, -3, 8, two, 8, one, None) != 0 and b"d = -3" in err()
    assert f(one, 1, 0, 65, 1, 8, two, 8, one, None) != 0 and b"at least 1" in err()
    assert f(one, 1, 4, 0, 1, 8, two, 8, one, None) != 0 and b"at least 1" in err()
    assert f(None, 1, 4, 65, 1, 8, two, 8, one, None) != 0 and b"null" in err()
    assert f(one, 1, 4, 65, 1, 8, None, 8, one, None) != 0 and b"null" in err()
    assert f(one, 1, 4, 65, 1, 8, two, 8, None, None) != 0 and b"null" in err()
    assert f(one, 1, 4, 65, 1, 7, two, 8, one, None) != 0 and b"ldb" in err()
    assert f(one, 1, 4, 65, 1, 8, two, 7, one, None) != 0 and b"ldo" in err()
    assert f(one, 1, 4, 65, 1, 8, one, 8, one, None) != 0 and b"in place" in err()
    assert f(one, -1, 4, 65, 1, 8, two, 8, one, None) != 0 and b"negative" in err()
    assert f(None, 0, 4, 65, 1, 8, None, 8, None, None) == 0

    f = lib.ape_hip_bitmask_unpack_rows  # (bits, n, H, W, ldb, masks, stream)
    assert f(None, 1, 4, 65, 8, one, None) != 0 and b"null" in err()
    assert f(one, 1, 4, 65, 8, None, None) != 0 and b"null" in err()
    assert f(one, 1, 0, 65, 8, one, None) != 0 and b"at least 1" in err()
    assert f(one, 1, 4, 65, 7, one, None) != 0 and b"ldb" in err()
    assert f(one, -1, 4, 65, 8, one, None) != 0 and b"negative" in err()
    assert f(None, 0, 4, 65, 8, None, None) == 0


def _tile(H, W, d, limit):
    from ape_amd import _lib
    rows, words = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _lib.load().ape_hip_bitmask_boundary_tile(H, W, d, limit, ctypes.byref(rows), ctypes.byref(words))
    return rc, rows.value, words.value


def test_tile_plan_fits_the_lds_limit_it_is_given():
    """the planner is a host function: for every limit the tile's two buffers of (rows + 2 d) x words 8-byte words fit, a tile never
    exceeds the image, and a band that is the whole mask needs no tile"""
    from ape_amd import build
    build.build(verbose=False)
    for limit in (16 * 1024, 64 * 1024, 160 * 1024):
        for (H, W, d) in ((1024, 1024, 29), (1536, 1536, 43), (700, 65, 3), (9, 4200, 3), (400, 4200, 66), (200, 200, 70), (5, 130, 2)):
            rc, rows, words = _tile(H, W, d, limit)
            assert rc == (rows + 2 * d) * words * 16 and 0 < rc <= limit, (limit, H, W, d, rc)
            assert 1 <= rows <= H and 1 <= words <= (W + 63) // 64
    assert _tile(1024, 1024, 29, 64 * 1024)[1:] == (116, 16)          # 4 d rows, the whole row of 16 words: 174 x 16 x 16 bytes
    assert _tile(1536, 1536, 43, 64 * 1024)[1:] == (170, 12)          # the row of 24 words is split in two
    assert _tile(70, 200, 63, 64 * 1024) == (0, 0, 0)                  # 2 d + 1 > H: the band is the mask
    assert _tile(4096, 4096, 2047, 64 * 1024)[0] > 0                   # one output row: 4095 staged rows of one word, twice
    assert _tile(4097, 4097, 2048, 64 * 1024)[0] < 0                   # does not fit
    lib_err = _tile(0, 5, 1, 1024)
    assert lib_err[0] < 0


def test_accumulator_on_empty_inputs_has_the_record_shape_of_mask_ap():
    """no detection or no ground truth: the [n, m] matrix is empty and nothing reaches the device (there is none here)"""
    from ape_amd.evaluation import BoundaryAPAccumulator, MaskAPAccumulator, boundary_ap
    some = torch.ones((2, 8, 8), dtype=torch.uint8)
    none = torch.zeros((0, 8, 8), dtype=torch.uint8)
    cases = [((none, torch.zeros(0), torch.zeros(0, dtype=torch.long)), (some, torch.tensor([1, 2]))),
             ((some, torch.tensor([0.9, 0.8]), torch.tensor([1, 2])), (none, torch.zeros(0, dtype=torch.long))),
             (([], [], []), ([], []))]
    for cls in (MaskAPAccumulator, BoundaryAPAccumulator):
        acc = cls()
        for (dm, ds, dc), (gm, gc) in cases:
            acc.update(dm, ds, dc, gm, gc)
        shapes = [tuple(r[3].shape) for r in acc.records]
        assert shapes == [(0, 2), (2, 0), (0, 0)] and all(r[3].dtype == torch.float64 and not r[3].is_cuda for r in acc.records)
        res = acc.compute()
        assert set(res) == {"AP", "AP50", "AP75", "classes", "gt", "dets"} and res["gt"] == 2 and res["dets"] == 2 and res["AP"] == 0.0
    assert issubclass(BoundaryAPAccumulator, MaskAPAccumulator) and BoundaryAPAccumulator(dilation_ratio=0.05).dilation_ratio == 0.05
    r = boundary_ap([cases[0][0]], [cases[0][1]])
    assert r["AP"] == 0.0 and r["gt"] == 2 and r["dets"] == 0
