"""Referring-expression scores without a GPU: `referring_metrics` on a hand-made table and against the reference's definition restated
on CPU tensors, the argument checks of `ape_hip_mask_paired_counts` (which run before any HIP call), the wrapper's refusal of host
tensors, and `ReferringAccumulator.reduce` without a process group."""
import ctypes

import pytest
import torch

KS = (5, 6, 7, 8, 9)


def test_metrics_on_a_hand_made_table():
    from ape_amd.evaluation import referring_metrics
    # (inter, area_pred, area_gt): IoU 50 / 100, 90 / 100, and empty against empty (the reference's convention: 1)
    counts = torch.tensor([[50, 100, 50], [90, 100, 90], [0, 0, 0]], dtype=torch.int64)
    # box IoUs of exactly 0.5, 0.9 and 1.0 in float64: 50 / 100, 90 / 100, 100 / 100
    boxes = torch.tensor([[0, 0, 10, 10, 0, 0, 10, 5], [0, 0, 10, 10, 0, 0, 10, 9], [2, 3, 12, 13, 2, 3, 12, 13]], dtype=torch.float64)
    r = referring_metrics(counts, boxes)
    assert set(r) == {"oIoU", "mIoU", "samples"} | {f"P@0.{k}" for k in KS} | {f"mask_P@0.{k}" for k in KS}
    assert r["samples"] == 3
    assert r["oIoU"] == 70.0                                    # (50 + 90 + 0) / (100 + 100 + 0)
    # (0.5 + 0.9 + 1) / 3 = 0.8; float32(0.9) is the only inexact term (0.5 and 1 are exact, and 1e-6 is below half an ulp of 50, 90 and 100):
    # its error of at most 2^-25 ~ 3e-8, a third of it in the mean, x 100 -> below 1e-5
    assert abs(r["mIoU"] - 80.0) < 1e-5
    # strict '>' in exact integers.  0.5: the 0.5 sample misses, the 0.9 sample and the empty pair hit; 0.6 .. 0.8: the same two;
    # 0.9: the 0.9 sample is not above 0.9 either, only the empty pair hits
    assert r["mask_P@0.5"] == 200 / 3
    assert r["mask_P@0.6"] == 200 / 3
    assert r["mask_P@0.7"] == 200 / 3
    assert r["mask_P@0.8"] == 200 / 3
    assert r["mask_P@0.9"] == 100 / 3
    # boxes: IoU 0.5 is not above 0.5, IoU 0.9 is above 0.5 .. 0.8 and not above 0.9, IoU 1 is above all
    assert r["P@0.5"] == 200 / 3
    assert r["P@0.6"] == 200 / 3
    assert r["P@0.7"] == 200 / 3
    assert r["P@0.8"] == 200 / 3
    assert r["P@0.9"] == 100 / 3
    without = referring_metrics(counts)
    assert not any(k.startswith("P@") for k in without) and without["oIoU"] == 70.0 and without["mIoU"] == r["mIoU"]


def test_box_iou_of_disjoint_and_zero_area_boxes_is_zero():
    from ape_amd.evaluation import referring_metrics
    counts = torch.tensor([[1, 1, 1]] * 4, dtype=torch.int64)
    boxes = torch.tensor([[0, 0, 4, 4, 5, 5, 9, 9],             # disjoint
                          [0, 0, 4, 4, 4, 0, 8, 4],             # touching along an edge: no area in common
                          [3, 3, 3, 3, 3, 3, 3, 3],             # a zero-area pair: the union is empty
                          [0, 0, 0, 0, 1, 1, 6, 6]],            # what a sample without prediction stores against a real box
                         dtype=torch.float64)
    r = referring_metrics(counts, boxes)
    assert all(r[f"P@0.{k}"] == 0.0 for k in KS)
    assert r["oIoU"] == 100.0 and r["mIoU"] == 100.0 and all(r[f"mask_P@0.{k}"] == 100.0 for k in KS)


def test_all_empty_and_argument_errors_of_the_metrics():
    from ape_amd.evaluation import referring_metrics
    r = referring_metrics(torch.zeros((2, 3), dtype=torch.int64))
    assert r["oIoU"] == 0.0 and r["mIoU"] == 100.0 and r["mask_P@0.9"] == 100.0       # no union at all: oIoU is 0 by definition
    r = referring_metrics(torch.tensor([[0, 0, 7]]))                                   # no prediction against 7 pixels
    assert r["oIoU"] == 0.0 and r["mIoU"] < 2e-5 and r["mask_P@0.5"] == 0.0
    with pytest.raises(ValueError):
        referring_metrics(torch.zeros((2, 4), dtype=torch.int64))
    with pytest.raises(ValueError):
        referring_metrics(torch.zeros((2, 3), dtype=torch.float32))
    with pytest.raises(ValueError):
        referring_metrics(torch.zeros((0, 3), dtype=torch.int64))
    with pytest.raises(ValueError):
        referring_metrics(torch.tensor([[5, 4, 9]]))                                   # more in common than one side holds
    with pytest.raises(ValueError):
        referring_metrics(torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.float64))


def test_miou_and_oiou_against_the_definition():
    """the reference's three lines (refcocoeval.py:34-39) restated on CPU tensors -- `outputs & labels`, `|`, `.float().sum`, the float32
    epsilon quotient -- and its totals (:246-249, refcoco_evaluation.py:413-414) on 20 random pairs of mixed sizes up to 64 x 48.
    1e-9 in percent covers the float64 summation order of at most 100 values of at most 100; it covers no difference in definition."""
    from ape_amd.evaluation import referring_metrics
    g = torch.Generator().manual_seed(5)
    sizes = [(1, 1), (3, 21), (8, 8), (5, 13), (37, 53), (64, 48), (64, 33), (17, 48), (40, 40), (2, 47)]
    ious, tot_i, tot_u, counts = [], 0.0, 0.0, []
    for i in range(20):
        H, W = sizes[i % len(sizes)]
        outputs = (torch.rand((1, H, W), generator=g) < 0.15 + 0.04 * i).to(torch.uint8)
        labels = (torch.rand((1, H, W), generator=g) < 0.9 - 0.04 * i).to(torch.uint8)
        if i == 7:
            outputs.zero_()                                     # no prediction
        if i == 11:
            outputs.zero_()
            labels.zero_()                                      # empty against empty
        out_i = outputs.int()
        intersection = (out_i & labels).float().sum((1, 2))
        union = (out_i | labels).float().sum((1, 2))
        iou = (intersection + 1e-6) / (union + 1e-6)
        ious.append(iou.item())
        tot_i += intersection.item()
        tot_u += union.item()
        a, b = outputs.bool(), labels.bool()
        counts.append([int((a & b).sum()), int(a.sum()), int(b.sum())])
    r = referring_metrics(torch.tensor(counts, dtype=torch.int64))
    want_m, want_o = sum(ious) / len(ious) * 100, tot_i / tot_u * 100
    print(f"mIoU {r['mIoU']!r} vs {want_m!r}; oIoU {r['oIoU']!r} vs {want_o!r}")
    assert abs(r["mIoU"] - want_m) < 1e-9
    assert abs(r["oIoU"] - want_o) < 1e-9
    assert ious[11] == 1.0 and ious[7] < 1e-6


def test_argument_errors_are_reported_without_a_gpu():
    from ape_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert "ape_hip_mask_paired_counts" in _lib.SIGNATURES and lib.ape_hip_abi_version() == 5
    f, err = lib.ape_hip_mask_paired_counts, lib.ape_hip_last_error        # (a, stride_a, b, stride_b, n, npix, out, stream)
    one = ctypes.c_void_p(64)            # never dereferenced: every call below is refused, or has nothing to do, before any HIP call
    assert f(None, 100, one, 100, 2, 100, one, None) != 0 and b"null" in err()
    assert f(one, 100, None, 100, 2, 100, one, None) != 0 and b"null" in err()
    assert f(one, 100, one, 100, 2, 100, None, None) != 0 and b"null" in err()
    assert f(None, 0, None, 0, 2, 0, None, None) != 0 and b"null" in err()           # npix == 0 still writes out
    assert f(one, 100, one, 100, -1, 100, one, None) != 0 and b"negative" in err()
    assert f(one, 100, one, 100, 70000, 100, one, None) != 0 and b"65535" in err()
    assert f(one, 1 << 32, one, 1 << 32, 1, 1 << 32, one, None) != 0 and b"too large" in err()
    assert f(one, 99, one, 100, 2, 100, one, None) != 0 and b"stride" in err()
    assert f(one, 100, one, 99, 2, 100, one, None) != 0 and b"stride" in err()
    assert f(None, 0, None, 0, 0, 100, None, None) == 0                                # n == 0: a successful no-op


def test_wrapper_refuses_host_tensors():
    from ape_amd import ops
    m = torch.zeros((2, 6, 10), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        ops.mask_paired_counts(m, m)


def test_reduce_is_a_no_op_without_a_process_group():
    from ape_amd.evaluation import ReferringAccumulator
    acc = ReferringAccumulator()
    acc.reduce()
    assert acc.n == 0 and acc.counts is None
    with pytest.raises(RuntimeError):
        acc.compute()
    with pytest.raises(ValueError):
        acc.update(None, None)                                  # no ground truth
