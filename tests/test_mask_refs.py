"""CPU checks of tests/mask_refs.py: the float64 definitions agree with the existing fp32 torch / oracle.thirdparty definitions
(tests/ref_ops.py) under the comparison rule, every case of tests/test_masks_gpu.py stays under the ambiguity cap, and no case is
trivially all ones or all zeros.  No GPU needed."""
import pytest
import torch

import mask_refs as R
import ref_ops

DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _balanced(value, thr, strict, label):
    want = (value > thr) if strict else (value >= thr)
    ones = want.double().mean().item()
    print(f"{label}: {ones:.1%} ones")
    assert 0.05 <= ones <= 0.95, f"{label}: {ones:.1%} ones"


def test_compare_bits_rule():
    value = torch.tensor([0.2, 0.5, 0.5004, 0.9, 0.4996, 0.1] + [0.0] * 294, dtype=torch.float64)
    want = (value >= 0.5).to(torch.uint8)
    r = R.compare_bits(want, value, 0.5, False, 1e-3, 0.01)
    assert r == (3 / 300, 0, 0)
    flipped = want.clone()
    flipped[2] ^= 1                                      # inside the band: counted, tolerated
    assert R.compare_bits(flipped, value, 0.5, False, 1e-3, 0.01) == (3 / 300, 1, 0)
    flipped[3] ^= 1                                      # outside: one pixel is enough to fail
    with pytest.raises(AssertionError, match="outside the band"):
        R.compare_bits(flipped, value, 0.5, False, 1e-3, 0.01)
    with pytest.raises(AssertionError, match="vacuous"):
        R.compare_bits(want, value, 0.5, False, 1e-3, 0.005)
    with pytest.raises(AssertionError, match="outside the band"):          # band 0: the tie itself is pinned, > is not >=
        R.compare_bits((value > 0.5).to(torch.uint8), value, 0.5, False, 0.0, 0.01)
    with pytest.raises(AssertionError, match="0 / 1"):
        R.compare_bits(want * 255, value, 0.5, False, 1e-3, 0.01)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.UPSAMPLE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_upsample_reference(case, kind, dtype):
    h0, w0, S = case
    for padded in ((False, True) if case == (16, 16, 64) else (False,)):
        logits, value, band = R.upsample_case(kind, h0, w0, S, dtype, padded)
        label = f"upsample {case} {kind} {dtype} padded={padded}"
        assert not torch.isnan(value).any()
        R.compare_bits(ref_ops.mask_upsample_bits(logits, h0, w0, S), value, 0.0, True, band, R.CAP, label)
        _balanced(value, 0.0, True, label)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("P", R.ROI_P)
def test_roi_align_reference(P, kind):
    bits, boxes, value = R.roi_case(kind, P)
    label = f"roi_align P={P} {kind}"
    got = ref_ops.roi_align_bits(bits, boxes, P)
    R.compare_bits(got, value, 0.5, False, R.UNIT_BAND, R.CAP, label)              # the cap: pooled over the 8 boxes
    for i in range(len(boxes)):
        r = R.compare_bits(got[i], value[i], 0.5, False, R.UNIT_BAND, R.CAP if P == 16 else 1.0, f"{label} box {i}")
        assert r.diff_out_of_band == 0
    for i in R.ROI_ALL_ZERO:
        assert float(value[i].abs().max()) == 0.0
    keep = [i for i in range(len(boxes)) if i not in R.ROI_ALL_ZERO]
    _balanced(value[keep], 0.5, False, label)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("frame", R.PASTE_FRAMES, ids=lambda f: "x".join(map(str, f)))
def test_paste_reference(frame, kind):
    Ho, Wo = frame
    masks, boxes, value = R.paste_case(kind, Ho, Wo)
    label = f"paste {frame} {kind}"
    got = ref_ops.paste_bits(masks, boxes, Ho, Wo)
    R.compare_bits(got, value, 0.5, False, R.UNIT_BAND, R.CAP, label)
    for i in range(len(boxes)):
        R.compare_bits(got[i], value[i], 0.5, False, R.UNIT_BAND, R.CAP, f"{label} box {i}")
    for i in R.PASTE_ALL_ZERO:
        assert float(value[i].abs().max()) == 0.0
    _balanced(value[0], 0.5, False, label + " interior box")
    # box 6: column 15 is reached only through its upper tap (lower tap -1), and some of its pixels are ones well clear of the band:
    # an early-out that treats the group of columns 0..15 as out of range loses them
    x0, x1, P = float(boxes[6, 0]), float(boxes[6, 2]), masks.shape[1]
    f15 = (15.5 - x0) / (x1 - x0) * P - 0.5
    ones15 = int((value[6][:, 15] >= 0.5 + R.UNIT_BAND).sum())
    print(f"{label}: box 6 source coordinate of column 15 = {f15:.3f}, ones in column 15: {ones15}, in columns 0..14: {int((value[6][:, :15] >= 0.5).sum())}")
    assert -0.5 <= f15 < 0.0 and ones15 >= 3 and int((value[6][:, :15] >= 0.5).sum()) == 0
    assert abs(float(boxes.abs().max())) <= 256


def test_tie_cases_have_ties():
    for dtype in DTYPES:
        logits, value = R.tie_upsample(dtype)
        ties = int((value == 0.0).sum())
        print("upsample ties", dtype, ties)
        assert ties >= 5
        R.compare_bits(ref_ops.mask_upsample_bits(logits, 16, 16, 8), value, 0.0, True, 0.0, 1.0, f"upsample tie {dtype}")
    bits, boxes, value = R.tie_roi()
    ties = int((value == 0.5).sum())
    print("roi_align ties", ties)
    assert ties >= 5
    R.compare_bits(ref_ops.roi_align_bits(bits, boxes, 8), value, 0.5, False, 0.0, 1.0, "roi_align tie")
    masks, boxes, value = R.tie_paste()
    ties = int((value == 0.5).sum())
    print("paste ties", ties)
    assert ties >= 5
    R.compare_bits(ref_ops.paste_bits(masks, boxes, 8, 16), value, 0.5, False, 0.0, 1.0, "paste tie")


@pytest.mark.parametrize("case", R.SIGMOID_CASES, ids=lambda c: c[0])
def test_sigmoid_reference(case):
    name, h0, w0, S, ch, cw, n, _ = case
    for dtype in DTYPES:
        x, value, amax = R.sigmoid_case(name, dtype)
        assert value.shape == (ch * cw, n) and not torch.isnan(value).any()
        got = ref_ops.mask_upsample_sigmoid(x, h0, w0, S, ch, cw, torch.float32)
        err = (got.double() - value).abs().max().item()
        print(f"sigmoid {name} {dtype}: fp32 torch vs float64 {err:.2e}")
        assert err <= 1e-4 * amax / 4 + 1e-6


@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=lambda c: c[0])
def test_resize_reference(case):
    name, C, h, w, H, W, _ = case
    x, value, amax = R.resize_case(name)
    assert value.shape == (C, H, W) and not torch.isnan(value).any()
    err = (ref_ops.bilinear_resize(x, H, W).double() - value).abs().max().item()
    print(f"resize {name}: fp32 torch vs float64 {err:.2e}")
    assert err <= 1e-4 * amax
