"""-m gpu: the mask resampling kernels of csrc/masks.hip against float64 definitions (tests/mask_refs.py) on every path they
take: x4 / general taps, 16-byte / scalar stores, the zero-run early-out, the adaptive roi_align grid, boxes that overhang,
miss or degenerate, all three logit types, padded strides, and exact ties (> against >=).

The rule (mask_refs.compare_bits): outside a band around the threshold that fp32 evaluation cannot cross, every bit must EQUAL
the float64 one; at most 1 % of a case's pixels may lie inside the band.  tests/test_mask_refs.py checks the references, the
caps and the balance of every case on the CPU."""
import os

import pytest
import torch

import mask_refs as R
import ref_ops

pytestmark = pytest.mark.gpu

# APE_TEST_SELFCHECK=1 runs this file on CPU with ops := ref_ops (validates the test harness itself)
SELF = os.environ.get("APE_TEST_SELFCHECK") == "1"
DEV = "cpu" if SELF else "cuda"

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
_dtname = lambda d: str(d).split(".")[-1]      # noqa: E731
_dims = lambda c: "x".join(map(str, c))        # noqa: E731


@pytest.fixture(scope="module")
def ops():
    if SELF:
        return ref_ops
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import ape_amd.ops as ops
    from ape_amd import _lib

    _lib.load()
    return ops


def _padded_rows_to_dev(x):
    """x: a [n, m] view with a row stride > m (slack NaN) -> the same view on DEV, slack included"""
    n, m = x.shape
    ld = x.stride(0)
    buf = torch.as_strided(x, (n, ld), (ld, 1)).to(DEV)
    return buf[:, :m]


@pytest.mark.parametrize("dtype", DTYPES, ids=_dtname)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.UPSAMPLE_CASES, ids=_dims)
def test_upsample_bits(ops, case, kind, dtype):
    h0, w0, S = case
    logits, value, band = R.upsample_case(kind, h0, w0, S, dtype)
    got = ops.mask_upsample_bits(logits.to(DEV), h0, w0, S)
    assert got.shape == (R.UPSAMPLE_N, S, S) and got.dtype == torch.uint8
    R.compare_bits(got, value, 0.0, True, band, R.CAP, f"upsample {case} {kind} {_dtname(dtype)}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_dtname)
@pytest.mark.parametrize("kind", R.KINDS)
def test_upsample_bits_padded_rows(ops, kind, dtype):
    """rows are a view of a [n, h0*w0 + 8] buffer whose slack is NaN: a tap read past a row's end turns its pixels to 0"""
    h0, w0, S = 16, 16, 64
    logits, value, band = R.upsample_case(kind, h0, w0, S, dtype, True)
    dev = _padded_rows_to_dev(logits)
    assert dev.stride(0) == h0 * w0 + R.UPSAMPLE_PAD and bool(torch.isnan(torch.as_strided(dev, (R.UPSAMPLE_N, R.UPSAMPLE_PAD), (dev.stride(0), 1), h0 * w0)).all())
    got = ops.mask_upsample_bits(dev, h0, w0, S)
    R.compare_bits(got, value, 0.0, True, band, R.CAP, f"upsample padded rows {kind} {_dtname(dtype)}")
    dense = ops.mask_upsample_bits(R.upsample_case(kind, h0, w0, S, dtype)[0].to(DEV), h0, w0, S)
    assert torch.equal(got, dense)                       # the same logits: the stride must not change a bit


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("P", R.ROI_P)
def test_roi_align_bits(ops, P, kind):
    bits, boxes, value = R.roi_case(kind, P)
    got = ops.roi_align_bits(bits.to(DEV), boxes.to(DEV), P)
    assert got.shape == (len(boxes), P, P) and got.dtype == torch.uint8
    label = f"roi_align P={P} {kind}"
    R.compare_bits(got, value, 0.5, False, R.UNIT_BAND, R.CAP, label)              # the cap: pooled over the 8 boxes (49 outputs each at P = 7)
    for i in range(len(boxes)):
        R.compare_bits(got[i], value[i], 0.5, False, R.UNIT_BAND, R.CAP if P == 16 else 1.0, f"{label} box {i}")
    for i in R.ROI_ALL_ZERO:
        assert int(got[i].sum()) == 0


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("frame", R.PASTE_FRAMES, ids=_dims)
def test_paste_bits(ops, frame, kind):
    Ho, Wo = frame
    masks, boxes, value = R.paste_case(kind, Ho, Wo)
    got = ops.paste_bits(masks.to(DEV), boxes.to(DEV), Ho, Wo)
    assert got.shape == (len(boxes), Ho, Wo) and got.dtype == torch.uint8
    label = f"paste {frame} {kind}"
    R.compare_bits(got, value, 0.5, False, R.UNIT_BAND, R.CAP, label)
    for i in range(len(boxes)):
        R.compare_bits(got[i], value[i], 0.5, False, R.UNIT_BAND, R.CAP, f"{label} box {i}")
    for i in R.PASTE_ALL_ZERO:
        assert int(got[i].sum()) == 0
    out = torch.full((len(boxes), Ho, Wo), 7, dtype=torch.uint8, device=DEV)       # out= given: every byte is written, same bits
    ret = ops.paste_bits(masks.to(DEV), boxes.to(DEV), Ho, Wo, out=out)
    assert ret is out and torch.equal(out, got)


@pytest.mark.parametrize("frame", R.PASTE_FRAMES[:2], ids=_dims)
def test_paste_bits_degenerate_rows(ops, frame):
    """postprocess_instance and the graphed runtime paste all k rows and drop the empty boxes afterwards: rows with x1 == x0 or
    y1 == y0 reach the kernel on every frame.  Their own content is unspecified (the caller drops them), but it is 0 / 1 bytes and
    the rows around them are untouched."""
    Ho, Wo = frame
    masks, boxes, value = R.paste_case("noise", Ho, Wo)
    boxes = boxes.clone()
    boxes[2] = torch.tensor([20.3, 5.2, 20.3, 30.1])     # x1 == x0
    boxes[5] = torch.tensor([10.4, 17.6, 40.2, 17.6])    # y1 == y0
    valid = [0, 1, 3, 4, 6, 7]
    got = ops.paste_bits(masks.to(DEV), boxes.to(DEV), Ho, Wo)
    if not SELF:
        torch.cuda.synchronize()
    assert got.shape == (8, Ho, Wo)
    assert bool((got[[2, 5]] <= 1).all())
    alone = ops.paste_bits(masks[valid].contiguous().to(DEV), boxes[valid].contiguous().to(DEV), Ho, Wo)
    assert torch.equal(got[valid], alone)
    R.compare_bits(got[valid], value[valid], 0.5, False, R.UNIT_BAND, R.CAP, f"paste {frame} around degenerate rows")


def test_exact_ties(ops):
    """dyadic geometry: every fp32 operation of the kernels is exact, so nothing is ambiguous -- an upsampled logit of exactly 0 is
    bit 0 (sigmoid > 0.5), a roi_align mean or a pasted value of exactly 0.5 is bit 1 (>= 0.5)"""
    for dtype in DTYPES:
        logits, value = R.tie_upsample(dtype)
        assert int((value == 0.0).sum()) >= 5
        got = ops.mask_upsample_bits(logits.to(DEV), 16, 16, 8)
        assert R.compare_bits(got, value, 0.0, True, 0.0, 0.0, f"upsample ties {_dtname(dtype)}").diff_out_of_band == 0
    bits, boxes, value = R.tie_roi()
    assert int((value == 0.5).sum()) >= 5
    got = ops.roi_align_bits(bits.to(DEV), boxes.to(DEV), 8)
    assert R.compare_bits(got, value, 0.5, False, 0.0, 0.0, "roi_align ties").diff_out_of_band == 0
    masks, boxes, value = R.tie_paste()
    assert int((value == 0.5).sum()) >= 5
    got = ops.paste_bits(masks.to(DEV), boxes.to(DEV), 8, 16)
    assert R.compare_bits(got, value, 0.5, False, 0.0, 0.0, "paste ties").diff_out_of_band == 0


# in -> out types of mask_upsample_sigmoid: fp32 logits into any type, 16-bit logits into their own type or fp32
SIGMOID_TYPES = [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.float32, torch.float16),
                 (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16), (torch.bfloat16, torch.float32),
                 (torch.float16, torch.float32)]


# APE_MASK_UP8=0 sends the cases that the vector kernel takes (n % 8 == 0) through the scalar kernel as well
SIGMOID_RUNS = [(c, "default") for c in R.SIGMOID_CASES] + [(c, "0") for c in R.SIGMOID_CASES if c[6] % 8 == 0]


@pytest.mark.parametrize("case,up8", SIGMOID_RUNS, ids=lambda v: v if isinstance(v, str) else v[0])
def test_upsample_sigmoid_stencil(ops, monkeypatch, case, up8):
    """per element against float64, absolute: 1e-4 max|logit| / 4 (the band of the bitmaps times the sigmoid's slope <= 1/4) + 1e-6
    (expf) + half an ulp of the output type at 1.0"""
    name, h0, w0, S, ch, cw, n, pad = case
    if up8 == "0":
        monkeypatch.setenv("APE_MASK_UP8", "0")
    for in_dt, out_dt in SIGMOID_TYPES:
        x, value, amax = R.sigmoid_case(name, in_dt)
        dev = _padded_rows_to_dev(x) if pad else x.to(DEV)
        got = ops.mask_upsample_sigmoid(dev, h0, w0, S, ch, cw, out_dt)
        assert got.shape == (ch * cw, n) and got.dtype == out_dt
        err = (got.cpu().double() - value).abs().max().item()
        bound = 1e-4 * amax / 4 + 1e-6 + R.HALF_ULP_AT_ONE[out_dt]
        print(f"upsample_sigmoid {name} up8={up8} {_dtname(in_dt)}->{_dtname(out_dt)}: max abs err {err:.3e} (bound {bound:.3e})")
        assert err <= bound


@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=lambda c: c[0])
def test_bilinear_resize_stencil(ops, case):
    name, C, h, w, H, W, padded = case
    x, value, amax = R.resize_case(name)
    if padded:
        base = torch.as_strided(x, (C, h + 3, w + 5), x.stride()).to(DEV)
        dev = base[:, :h, :w]
        assert dev.stride() == x.stride()
    else:
        dev = x.to(DEV)
    got = ops.bilinear_resize(dev, H, W)
    assert got.shape == (C, H, W) and got.dtype == torch.float32
    err = (got.cpu().double() - value).abs().max().item()
    print(f"bilinear_resize {name}: max abs err {err:.3e} (bound {1e-4 * amax:.3e})")
    assert err <= 1e-4 * amax
