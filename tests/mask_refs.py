"""float64 definitions of the mask resampling operations (csrc/masks.hip) and the rule their bitmaps are compared by.

Written from the formulas of F.interpolate (bilinear, align_corners=False), torchvision roi_align (aligned=True,
sampling_ratio=0, spatial_scale=1) and detectron2's _do_paste_mask (F.grid_sample, align_corners=False, zeros padding);
plain torch on the CPU, independent of tests/ref_ops.py and oracle/thirdparty.py.  Every function returns the value BEFORE
the threshold: compare_bits() then demands equal bits wherever that value is further from the threshold than fp32
evaluation can move it, and bounds how many pixels may lie closer.
"""
import collections
import functools
import math

import torch
import torch.nn.functional as F

F64 = torch.float64


def _axis_taps(n_in, n_out):
    """lower tap, upper tap, upper weight of each of n_out destinations on an axis of n_in sources"""
    dst = torch.arange(n_out, dtype=F64)
    src = ((dst + 0.5) * n_in / n_out - 0.5).clamp_min(0.0)
    lo = src.floor().long().clamp_max(n_in - 1)
    hi = (lo + 1).clamp_max(n_in - 1)
    return lo, hi, src - lo.to(F64)


def bilinear_value(x, H, W):
    """x [C, h, w] (any float type, converted exactly) -> float64 [C, H, W]"""
    x = x.detach().cpu().to(F64)
    h, w = x.shape[-2:]
    y0, y1, ly = _axis_taps(h, H)
    x0, x1, lx = _axis_taps(w, W)
    ly, lx = ly[:, None], lx[None, :]
    top = (1.0 - lx) * x[:, y0][:, :, x0] + lx * x[:, y0][:, :, x1]
    bot = (1.0 - lx) * x[:, y1][:, :, x0] + lx * x[:, y1][:, :, x1]
    return (1.0 - ly) * top + ly * bot


def upsample_value(logits, h0, w0, S):
    """logits [n, h0*w0] (rows may be a strided view) -> float64 [n, S, S], the upsampled logit"""
    n = logits.shape[0]
    return bilinear_value(logits.detach().cpu().to(F64).reshape(n, h0, w0), S, S)


def upsample_sigmoid_value(logits_t, h0, w0, S, crop_h, crop_w):
    """pixel-major logits [h0*w0, n] -> float64 [crop_h*crop_w, n], sigmoid of the upsampled logit on the top-left crop"""
    n = logits_t.shape[1]
    up = upsample_value(logits_t.detach().cpu().to(F64).t(), h0, w0, S)[:, :crop_h, :crop_w]
    return torch.sigmoid(up).reshape(n, -1).t().contiguous()


def roi_align_value(bits, box, P):
    """bits [H, W] (0 / 1), box xyxy (its float32 values, converted exactly) -> float64 [P, P], the mean over the sampling grid"""
    img = bits.detach().cpu().to(F64)
    H, W = img.shape
    x1, y1, x2, y2 = [float(v) for v in torch.as_tensor(box).detach().cpu().to(F64)]
    sw, sh = x1 - 0.5, y1 - 0.5
    rw, rh = (x2 - 0.5) - sw, (y2 - 0.5) - sh
    bw, bh = rw / P, rh / P
    gh, gw = int(math.ceil(rh / P)), int(math.ceil(rw / P))
    if gh <= 0 or gw <= 0:
        return torch.zeros((P, P), dtype=F64)
    p = torch.arange(P, dtype=F64)
    ys = (sh + p[:, None] * bh + (torch.arange(gh, dtype=F64)[None, :] + 0.5) * bh / gh).reshape(-1)      # [P*gh]
    xs = (sw + p[:, None] * bw + (torch.arange(gw, dtype=F64)[None, :] + 0.5) * bw / gw).reshape(-1)      # [P*gw]

    def taps(c, size):
        dead = (c < -1.0) | (c > size)
        c = c.clamp_min(0.0)
        lo = c.floor().long()
        last = lo >= size - 1
        lo = torch.where(last, torch.full_like(lo, size - 1), lo)
        hi = torch.where(last, lo, lo + 1)
        c = torch.where(last, lo.to(F64), c)
        return dead, lo, hi, c - lo.to(F64)

    dy, ylo, yhi, ly = taps(ys, H)
    dx, xlo, xhi, lx = taps(xs, W)
    ly, lx = ly[:, None], lx[None, :]
    v = ((1.0 - ly) * (1.0 - lx) * img[ylo][:, xlo] + (1.0 - ly) * lx * img[ylo][:, xhi] +
         ly * (1.0 - lx) * img[yhi][:, xlo] + ly * lx * img[yhi][:, xhi])
    v = torch.where(dy[:, None] | dx[None, :], torch.zeros_like(v), v)
    return v.reshape(P, gh, P, gw).sum(dim=(1, 3)) / max(gh * gw, 1)


def paste_value(mask, box, Ho, Wo):
    """mask [P, P] (0 / 1), box xyxy in the output frame (float32 values, converted exactly) -> float64 [Ho, Wo]"""
    m = mask.detach().cpu().to(F64)
    P = m.shape[0]
    x0, y0, x1, y1 = [float(v) for v in torch.as_tensor(box).detach().cpu().to(F64)]
    mp = torch.zeros((P + 2, P + 2), dtype=F64)          # one ring of zero padding: tap t lives at index t + 1
    mp[1:-1, 1:-1] = m

    def taps(n, a, b):
        g = (torch.arange(n, dtype=F64) + 0.5 - a) / (b - a) * 2.0 - 1.0
        f = ((g + 1.0) * P - 1.0) / 2.0
        fl = f.floor()
        lo = fl.clamp(-1, P).long() + 1                  # every tap outside [0, P) reads padding
        hi = (fl + 1).clamp(-1, P).long() + 1
        return lo, hi, f - fl

    ylo, yhi, ly = taps(Ho, y0, y1)
    xlo, xhi, lx = taps(Wo, x0, x1)
    ly, lx = ly[:, None], lx[None, :]
    return ((1.0 - ly) * (1.0 - lx) * mp[ylo][:, xlo] + (1.0 - ly) * lx * mp[ylo][:, xhi] +
            ly * (1.0 - lx) * mp[yhi][:, xlo] + ly * lx * mp[yhi][:, xhi])


Compared = collections.namedtuple("Compared", "ambiguous_share diff_in_band diff_out_of_band")


def compare_bits(got, value, thr, strict, band, cap, label=""):
    """got: 0 / 1 of any integer or bool type; value: the float64 pre-threshold value of the same shape.

    want = value > thr (strict) or value >= thr.  Pixels with |value - thr| <= band are ambiguous; everywhere else got must
    EQUAL want (band = 0: no pixel is ambiguous, all must match).  More than `cap` of the pixels ambiguous fails too: the
    comparison would be vacuous.  Prints and returns (ambiguous share, differing pixels inside the band, differing pixels
    outside the band)."""
    got = got.detach().cpu().reshape(-1)
    value = value.detach().cpu().to(F64).reshape(-1)
    assert got.numel() == value.numel(), (got.numel(), value.numel())
    assert bool(((got == 0) | (got == 1)).all()), f"{label}: bytes other than 0 / 1"
    want = (value > thr) if strict else (value >= thr)
    ambiguous = (value - thr).abs() <= band
    if band == 0:                                        # exact arithmetic: the tie itself is decided by > against >=, nothing is ambiguous
        ambiguous = torch.zeros_like(ambiguous)
    diff = got.bool() != want
    share = ambiguous.double().mean().item() if value.numel() else 0.0
    inside, outside = int((diff & ambiguous).sum()), int((diff & ~ambiguous).sum())
    print(f"{label}: ambiguous {share:.4%} of {value.numel()}, differing in band {inside}, out of band {outside}")
    assert outside == 0, f"{label}: {outside} pixels differ outside the band of {band:g} (first at flat index {int(torch.nonzero(diff & ~ambiguous)[0])})"
    assert share <= cap, f"{label}: {share:.3%} of the pixels are within {band:g} of the threshold (cap {cap:.1%}): vacuous"
    return Compared(share, inside, outside)


# ---------------------------------------------------------------------------------------------------------------
# The cases, shared by tests/test_mask_refs.py (CPU: references and caps) and tests/test_masks_gpu.py (the kernels).
# Inputs come from seeded CPU generators; the float64 values are computed once per case and must not be modified.
# Coordinates stay below 256 in magnitude: the bands below are derived for that range.
# ---------------------------------------------------------------------------------------------------------------
KINDS = ("noise", "blobs")
CAP = 0.01                       # at most 1 % of a case's pixels may be ambiguous
UPSAMPLE_BAND_REL = 1e-4         # band = 1e-4 * max|logit|: fp32 blend (a few 2^-24 max|tap|) + fp32 source coordinate (~1e-5 x slope 2 max|tap|)
UNIT_BAND = 1e-3                 # roi_align / paste: the same reasoning on a value in [0, 1]

# (h0, w0, S) -> the path of mask_upsample_bits_kernel it reaches
UPSAMPLE_CASES = [
    (16, 16, 64),                # x4 register path, 16-byte store
    (12, 16, 64),                # x4 in x only
    (10, 10, 40),                # x4 taps for two groups; general taps and the scalar store for the last
    (7, 9, 37),                  # general taps, ragged tail
    (24, 24, 64),                # general taps, 16-byte store
    (1, 5, 20),                  # a single source row
    (32, 32, 16),                # downsampling
]
UPSAMPLE_N = 3
UPSAMPLE_PAD = 8                 # slack elements behind each row of the padded-stride case, set to NaN

ROI_BITS_SHAPE = (8, 40, 56)
ROI_P = (7, 16)
ROI_BOXES = [
    (5.3, 4.1, 49.7, 33.2),      # interior
    (-6.0, -3.5, 20.2, 18.9),    # overhanging top-left
    (30.1, 20.7, 70.0, 50.0),    # overhanging bottom-right
    (60.0, 45.0, 80.0, 70.0),    # outside by more than 1 px: all zeros
    (10.2, 10.4, 10.9, 10.8),    # sub-pixel
    (-8.0, -8.0, 64.0, 48.0),    # larger than the image
    (12.0, 9.0, 12.0, 30.0),     # empty: all zeros
    (3.0, 2.0, 54.9, 39.1),      # near-full
]
ROI_ALL_ZERO = (3, 6)

PASTE_FRAMES = [(48, 64), (45, 70), (33, 16)]      # 16-byte stores + zero-run early-out / scalar stores / one group per row
PASTE_P = {"noise": 12, "blobs": 28}
PASTE_ALL_ZERO = (3,)


def paste_boxes(Ho, Wo, P):
    """float32 [8, 4] boxes in a Ho x Wo frame for P x P masks; the decimals keep every edge off the half-pixel lattice"""
    k = math.floor(0.4 * Wo)
    left = 15.5 - 0.45 * 17.4 / P                        # box 6: the source coordinate of column 15 is 0.45 - 0.5 = -0.05
    return torch.tensor([
        (0.21 * Wo + 0.13, 0.17 * Ho + 0.29, 0.83 * Wo - 0.41, 0.88 * Ho - 0.23),          # interior
        (-0.3 * Wo + 0.37, -0.2 * Ho + 0.11, 0.55 * Wo + 0.19, 0.6 * Ho + 0.43),           # overhanging top and left
        (0.45 * Wo + 0.27, 0.38 * Ho + 0.31, 1.25 * Wo + 0.33, 1.3 * Ho + 0.17),           # overhanging bottom and right
        (Wo + 4.3, Ho + 3.7, Wo + 30.1, Ho + 25.9),                                        # outside the frame: all zeros
        (-0.4 * Wo - 0.23, -0.35 * Ho - 0.31, 1.3 * Wo + 0.47, 1.45 * Ho + 0.39),          # larger than the frame
        (k + 0.27, 0.2 * Ho + 0.15, k + 0.89, 0.8 * Ho + 0.35),                            # narrower than one pixel
        # left edge in one 16-pixel group, right edge two groups on; of the first group only its last pixel (x = 15) is in range, and only
        # through its upper tap (lower tap -1): the narrowest group that the zero-run early-out must NOT take
        (left, 0.1 * Ho + 0.4, left + 17.4, 0.7 * Ho + 0.2),
        (Wo - 13.6, 2.3, Wo - 1.2, Ho - 3.4),                                              # against the right border
    ], dtype=torch.float32)


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _smooth(t):
    """the 5 x 5 box filter of tests/test_ops_gpu.py::test_mask_postprocess; t [n, h, w]"""
    return F.avg_pool2d(F.pad(t[:, None], (2, 2, 2, 2), mode="replicate"), 5, 1)[:, 0]


def _field(kind, n, h, w, seed):
    x = torch.randn(n, h, w, generator=_gen(seed))
    return _smooth(x) if kind == "blobs" else x


def _random_bits(kind, n, h, w, seed):
    if kind == "blobs":
        return (_field(kind, n, h, w, seed) > 0).to(torch.uint8)
    return (torch.rand(n, h, w, generator=_gen(seed)) < 0.5).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def upsample_case(kind, h0, w0, S, dtype, padded=False):
    """-> (logits [n, h0*w0] of dtype on the CPU, float64 value [n, S, S], band); padded: rows are a view of a [n, h0*w0 + 8] buffer whose
    slack is NaN"""
    x = _field(kind, UPSAMPLE_N, h0, w0, seed=1000 + 37 * h0 + 5 * w0 + S).reshape(UPSAMPLE_N, h0 * w0).to(dtype)
    if padded:
        buf = torch.full((UPSAMPLE_N, h0 * w0 + UPSAMPLE_PAD), float("nan"), dtype=dtype)
        buf[:, : h0 * w0] = x
        x = buf[:, : h0 * w0]
    return x, upsample_value(x, h0, w0, S), UPSAMPLE_BAND_REL * x.double().abs().max().item()


@functools.lru_cache(maxsize=None)
def roi_case(kind, P):
    """-> (bits uint8 [8, H, W], boxes float32 [8, 4], float64 value [8, P, P])"""
    n, H, W = ROI_BITS_SHAPE
    bits = _random_bits(kind, n, H, W, seed=2034)
    boxes = torch.tensor(ROI_BOXES, dtype=torch.float32)
    return bits, boxes, torch.stack([roi_align_value(bits[i], boxes[i], P) for i in range(n)])


@functools.lru_cache(maxsize=None)
def paste_case(kind, Ho, Wo):
    """-> (masks uint8 [8, P, P], boxes float32 [8, 4], float64 value [8, Ho, Wo])"""
    P = PASTE_P[kind]
    masks = _random_bits(kind, 8, P, P, seed=3013)
    boxes = paste_boxes(Ho, Wo, P)
    return masks, boxes, torch.stack([paste_value(masks[i], boxes[i], Ho, Wo) for i in range(8)])


# exact ties: dyadic geometry, every fp32 operation of the kernels is exact, so band = 0 and ALL pixels must match
TIE_SEEDS = {"upsample": 1, "roi_align": 1, "paste": 1}


@functools.lru_cache(maxsize=None)
def tie_upsample(dtype):
    """+-1 logits, 16 x 16 -> 8 x 8: every output is the mean of 4 taps; an exact 0 gives bit 0 (strict >)"""
    x = (torch.rand(UPSAMPLE_N, 256, generator=_gen(TIE_SEEDS["upsample"])) < 0.5).to(dtype) * 2 - 1
    return x, upsample_value(x, 16, 16, 8)


@functools.lru_cache(maxsize=None)
def tie_roi():
    """box (0.5, 0.5, 16.5, 16.5), P = 8: a 2 x 2 grid of half-pixel samples per bin; a mean of exactly 0.5 gives bit 1 (>=)"""
    bits = _random_bits("noise", 1, 16, 16, seed=TIE_SEEDS["roi_align"])
    boxes = torch.tensor([(0.5, 0.5, 16.5, 16.5)], dtype=torch.float32)
    return bits, boxes, roi_align_value(bits[0], boxes[0], 8)[None]


@functools.lru_cache(maxsize=None)
def tie_paste():
    """P = 16 into box (0, 0, 8, 8) of an 8 x 16 frame: every weight is 0.25; exactly 0.5 gives bit 1 (>=)"""
    masks = _random_bits("noise", 3, 16, 16, seed=TIE_SEEDS["paste"])
    boxes = torch.tensor([(0.0, 0.0, 8.0, 8.0)] * 3, dtype=torch.float32)
    return masks, boxes, torch.stack([paste_value(masks[i], boxes[i], 8, 16) for i in range(3)])


# the continuous outputs of the same tap code: (name, h0, w0, S, crop_h, crop_w, n, slack columns behind each input row)
SIGMOID_CASES = [
    ("single_source_row", 1, 7, 20, 13, 20, 12, 0),
    ("single_source_column", 6, 1, 20, 20, 9, 12, 0),
    ("no_crop", 5, 6, 24, 24, 24, 12, 0),
    ("scalar_4_query_tail", 6, 5, 20, 17, 19, 12, 0),
    ("scalar_partial_group", 6, 5, 20, 17, 19, 10, 0),
    ("vector", 6, 5, 20, 17, 19, 16, 0),
    ("padded_ldl_vector", 6, 5, 20, 17, 19, 16, 4),
    ("padded_ldl_scalar", 6, 5, 20, 17, 19, 12, 3),
]
HALF_ULP_AT_ONE = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}


@functools.lru_cache(maxsize=None)
def sigmoid_case(name, in_dtype):
    """-> (pixel-major logits [h0*w0, n] of in_dtype, float64 probabilities [crop_h*crop_w, n], max|logit|)"""
    _, h0, w0, S, ch, cw, n, pad = next(c for c in SIGMOID_CASES if c[0] == name)
    x = (torch.randn(h0 * w0, n, generator=_gen(4000 + n + pad)) * 3.0).to(in_dtype)
    if pad:
        buf = torch.full((h0 * w0, n + pad), float("nan"), dtype=in_dtype)
        buf[:, :n] = x
        x = buf[:, :n]
    return x, upsample_sigmoid_value(x, h0, w0, S, ch, cw), x.double().abs().max().item()


# bilinear_resize: (name, C, h, w, H, W, padded strides)
RESIZE_CASES = [
    ("single_source_row", 3, 1, 7, 5, 20, False),
    ("single_source_column", 3, 6, 1, 20, 4, False),
    ("upscale_odd", 2, 9, 11, 23, 31, False),
    ("downscale_padded_view", 2, 33, 40, 20, 17, True),
    ("identity", 2, 8, 8, 8, 8, False),
]


@functools.lru_cache(maxsize=None)
def resize_case(name):
    """-> (x float32 [C, h, w], float64 value [C, H, W], max|x|); padded: x is a view into a larger NaN-filled buffer"""
    _, C, h, w, H, W, padded = next(c for c in RESIZE_CASES if c[0] == name)
    x = torch.randn(C, h, w, generator=_gen(5000 + h + w))
    if padded:
        buf = torch.full((C, h + 3, w + 5), float("nan"))
        buf[:, :h, :w] = x
        x = buf[:, :h, :w]
    return x, bilinear_value(x, H, W), x.abs().max().item()
