"""-m gpu parity tests: every HIP kernel (through the C-ABI) vs its torch fp32 definition (tests/ref_ops.py)."""

import pytest
import torch

import ref_ops

pytestmark = pytest.mark.gpu

import os

# APE_TEST_SELFCHECK=1 runs this file on CPU with ops := ref_ops (validates the test harness itself)
SELF = os.environ.get("APE_TEST_SELFCHECK") == "1"
DEV = "cpu" if SELF else "cuda"


@pytest.fixture(scope="module")
def ops():
    if SELF:
        return ref_ops
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import ape_amd.ops as ops
    from ape_amd import _lib

    _lib.load()
    return ops


def relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def rnd(*shape, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


TOL = {torch.bfloat16: 6e-3, torch.float16: 8e-4, torch.float32: 2e-5}
H16 = (torch.bfloat16, torch.float16)      # the two 16-bit flavours of the pipeline (csrc/common.h h16<>)


def T16(dtype, bf16_tol, f32_tol):
    """tolerance of a 16-bit-input case: given for bf16 (8 significant bits), / 6 for IEEE half (11 bits), f32_tol for float32"""
    return {torch.bfloat16: bf16_tol, torch.float16: bf16_tol / 6, torch.float32: f32_tol}[dtype]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("M,N,K", [(256, 256, 256), (4096, 1024, 1024), (900, 2048, 256), (1000, 130, 64), (333, 8, 256), (87296, 480, 256), (700, 200, 2736), (130, 70, 40)])
def test_gemm_plain(ops, dtype, M, N, K):
    if dtype == torch.float32 and M * N * K > 2e9:
        pytest.skip("f32 validation kernel: keep the case small")
    a, w = rnd(M, K, dtype=dtype, seed=1), rnd(N, K, dtype=dtype, scale=K ** -0.5, seed=2)
    bias = rnd(N, seed=3)
    for odt in (dtype, torch.float32):
        got = ops.gemm(a, w, bias, out_dtype=odt)
        ref = ref_ops.gemm(a, w, bias, out_dtype=odt)
        e = relerr(got, ref)
        print(f"gemm {dtype} M{M} N{N} K{K} out={odt}: relerr {e:.3e}")
        assert e < (TOL[odt] if odt in H16 else 2e-4 if dtype in H16 else 2e-5)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_gemm_epilogues(ops, dtype):
    M, N, K = 1100, 384, 320 if dtype == torch.float32 else 320 + 0
    K = 320
    a, w = rnd(M, K, dtype=dtype, seed=1), rnd(N, K, dtype=dtype, scale=K ** -0.5, seed=2)
    bias = rnd(N, seed=3)
    res32, res16 = rnd(M, N, seed=4), rnd(M, N, dtype=dtype if dtype in H16 else torch.bfloat16, seed=5)
    mask = (torch.arange(M) % 7 == 3).to(DEV)
    cases = {
        "relu": dict(act=ref_ops.ACT_RELU),
        "gelu": dict(act=ref_ops.ACT_GELU),
        "res32": dict(residual=res32, out_dtype=torch.float32),
        "res16": dict(residual=res16, out_dtype=res16.dtype),
        "alpha_clamp": dict(alpha=0.37, clamp=0.8, out_dtype=torch.float32),
        "mask_in": dict(rowmask=mask, mask_mode=ref_ops.MASK_ZERO_INPUT, out_dtype=torch.float32),
        "mask_out": dict(rowmask=mask, mask_mode=ref_ops.MASK_ZERO_OUTPUT, out_dtype=torch.float32),
        "swiglu": dict(act=ref_ops.ACT_SWIGLU, out_dtype=torch.float32),
        "trans": dict(trans_out=True, m_pad=1152, out_dtype=dtype),
        "nobias_trans_gelu": dict(trans_out=True, act=ref_ops.ACT_GELU, out_dtype=torch.float32),
    }
    if dtype == torch.float32:
        cases.pop("res16")
    for name, kw in cases.items():
        b = None if name.startswith("nobias") else bias
        got = ops.gemm(a, w, b, **kw)
        ref = ref_ops.gemm(a, w, b, **kw)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        e = relerr(got, ref)
        print(f"gemm[{name}] {dtype}: relerr {e:.3e}")
        odt = kw.get("out_dtype", dtype)
        assert e < (TOL[odt] if odt in H16 else 3e-4 if dtype in H16 else 2e-5), name
    # RoPE epilogue: 2048 rotated columns of 3072, table rows cycle every 100 rows
    N2 = 3 * 256
    w2 = rnd(N2, K, dtype=dtype, scale=K ** -0.5, seed=6)
    cos, sin = rnd(100, 64, seed=7), rnd(100, 64, seed=8)
    kw = dict(rope=(cos, sin, 100, 64, 512), out_dtype=torch.float32)
    e = relerr(ops.gemm(a, w2, rnd(N2, seed=9), **kw), ref_ops.gemm(a, w2, rnd(N2, seed=9), **kw))
    print(f"gemm[rope] {dtype}: relerr {e:.3e}")
    assert e < 3e-4


@pytest.mark.parametrize("bf", H16)
def test_gemm_into_view(ops, bf):
    """write into a column slice of a wider buffer (ldc > N) and read A from a strided view"""
    M, N, K = 512, 256, 128
    big = rnd(M, 3 * K, dtype=bf, seed=1)
    a = big[:, K:2 * K]
    w = rnd(N, K, dtype=bf, scale=K ** -0.5, seed=2)
    out = torch.zeros(M, 1024, dtype=bf, device=DEV)
    ops.gemm(a, w, None, out=out[:, 256:512])
    ref = ref_ops.gemm(a, w, None)
    assert relerr(out[:, 256:512], ref) < TOL[bf]
    assert out[:, :256].abs().max().item() == 0 and out[:, 512:].abs().max().item() == 0


@pytest.mark.parametrize("bf", H16)
def test_gemm_splitk(ops, bf):
    """split-K ring kernel + reduce/epilogue kernel (tiny-grid GEMMs of the decoder, K = tokens reductions)"""
    for (M, N, K, sk) in [(900, 256, 2048, 8), (900, 256, 2048, None), (256, 256, 87296, 32), (100, 512, 1024, 3), (77, 8, 256, 2)]:
        a, w = rnd(M, K, dtype=bf, seed=1), rnd(N, K, dtype=bf, scale=K ** -0.5, seed=2)
        bias, res = rnd(N, seed=3), rnd(M, N, seed=4)
        for kw in (dict(out_dtype=torch.float32), dict(act=ref_ops.ACT_RELU, residual=res, out_dtype=bf)):
            got = ops.gemm(a, w, bias, splitk=sk, **kw)
            ref = ref_ops.gemm(a, w, bias, **kw)
            e = relerr(got, ref)
            print(f"gemm splitk M{M} N{N} K{K} sk={sk} {list(kw)}: {e:.3e}")
            assert e < (TOL[bf] if kw["out_dtype"] == bf else 3e-4)


@pytest.mark.parametrize("bf", H16)
@pytest.mark.parametrize("trans", [False, True])
def test_gemm_tile64(ops, trans, bf):
    """64x64-tile ring kernel (small launches), with and without split-K, all epilogues that matter for the decoder"""
    M, N, K = 900, 256, 256
    a, w = rnd(M, K, dtype=bf, seed=1), rnd(N, K, dtype=bf, scale=K ** -0.5, seed=2)
    bias, res = rnd(N, seed=3), rnd(M, N, dtype=bf, seed=4)
    if trans:
        cases = [dict(trans_out=True, m_pad=960), dict(trans_out=True, out_dtype=torch.float32, act=ref_ops.ACT_RELU)]
    else:
        cases = [dict(), dict(out_dtype=torch.float32), dict(residual=res, act=ref_ops.ACT_RELU), dict(splitk=4, residual=res),
                 dict(act=ref_ops.ACT_SWIGLU, out_dtype=torch.float32)]
    for kw in cases:
        got = ops.gemm(a, w, bias, tile64=1, **kw)
        ref = ref_ops.gemm(a, w, bias, **kw)
        e = relerr(got, ref)
        print(f"gemm tile64 trans={trans} {list(kw)}: {e:.3e}")
        assert got.shape == ref.shape and e < (TOL[bf] if kw.get("out_dtype") != torch.float32 else 3e-4)
    # ragged shapes
    for (M2, N2, K2) in [(77, 40, 96), (130, 200, 64), (64, 64, 32)]:
        a2, w2 = rnd(M2, K2, dtype=bf, seed=5), rnd(N2, K2, dtype=bf, seed=6)
        e = relerr(ops.gemm(a2, w2, None, tile64=1, out_dtype=torch.float32), ref_ops.gemm(a2, w2, None, out_dtype=torch.float32))
        assert e < 3e-4, (M2, N2, K2, e)


@pytest.mark.parametrize("bf", H16)
def test_gemm_kres(ops, bf):
    """K == 256 register-resident-A kernel (big-M linears of the deformable encoder): every epilogue it takes, full and
    ragged row blocks, partial last column chunk, column splits over blockIdx.y, strided operands"""
    K = 256
    for (M, N) in [(87296, 256), (21824, 2048), (5000, 480), (2048, 1536), (4100, 64), (6000, 2304)]:
        a, w = rnd(M, K, dtype=bf, seed=1), rnd(N, K, dtype=bf, scale=K ** -0.5, seed=2)
        bias, res = rnd(N, seed=3), rnd(M, N, dtype=bf, seed=4)
        mask = (torch.arange(M) % 5 == 2).to(DEV)
        cases = [dict(), dict(out_dtype=torch.float32), dict(residual=res), dict(act=ref_ops.ACT_RELU),
                 dict(rowmask=mask, mask_mode=ref_ops.MASK_ZERO_INPUT), dict(rowmask=mask, mask_mode=ref_ops.MASK_ZERO_OUTPUT, residual=res),
                 dict(residual=res, out_dtype=torch.float32, alpha=0.5, clamp=2.0)]
        if M > 50000:
            cases = cases[:3] + cases[4:5]
        for kw in cases:
            got = ops.gemm(a, w, bias, **kw)
            ref = ref_ops.gemm(a, w, bias, **kw)
            e = relerr(got, ref)
            print(f"gemm kres M{M} N{N} {[k for k in kw]}: {e:.3e}")
            assert e < (3e-4 if kw.get("out_dtype") == torch.float32 else TOL[bf]), (M, N, kw.keys())
    # strided A (column slice), output into a wider buffer, no bias
    big = rnd(4096, 3 * K, dtype=bf, seed=7)
    w = rnd(512, K, dtype=bf, scale=K ** -0.5, seed=8)
    out = torch.zeros(4096, 1024, dtype=bf, device=DEV)
    ops.gemm(big[:, K:2 * K], w, None, out=out[:, 256:768])
    assert relerr(out[:, 256:768], ref_ops.gemm(big[:, K:2 * K], w, None)) < TOL[bf]
    assert out[:, :256].abs().max().item() == 0 and out[:, 768:].abs().max().item() == 0


@pytest.mark.parametrize("bf", H16)
def test_gemm_kres_tail_split(ops, monkeypatch, bf):
    """the K == 256 kernel's TAIL SPLIT: 87 296 encoder tokens are 682 row blocks = one full round of 512 resident workgroups + 170;
    the launcher cuts those 170 into column parts (csrc/gemm.hip) -- bit-identical to the plain grid (APE_KRES_TAILSPLIT=0) for every
    column count the forward uses (offsets | logits 480, value / output 256, the decoder's 6 x 256 value projection, 2048), incl. a ragged
    last row block, a residual, IEEE-half output and a masked value projection"""
    if SELF:
        pytest.skip("grid selection: HIP library only")
    K = 256
    for (M, N) in [(87296, 480), (87296, 1024), (87296, 1536), (87000, 2048), (65536 + 128 * 3 + 5, 1280)]:
        a, w = rnd(M, K, dtype=bf, seed=31), rnd(N, K, dtype=bf, scale=K ** -0.5, seed=32)
        bias = rnd(N, seed=33)
        mask = (torch.arange(M) % 7 == 1).to(DEV)
        cases = [dict(), dict(rowmask=mask, mask_mode=ref_ops.MASK_ZERO_OUTPUT)]
        if N <= 1024:
            cases += [dict(residual=rnd(M, N, dtype=bf, seed=34)), dict(out_dtype=torch.float32)]
        if bf == torch.bfloat16 and N in (480, 1536):
            cases.append(dict(out_dtype=torch.float16))
        for kw in cases:
            monkeypatch.setenv("APE_KRES_TAILSPLIT", "0")
            plain = ops.gemm(a, w, bias, **kw)
            monkeypatch.setenv("APE_KRES_TAILSPLIT", "1")
            got = ops.gemm(a, w, bias, **kw)
            assert torch.equal(got, plain), (M, N, list(kw))
        e = relerr(ops.gemm(a, w, bias), ref_ops.gemm(a, w, bias))
        print(f"gemm kres tail split M{M} N{N}: identical to the plain grid; vs the definition {e:.3e}")
        assert e < TOL[bf]


@pytest.mark.parametrize("bf", H16)
def test_gemm_kres_layernorm_epilogue(ops, bf):
    """K = N = 256 linear + bias + residual + LayerNorm in one launch (the encoder's attention output projection and the norm behind
    it) vs the two-step definition; ragged last row block; statistics on the fp32 sums"""
    for M in (87296, 5000, 2048):
        a, w = rnd(M, 256, dtype=bf, seed=1), rnd(256, 256, dtype=bf, scale=1 / 16, seed=2)
        bias, res = rnd(256, seed=3), rnd(M, 256, dtype=bf, seed=4) * 2.0 + 0.3
        gamma, beta = 1.0 + 0.1 * rnd(256, seed=5), 0.1 * rnd(256, seed=6)
        assert ops.gemm_norm_fusable(a, w, res)
        for r in (res, None):
            got = ops.gemm(a, w, bias, residual=r, norm=(gamma, beta, 1e-5))
            if not SELF:
                from ape_amd import _lib
                assert b"kres_ln" in _lib.load().ape_hip_gemm_last_kernel()
            want = ref_ops.gemm(a, w, bias, residual=r, norm=(gamma, beta, 1e-5))
            two = ref_ops.layernorm(ref_ops.gemm(a, w, bias, residual=r), gamma, beta, 1e-5)      # what two launches give (one more rounding)
            e, e2 = relerr(got, want), relerr(got, two)
            print(f"gemm + LayerNorm epilogue {bf} M{M} residual={r is not None}: {e:.3e} (vs the two-launch form {e2:.3e})")
            assert got.dtype == bf and e < TOL[bf] and e2 < 3 * TOL[bf] and torch.isfinite(got.float()).all()


def test_gemv(ops):
    x = rnd(3, 1024, seed=1)
    for dt in (torch.float32, torch.bfloat16):
        w = rnd(2048, 1024, dtype=dt, scale=1 / 32, seed=2)
        b = rnd(2048, seed=3)
        e = relerr(ops.gemv(x, w, b, alpha=0.5), ref_ops.gemv(x, w, b, alpha=0.5))
        print(f"gemv {dt}: {e:.3e}")
        assert e < 2e-5


def test_head_gemv(ops):
    """per-head matrix-vector products of the single-token language side (replaces torch.einsum / matmul launches)"""
    for (H, N, D) in [(8, 256, 256), (8, 1, 256), (8, 256, 256), (3, 17, 100)]:
        x, w, b = rnd(H, D, seed=1), rnd(H, N, D, scale=D ** -0.5, seed=2), rnd(H, N, seed=3)
        for bias in (None, b):
            e = relerr(ops.head_gemv(x, w, bias, alpha=0.7), ref_ops.head_gemv(x, w, bias, alpha=0.7))
            assert e < 2e-5, (H, N, D, e)


@pytest.mark.parametrize("C,cpad", [(256, 256), (512, 512), (1024, 1024), (2730, 2752), (100, 104), (1536, 1536), (341, 384), (3500, 3504)])
@pytest.mark.parametrize("xdt,ydt", [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float16), (torch.float16, torch.float16)])
def test_layernorm(ops, C, cpad, xdt, ydt):
    M = 1037
    buf = rnd(M, cpad + 8, dtype=xdt, seed=1) * 2 + 0.5
    x = buf[:, :C]
    w, b = rnd(C, seed=2) + 1, rnd(C, seed=3)
    for act in (ref_ops.ACT_NONE, ref_ops.ACT_GELU):
        got = ops.layernorm(x, w, b, 1e-6, out_dtype=ydt, cpad=cpad, act=act)
        ref = ref_ops.layernorm(x, w, b, 1e-6, out_dtype=ydt, cpad=cpad, act=act)
        e = relerr(got, ref)
        print(f"layernorm C{C} {xdt}->{ydt} act{act}: {e:.3e}")
        assert got.shape == (M, cpad) and e < TOL[ydt] * 1.5
        if cpad > C:
            assert got[:, C:].abs().max().item() == 0
    add = rnd(M, C, dtype=ydt, seed=4)
    g1, g2 = ops.layernorm(x, w, b, 1e-5, out_dtype=ydt, cpad=cpad, add=add)
    r1, r2 = ref_ops.layernorm(x, w, b, 1e-5, out_dtype=ydt, cpad=cpad, add=add)
    assert relerr(g1, r1) < TOL[ydt] * 1.5 and relerr(g2, r2) < TOL[ydt] * 1.5


@pytest.mark.parametrize("HW", [256, 5000, 65536])
@pytest.mark.parametrize("xdt,ydt", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.bfloat16), (torch.float16, torch.float16), (torch.float32, torch.float16)])
def test_groupnorm(ops, HW, xdt, ydt):
    x = rnd(HW, 256, dtype=xdt, seed=1) * 1.7 + 3.0  # large mean: exercises the two-pass statistics
    w, b = rnd(256, seed=2) + 1, rnd(256, seed=3)
    add = rnd(HW, 256, dtype=ydt, seed=4)
    for kw in (dict(), dict(act=ref_ops.ACT_RELU), dict(add=add)):
        got = ops.groupnorm(x, w, b, 32, 1e-5, out_dtype=ydt, **kw)
        ref = ref_ops.groupnorm(x, w, b, 32, 1e-5, out_dtype=ydt, **kw)
        e = relerr(got, ref)
        print(f"groupnorm HW{HW} {xdt}->{ydt} {list(kw)}: {e:.3e}")
        assert e < TOL[ydt] * 1.5


def _msda_inputs(shapes, Q, refdim, dtype, seed=0, batch=1):
    L = len(shapes)
    S = sum(h * w for h, w in shapes)
    starts = [0]
    for h, w in shapes[:-1]:
        starts.append(starts[-1] + h * w)
    value = rnd(batch * S, 256, dtype=dtype, seed=seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    offw = torch.cat([torch.randn(batch * Q, 8 * L * 4 * 2, generator=g) * 3.0, torch.randn(batch * Q, 8 * L * 4, generator=g) * 2.0], 1).to(DEV)
    if refdim == 2:
        ref = torch.rand(batch * Q, L, 2, generator=g) * 1.2 - 0.1  # some out-of-range points
    else:
        ref = torch.cat([torch.rand(batch * Q, L, 2, generator=g), torch.rand(batch * Q, L, 2, generator=g) * 0.5], -1)
    return value, shapes, starts, offw, ref.to(DEV).contiguous(), S


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("refdim", [2, 4])
@pytest.mark.parametrize("shapes,Q", [([(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)], 341), ([(32, 20), (16, 10), (8, 5), (4, 3)], 900),
                                      ([(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)], 20000)])
def test_msda_fused(ops, dtype, refdim, shapes, Q):
    value, shapes, starts, offw, ref, S = _msda_inputs(shapes, Q, refdim, dtype)
    got = ops.msda_fused(value, shapes, starts, offw, ref, out_dtype=torch.float32 if dtype == torch.float32 else dtype)
    want = ref_ops.msda_fused(value, shapes, starts, offw, ref, out_dtype=torch.float32)
    e = relerr(got, want)
    print(f"msda_fused {dtype} refdim{refdim} L{len(shapes)} Q{Q}: {e:.3e}")
    assert e < (TOL[dtype] if dtype in H16 else 1e-4)
    if dtype in H16:
        got32 = ops.msda_fused(value, shapes, starts, offw, ref, out_dtype=torch.float32)
        assert relerr(got32, want) < 1e-4


@pytest.mark.parametrize("refdim,Q", [(2, 20000), (4, 900), (2, 341)])
def test_msda_half_values(ops, refdim, Q):
    """production path: values projected to IEEE half (saturating K = 256 GEMM), consumed by the sampler with v_fma_mix_f32;
    vs the definition on the SAME half tensor (fp32 and half offsets), and the masked / saturating value projection itself"""
    shapes = [(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)] if Q > 341 else [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    value, shapes, starts, offw, ref, S = _msda_inputs(shapes, Q, refdim, torch.bfloat16)
    vh = (value.float() * 3.0).to(torch.float16)                    # a genuinely half tensor (values off the bf16 grid)
    for ow in (offw, offw.to(torch.float16)):
        want = ref_ops.msda_fused(vh, shapes, starts, ow.float(), ref, out_dtype=torch.float32)
        got32 = ops.msda_fused(vh, shapes, starts, ow, ref, out_dtype=torch.float32)
        got16 = ops.msda_fused(vh, shapes, starts, ow, ref, out_dtype=torch.bfloat16)
        e32, e16 = relerr(got32, want), relerr(got16, want)
        print(f"msda_fused half values refdim{refdim} Q{Q} offsets {ow.dtype}: f32 out {e32:.3e}, bf16 out {e16:.3e}")
        assert e32 < 1e-4 and e16 < TOL[torch.bfloat16]
    if S >= 2048:
        x = rnd(S, 256, dtype=torch.bfloat16, seed=11)
        w, b = rnd(256, 256, dtype=torch.bfloat16, scale=1 / 16, seed=12), rnd(256, seed=13)
        b[3] = 1e6                                                   # one column saturates
        mask = (torch.arange(S) % 7 == 0).to(torch.uint8).to(DEV)
        got = ops.gemm(x, w, b, rowmask=mask, mask_mode=ops.MASK_ZERO_OUTPUT, out_dtype=torch.float16, clamp=65504.0)
        want = ref_ops.gemm(x, w, b, rowmask=mask, mask_mode=ops.MASK_ZERO_OUTPUT, out_dtype=torch.float16, clamp=65504.0)
        assert got.dtype == torch.float16 and torch.isfinite(got.float()).all() and float(got[1, 3]) == 65504.0 and float(got[0, 3]) == 0.0
        assert relerr(got, want) < 1e-3


def test_msda_half_offsets_path(ops):
    """production encoder path: the K = 256 offset | logit GEMM writes IEEE half, the sampler reads it (exactly the rounded
    values: vs the definition on the SAME half tensor the sampler matches like the fp32 path; vs fp32 offsets the difference
    is the half rounding of offsets / logits)"""
    shapes = [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4)]
    Q = 4096 + 37
    value, shapes, starts, offw, ref, S = _msda_inputs(shapes, Q, 2, torch.bfloat16)
    q = rnd(Q, 256, dtype=torch.bfloat16, seed=7)
    w = rnd(480, 256, dtype=torch.bfloat16, scale=0.3, seed=8)
    b = rnd(480, seed=9)
    o16 = ops.gemm(q, w, b, out_dtype=torch.float16)
    if not SELF:
        from ape_amd import _lib
        assert b"kres_kernel<0, false, true>" in _lib.load().ape_hip_gemm_last_kernel()      # the K = 256 kernel's half-output instantiation
    o32 = ops.gemm(q, w, b, out_dtype=torch.float32)
    assert o16.dtype == torch.float16 and torch.equal(o16, o32.to(torch.float16))            # same accumulators, one RNE rounding
    got = ops.msda_fused(value, shapes, starts, o16, ref, out_dtype=torch.float32)
    want = ref_ops.msda_fused(value, shapes, starts, o16.float(), ref, out_dtype=torch.float32)
    e = relerr(got, want)
    full = ref_ops.msda_fused(value, shapes, starts, o32, ref, out_dtype=torch.float32)
    print(f"msda_fused half offsets: {e:.3e} vs the definition on the half tensor; half-vs-fp32 offsets {relerr(want, full):.3e}")
    assert e < 1e-4 and relerr(want, full) < 1.2e-2      # harsh synthetic weights (logit std ~5, offsets of several pixels on a 4x4 level); below the bf16 rounding of the output


@pytest.mark.parametrize("shapes", [[(64, 64), (32, 32), (16, 16), (8, 8), (4, 4)], [(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)],
                                    [(96, 96), (48, 48), (24, 24), (12, 12), (6, 6)]], ids=["64", "256", "96"])
@pytest.mark.parametrize("out_dt", [torch.bfloat16, torch.float16])
def test_msda_lds_staged_encoder_path(ops, monkeypatch, shapes, out_dt):
    """the LDS-staged sampler of the encoder's level-0 queries (csrc/msda.hip msda_lds_kernel; multi_scale_deform_attn.py:298-303 with the
    queries' own positions as reference points): vs the definition and vs the quad kernel (APE_MSDA_LDS=0) on the SAME inputs -- local
    offsets (every corner inside the staged windows), offsets far beyond the halo (global-memory fall-back), a padded image (valid
    ratios < 1: windows shifted against the tile), random reference points (the locality assumption violated on purpose), fp32 and
    half offsets | logits; 96 x 96: extents that are not powers of two (division path)"""
    if SELF:
        pytest.skip("kernel-internal data path: HIP library only")
    S = sum(h * w for h, w in shapes)
    g = torch.Generator().manual_seed(5)
    value = (torch.randn(S, 256, generator=g) * 2.0).to(torch.float16).to(DEV)
    starts = [0]
    for h, w in shapes[:-1]:
        starts.append(starts[-1] + h * w)

    def own_refs(vr):                # get_reference_points (deformable_transformer_vl.py:371-400) for valid ratios vr = (vx, vy)
        pts = []
        for (H, W) in shapes:
            ys, xs = torch.meshgrid(torch.linspace(0.5, H - 0.5, H), torch.linspace(0.5, W - 0.5, W), indexing="ij")
            pts.append(torch.stack((xs.reshape(-1) / (vr[0] * W), ys.reshape(-1) / (vr[1] * H)), -1))
        ref = torch.cat(pts, 0)[:, None, :] * torch.tensor(vr)[None, None, :]
        return ref.repeat(1, 5, 1).contiguous().to(DEV)

    cases = [("local +-3 px", own_refs((1.0, 1.0)), 1.5), ("beyond the halo +-20 px", own_refs((1.0, 1.0)), 10.0),
             ("padded 0.67 x 0.81", own_refs((0.67, 0.81)), 2.0), ("random references", torch.rand(S, 5, 2, generator=g).to(DEV), 2.0)]
    for name, ref, sigma in cases:
        off = torch.randn(S, 8 * 5 * 4 * 2, generator=g) * sigma
        logit = torch.randn(S, 8 * 20, generator=g) * 2.0
        offw32 = torch.cat([off, logit], 1).contiguous().to(DEV)
        for offw in (offw32, offw32.to(torch.float16)):
            monkeypatch.setenv("APE_MSDA_LDS", "1")
            got = ops.msda_fused(value, shapes, starts, offw, ref, out_dtype=out_dt)
            monkeypatch.setenv("APE_MSDA_LDS", "0")
            quad = ops.msda_fused(value, shapes, starts, offw, ref, out_dtype=out_dt)
            want = ref_ops.msda_fused(value, shapes, starts, offw.float(), ref, out_dtype=torch.float32)
            e, eq = relerr(got, want), relerr(got, quad)
            n0 = shapes[0][0] * shapes[0][1]
            assert torch.equal(got[n0:], quad[n0:])                          # the coarser levels' queries take the quad kernel either way
            print(f"msda LDS-staged {shapes[0]} {out_dt} {name} offsets {offw.dtype}: vs definition {e:.3e}, vs quad kernel {eq:.3e}")
            assert e < TOL[out_dt] and eq < TOL[out_dt], (name, e, eq)
    monkeypatch.delenv("APE_MSDA_LDS", raising=False)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.float16])
def test_ms_deform_attn_forward_operator(ops, dtype):
    """the reference operator signature (ape/layers/csrc/vision.cpp:76-79) incl. batch > 1"""
    shapes = [(24, 32), (12, 16), (6, 8), (3, 4), (2, 2)]
    B, Q = 2, 517
    S = sum(h * w for h, w in shapes)
    value = rnd(B, S, 8, 32, dtype=dtype, seed=1)
    g = torch.Generator().manual_seed(3)
    loc = (torch.rand(B, Q, 8, 5, 4, 2, generator=g) * 1.2 - 0.1).to(dtype).to(DEV)
    aw = torch.rand(B, Q, 8, 20, generator=g).softmax(-1).reshape(B, Q, 8, 5, 4).to(dtype).to(DEV)
    ss = torch.tensor(shapes, dtype=torch.long, device=DEV)
    lsi = torch.cat((ss.new_zeros((1,)), ss.prod(1).cumsum(0)[:-1]))
    got = ops.ms_deform_attn_forward(value, ss, lsi, loc, aw, 64)
    want = ref_ops.ms_deform_attn_forward(value, ss, lsi, loc, aw, 64)
    e = relerr(got, want)
    print(f"ms_deform_attn_forward {dtype}: {e:.3e}")
    tol = {torch.bfloat16: TOL[torch.bfloat16], torch.float16: 1e-3, torch.float32: 1e-5}[dtype]     # one rounding of the output
    assert got.shape == (B, Q, 256) and got.dtype == dtype and e < tol
    if not SELF:
        # the torch operator the reference calls (ape/layers/csrc/vision.cpp:76-79; multi_scale_deform_attn.py:33-43)
        import ape_amd.layers  # noqa: F401  (registers torch.ops.ape.ms_deform_attn_forward)
        got2 = torch.ops.ape.ms_deform_attn_forward(value, ss, lsi, loc, aw, 64)
        assert torch.equal(got2, got)


def poisoned_vt(E, batch, stride, n, dtype, seed):
    """V^T [E, (batch-1)*stride + round_up(n, 64)] -- exactly the columns ops.attention may read -- as a view into a wider
    allocation whose remaining columns are NaN: a kernel that reads past the documented bound turns its output into NaN."""
    rows = batch * stride
    need = (batch - 1) * stride + (n + 63) // 64 * 64
    big = torch.full((E, need + 64), float("nan"), dtype=dtype, device=DEV)
    vt = big[:, :need]
    vt.zero_()
    vt[:, : min(rows, need)] = rnd(E, rows, dtype=dtype, seed=seed)[:, : min(rows, need)]
    return vt


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("B,N,H,HD", [(4, 1024, 16, 64), (1, 4096, 16, 64), (1, 900, 8, 32), (2, 200, 3, 64), (1, 77, 2, 32),
                                      (1, 4096, 16, 128), (4, 1024, 16, 128), (3, 72, 2, 128), (4, 256, 2, 128), (1, 1024, 2, 128)])     # 128: ViT-e (112 zero-padded)
def test_attention(ops, dtype, B, N, H, HD):
    if dtype == torch.float32 and N > 2048:
        pytest.skip("f32 validation kernel: keep the case small")
    E = H * HD
    qk = rnd(B * N, 2 * E + 64, dtype=dtype, seed=1)
    q, k = qk[:, :E], qk[:, E:2 * E]
    vt = poisoned_vt(E, B, N, N, dtype, 2)
    scale = HD ** -0.5
    got = ops.attention(q, k, vt, batch=B, n=N, heads=H, head_dim=HD, scale=scale)
    want = ref_ops.attention(q, k, vt, batch=B, n=N, heads=H, head_dim=HD, scale=scale)
    e = relerr(got, want)
    print(f"attention {dtype} B{B} N{N} H{H} HD{HD}: {e:.3e}")
    assert e < T16(dtype, 1e-2, 2e-5)
    # peaked softmax (forces the online-softmax rescale path): one dominant key per query row
    qs = q.clone()
    qs[::3] *= 12.0
    got = ops.attention(qs, k, vt, batch=B, n=N, heads=H, head_dim=HD, scale=scale)
    want = ref_ops.attention(qs, k, vt, batch=B, n=N, heads=H, head_dim=HD, scale=scale)
    e = relerr(got, want)
    print(f"attention(peaked) {dtype}: {e:.3e}")
    assert e < T16(dtype, 2e-2, 2e-5)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("B,N,H,HDQ", [(2, 1024, 4, 256), (1, 4096, 2, 256), (1, 2304, 2, 288), (1, 1000, 2, 320), (3, 200, 4, 256)])
def test_attention_wide_keys(ops, dtype, B, N, H, HDQ):
    """q.k width 256 / 288 / 320 over a V width of 128 (ape_hip_attention_ext): the operands of the EVA-01 MIM ViT's global blocks,
    whose relative-position terms ride as extra q / k channels (vit_eva.py:121-146)"""
    if dtype == torch.float32 and N > 2048:
        pytest.skip("f32 validation kernel: keep the case small")
    HDV = 128
    q = rnd(B * N, H * HDQ, dtype=dtype, seed=1)
    k = rnd(B * N, H * HDQ, dtype=dtype, seed=3)
    vt = poisoned_vt(H * HDV, B, N, N, dtype, 2)
    scale = HDQ ** -0.5
    kw = dict(batch=B, n=N, heads=H, head_dim=HDQ, v_head_dim=HDV, scale=scale)
    got = ops.attention(q, k, vt, **kw)
    want = ref_ops.attention(q, k, vt, **kw)
    assert tuple(got.shape) == (B * N, H * HDV)
    e = relerr(got, want)
    print(f"attention wide {dtype} B{B} N{N} H{H} HDQ{HDQ}: {e:.3e}")
    assert e < T16(dtype, 1e-2, 2e-5)
    qs = q.clone()
    qs[::3] *= 12.0
    e = relerr(ops.attention(qs, k, vt, **kw), ref_ops.attention(qs, k, vt, **kw))
    print(f"attention wide (peaked) {dtype}: {e:.3e}")
    assert e < T16(dtype, 2e-2, 2e-5)
    if not SELF:
        with pytest.raises(RuntimeError):                                  # widths outside the instantiated set are refused
            ops.attention(q[:, :H * 192], k[:, :H * 192], vt, batch=B, n=N, heads=H, head_dim=192, v_head_dim=HDV, scale=scale)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("rows,nh,hd,hs,g,ext,period", [(1024, 4, 88, 128, 16, 128, 256), (2048, 2, 88, 128, 32, 256, 1024), (512, 3, 64, 64, 16, 128, 256)])
def test_relpos_extend(ops, dtype, rows, nh, hd, hs, g, ext, period):
    """q_ext = [scale q | q.Rh[ty - kh] | q.Rw[tx - kw] | 0], k_ext = [k | one-hot ty | one-hot tx | 0] (csrc/relpos.hip) -- a pure
    gather / scale: exact up to the one rounding of scale q; and its dot product reproduces add_decomposed_rel_pos
    (utils_eva.py:132-161) on the scores"""
    qk = rnd(rows, 2 * nh * hs, dtype=dtype, seed=1)
    q, k = qk[:, :nh * hs], qk[:, nh * hs:]
    nr = 2 * (2 * g - 1)
    tper = 2 * nh
    t = rnd(rows * tper, nr + 2, dtype=dtype, seed=2)
    perm = torch.randperm(period, generator=torch.Generator().manual_seed(0))
    ty = (perm // g % g).int().to(DEV).contiguous()
    tx = (perm % g).int().to(DEV).contiguous()
    kw = dict(heads=nh, head_stride=hs, head_dim=hd, hk=g, wk=g, ext_dim=ext, scale=hd ** -0.5, t_rows_per_token=tper)
    qe, ke = ops.relpos_extend(q, k, t, ty, tx, **kw)
    qw, kw_ = ref_ops.relpos_extend(q, k, t, ty, tx, **kw)
    assert tuple(qe.shape) == (rows, nh * ext)
    assert torch.equal(ke, kw_)
    e = relerr(qe, qw)
    print(f"relpos_extend {dtype} rows{rows} nh{nh} g{g} ext{ext}: q_ext {e:.2e}, k_ext exact")
    assert e < T16(dtype, 4e-3, 1e-6)
    if dtype == torch.float32:
        # one attention group, end to end vs the reference formulation: t = q . [Rh ; Rw]^T
        R = rnd(nr, hd, dtype=dtype, seed=5)
        n = g * g
        qh = q[:n].reshape(n, nh, hs)[..., :hd]
        kh = k[:n].reshape(n, nh, hs)[..., :hd]
        tt = torch.zeros((n * tper, nr), device=DEV)
        tt.view(n, tper, nr)[:, :nh] = qh @ R.t()
        yy = (torch.arange(n, device=DEV) // g).int().contiguous()
        xx = (torch.arange(n, device=DEV) % g).int().contiguous()
        qe, ke = ops.relpos_extend(q[:n], k[:n], tt, yy, xx, **kw)
        scores = torch.einsum("qhc,khc->hqk", qe.view(n, nh, ext), ke.view(n, nh, ext))
        Rh, Rw = R[:2 * g - 1], R[2 * g - 1:]
        idx = (torch.arange(g, device=DEV)[:, None] - torch.arange(g, device=DEV)[None, :]) + g - 1
        rel_h = torch.einsum("qhc,qkc->hqk", qh, Rh[idx][yy.long()])                      # [nh, n, g]: q . Rh[qy - ky]
        rel_w = torch.einsum("qhc,qkc->hqk", qh, Rw[idx][xx.long()])
        want = (hd ** -0.5) * torch.einsum("qhc,khc->hqk", qh, kh) + rel_h[:, :, yy.long()] + rel_w[:, :, xx.long()]
        e = relerr(scores, want)
        print(f"relpos_extend: q_ext . k_ext vs scale q.k + decomposed relative positions: {e:.2e}")
        assert e < 1e-5


def test_attention_kernel_variants_agree(ops, monkeypatch):
    """the opt-in 256-query kernel (APE_ATTN_QT4=1) computes every query with the 128-query kernel's arithmetic: bit-identical
    outputs, incl. ragged last tiles (N % 64 != 0), single-tile and two-tile sequences"""
    for (B, N, H, HD) in [(2, 4096, 16, 64), (8, 1024, 16, 64), (40, 200, 16, 64), (1, 4096, 16, 64), (4, 1000, 16, 64), (1, 5000, 16, 64),
                           (600, 56, 16, 64), (300, 120, 16, 64)]:
        E = H * HD
        qk = rnd(B * N, 2 * E, dtype=torch.bfloat16, seed=1)
        q, k = qk[:, :E], qk[:, E:]
        vt = poisoned_vt(E, B, N, N, torch.bfloat16, 2)
        kw = dict(batch=B, n=N, heads=H, head_dim=HD, scale=HD ** -0.5)
        monkeypatch.setenv("APE_ATTN_QT4", "0")
        base = ops.attention(q, k, vt, **kw)
        monkeypatch.setenv("APE_ATTN_QT4", "1")
        qt4 = ops.attention(q, k, vt, **kw)
        want = ref_ops.attention(q, k, vt, **kw)
        e = relerr(base, want)
        print(f"attention variants B{B} N{N}: 128-query kernel {e:.3e} vs definition; 256-query kernel differs by {relerr(qt4, base):.1e}")
        assert e < 1e-2 and torch.equal(qt4, base)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_attention_strided_windows(ops, dtype):
    """windows of 196 tokens stored at a stride of 200 rows (APE-Ti: zero-padded 14 x 14 windows, vit_eva02.py:437-458):
    the 4 slack rows of a window are neither queries nor keys"""
    B, N, S, H, HD = 25, 196, 200, 3, 64
    E = H * HD
    qk = rnd(B * S, 2 * E, dtype=dtype, seed=1)
    q, k = qk[:, :E], qk[:, E:]
    vt = poisoned_vt(E, B, S, N, dtype, 2)
    with (pytest.raises(ValueError) if not SELF else __import__("contextlib").nullcontext()):          # one column short of the documented bound is refused, not over-read
        ops.attention(q, k, vt[:, :-1], batch=B, n=N, heads=H, head_dim=HD, scale=HD ** -0.5, stride=S)
    got = ops.attention(q, k, vt, batch=B, n=N, heads=H, head_dim=HD, scale=HD ** -0.5, stride=S)
    want = ref_ops.attention(q, k, vt, batch=B, n=N, heads=H, head_dim=HD, scale=HD ** -0.5, stride=S)
    rows = (torch.arange(B * S) % S < N).to(DEV)
    assert torch.isfinite(got[rows].float()).all()
    e = relerr(got[rows], want[rows])
    print(f"attention strided {dtype}: {e:.3e}")
    assert e < T16(dtype, 1e-2, 2e-5)


# ------------------------------------------------------------------------------------------------ set 2
def _wm_perm(ht, wt, ws):
    """window-major token order: tok -> raster index, and the inverse"""
    r = torch.arange(ht * wt).view(ht // ws, ws, wt // ws, ws).permute(0, 2, 1, 3).reshape(-1)
    inv = torch.empty_like(r)
    inv[r] = torch.arange(ht * wt)
    return r.int(), inv.int()


@pytest.mark.parametrize("odt", [torch.bfloat16, torch.float16, torch.float32])
def test_patchify(ops, odt):
    ht = wt = 16
    img = torch.randint(0, 256, (3, 200, 144), generator=torch.Generator().manual_seed(1)).float().to(DEV)
    t2r, _ = _wm_perm(ht, wt, 8)
    mean, std = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
    for perm in (None, t2r.to(DEV)):
        got = ops.patchify(img, perm, ht, wt, mean, std, out_dtype=odt)
        ref = ref_ops.patchify(img, perm, ht, wt, mean, std, out_dtype=odt)
        assert got.shape == (256, 768) and relerr(got, ref) < 1e-6


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
def test_spatial_gathers(ops, dt):
    H = W = 32
    C = 64
    x = rnd(H * W, C, dtype=dt, seed=1)
    _, r2t = _wm_perm(H, W, 8)
    for perm in (None, r2t.to(DEV)):
        assert torch.equal(ops.im2col3x3(x, perm, H, W).float(), ref_ops.im2col3x3(x, perm, H, W).float())
        assert torch.equal(ops.maxpool2x2(x, perm, H, W).float(), ref_ops.maxpool2x2(x, perm, H, W).float())
    idx = torch.randint(0, H * W, (777,), generator=torch.Generator().manual_seed(2)).int().to(DEV)
    assert torch.equal(ops.gather_rows(x, idx).float(), ref_ops.gather_rows(x, idx).float())


def _rand_boxes(n, seed, size=1.0, jitter=0.02):
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(n // 4 + 1, 2, generator=g)
    c = c[torch.randint(0, len(c), (n,), generator=g)] + torch.randn(n, 2, generator=g) * jitter  # clustered -> overlaps
    wh = (torch.rand(n, 2, generator=g) * 0.2 + 0.05)
    return (torch.cat([c - wh / 2, c + wh / 2], 1) * size).float().contiguous()


def test_nms_segments(ops):
    g = torch.Generator().manual_seed(5)
    n = 3000
    boxes = _rand_boxes(n, 1)
    scores = torch.rand(n, generator=g)
    levels = torch.randint(0, 5, (n,), generator=g)
    order = torch.argsort(scores, descending=True, stable=True)
    order = order[torch.argsort(levels[order], stable=True)]  # group-major, score-descending inside
    b, lv = boxes[order].contiguous().to(DEV), levels[order].int().to(DEV)
    counts = torch.bincount(levels, minlength=5)
    seg = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]).int().to(DEV)
    valid = (torch.rand(n, generator=g) > 0.1).to(torch.uint8).to(DEV)
    for v in (None, valid):
        got = ops.nms_segments(b, lv, seg, int(counts.max()), 0.6, v)
        ref = ref_ops.nms_segments(b, lv, seg, int(counts.max()), 0.6, v)
        print("nms_segments kept", int(got.sum()), "of", n)
        assert torch.equal(got.cpu(), ref.cpu())
    # one segment holding mixed groups (the p6 "extras" case): suppression must respect group ids
    seg1 = torch.tensor([0, n], dtype=torch.int32).to(DEV)
    o2 = torch.argsort(scores, descending=True, stable=True)
    b2, lv2 = boxes[o2].contiguous().to(DEV), levels[o2].int().to(DEV)
    assert torch.equal(ops.nms_segments(b2, lv2, seg1, n, 0.6).cpu(), ref_ops.nms_segments(b2, lv2, seg1, n, 0.6).cpu())


def test_nms_classes(ops):
    g = torch.Generator().manual_seed(6)
    n, K = 900, 37
    boxes = _rand_boxes(n, 2, size=1024.0).to(DEV)
    scores = torch.rand(n, K, generator=g)
    order = torch.argsort(scores, dim=0, descending=True, stable=True).t().contiguous().int().to(DEV)
    valid = (torch.gather(scores.t(), 1, order.cpu().long()) > 0.05).to(torch.uint8).contiguous().to(DEV)
    got = ops.nms_classes(boxes, order, 0.7, valid)
    ref = ref_ops.nms_classes(boxes, order, 0.7, valid)
    print("nms_classes kept", int(got.sum()), "of", n * K)
    assert torch.equal(got.cpu(), ref.cpu())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
def test_vl_pool(ops, dt):
    T = 5456
    S = rnd(T, 8, seed=1) * 3.0
    x = rnd(T, 256, dtype=dt, seed=2)
    e = relerr(ops.vl_pool(S, x), ref_ops.vl_pool(S, x))
    print("vl_pool", dt, e)
    assert e < 2e-5


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("T,L", [(341, 9), (5456, 256), (1000, 300)])
def test_dense_fusion_softmaxes(ops, dt, T, L):
    """segment_softmax / col_softmax_t / transpose (csrc/softmax.hip) vs fuse_helper.py:89-131 in torch"""
    nh = 8
    S = rnd(T, nh * L, seed=3) * 4.0
    S[0, 0] = -80000.0                       # exercises the +-5e4 clamp after the global-max subtraction
    gmax = S.max().reshape(1)
    pv = ops.segment_softmax(S, nh, gmax, dt)
    ref = ref_ops.segment_softmax(S, nh, gmax, torch.float32)
    e1 = relerr(pv, ref)
    assert pv.shape == (T, nh * L) and pv.dtype == dt
    assert (pv.float().reshape(T, nh, L).sum(-1) - 1).abs().max().item() < T16(dt, 2e-2, 1e-5)
    pl = ops.col_softmax_t(S, gmax, dt, pad=8)
    refl = ref_ops.col_softmax_t(S, gmax, torch.float32, pad=8)
    e2 = relerr(pl, refl)
    Tp = (T + 7) // 8 * 8
    assert pl.shape == (nh * L, Tp) and pl.dtype == dt and (pl[:, T:] == 0).all()
    x = rnd(T, 256, dtype=dt, seed=4)
    xt = ops.transpose(x, pad=8)
    assert xt.shape == (256, Tp) and torch.equal(xt[:, :T].cpu(), x.t().cpu()) and (xt[:, T:] == 0).all()
    print(f"dense fusion softmaxes {dt} T={T} L={L}: vision {e1:.2e} language {e2:.2e}")
    tol = T16(dt, 5e-3, 1e-4) if dt != torch.float16 else 1e-3          # device expf vs libm over a 5456-term online sum
    assert e1 < tol and e2 < tol


def test_mask_postprocess(ops):
    n, h0, S = 7, 64, 256
    logits = rnd(n, h0 * h0, seed=1)
    # smooth the logits so masks have structure
    logits = F_avg(logits.view(n, 1, h0, h0)).reshape(n, h0 * h0).contiguous()
    bits = ops.mask_upsample_bits(logits, h0, h0, S)
    ref = ref_ops.mask_upsample_bits(logits, h0, h0, S)
    mism = (bits != ref).float().mean().item()
    print("upsample mismatch", mism)
    assert mism < 1e-5
    boxes = _rand_boxes(n, 3, size=200.0).to(DEV) + 10
    boxes[0] = torch.tensor([-5.0, 3.0, 300.0, 100.0])  # partly outside
    r = ops.roi_align_bits(ref.contiguous(), boxes, 128)
    rr_ = ref_ops.roi_align_bits(ref, boxes, 128)
    mism = (r != rr_).float().mean().item()
    print("roi_align mismatch", mism)
    assert mism < 1e-4
    ob = boxes * 1.5
    p = ops.paste_bits(rr_.contiguous(), ob.contiguous(), 300, 420)
    pr = ref_ops.paste_bits(rr_, ob, 300, 420)
    mism = (p != pr).float().mean().item()
    print("paste mismatch", mism)
    assert mism < 1e-4


def F_avg(t):
    import torch.nn.functional as F
    return F.avg_pool2d(F.pad(t, (2, 2, 2, 2), mode="replicate"), 5, 1)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
def test_semantic_kernels(ops, dt):
    """mask_upsample_sigmoid (pixel-major, cropped) and bilinear_resize vs F.interpolate"""
    h0, w0, S, n = 24, 24, 96, 20
    lt = rnd(h0 * w0, n, seed=5) * 3.0
    got = ops.mask_upsample_sigmoid(lt, h0, w0, S, 70, 93, dt)
    ref = ref_ops.mask_upsample_sigmoid(lt, h0, w0, S, 70, 93, torch.float32)
    assert got.shape == (70 * 93, n) and got.dtype == dt
    e = relerr(got, ref)
    x = rnd(5, 70, 93, seed=6)
    e2 = relerr(ops.bilinear_resize(x, 105, 140), ref_ops.bilinear_resize(x, 105, 140))
    e3 = relerr(ops.bilinear_resize(x[:, :33, :40], 20, 17), ref_ops.bilinear_resize(x[:, :33, :40], 20, 17))   # strided view, downscale
    print("semantic kernels", dt, e, e2, e3)
    assert e < T16(dt, 5e-3, 1e-5) and e2 < 1e-5 and e3 < 1e-5
    if not SELF:
        # the vector kernel (8 queries per thread, 16-byte stores; n % 8 == 0) against the scalar kernel: the same arithmetic per element,
        # bit-identical outputs -- incl. more than 512 queries (a lane's second trip) and a crop that is not a multiple of the pixel quad
        import os
        for (h1, w1, S1, n1, ch, cw) in [(24, 24, 96, 24, 70, 93), (16, 20, 64, 1032, 33, 61), (96, 96, 384, 504, 40, 384)]:
            lt1 = rnd(h1 * w1, n1, seed=7) * 3.0
            os.environ["APE_MASK_UP8"] = "0"
            try:
                scalar = ops.mask_upsample_sigmoid(lt1, h1, w1, S1, ch, cw, dt)
            finally:
                os.environ.pop("APE_MASK_UP8")
            vec = ops.mask_upsample_sigmoid(lt1, h1, w1, S1, ch, cw, dt)
            assert torch.equal(vec, scalar), (h1, w1, n1, ch, cw)


@pytest.mark.parametrize("K,nt", [(134, 80), (20, 3), (1203, 1), (65, 65)])
def test_class_score_kernels(ops, K, nt):
    """stuff_collapse / sem_class_weights / pan_class_scores / argmax_labels (csrc/softmax.hip) vs their tensor-level definitions
    (deformable_detr_segm_vl.py:1251-1271, :891-894, :944-949): values to fp32 rounding, labels / keep flags / argmax IDENTICAL"""
    Q, k = 900, 300
    g = torch.Generator().manual_seed(K)
    logits = (torch.randn(Q, K, generator=g) * 3.0 - 2.0).to(DEV)
    logits[5, :] = logits[5, 0]                                       # a row of ties: first index wins
    qidx = torch.randperm(Q, generator=g)[:k].to(DEV)
    vscore = torch.where(torch.rand(k, generator=g) < 0.1, torch.tensor(-1.0), torch.rand(k, generator=g)).to(DEV)
    got, want = ops.stuff_collapse(logits, nt), ref_ops.stuff_collapse(logits, nt)
    assert torch.equal(got, want)
    kp = (k + 7) // 8 * 8
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        for v in (vscore, None):
            A, B = ops.sem_class_weights(got, qidx, v, 0.06, kp, dt), ref_ops.sem_class_weights(want, qidx, v, 0.06, kp, dt)
            assert A.shape == B.shape == (K - nt + 1, kp) and A.dtype == dt
            assert relerr(A, B) < T16(dt, 5e-3, 2e-6), (dt, relerr(A, B))
            assert float(A[:, k:].abs().max()) == 0.0
    for transform in (False, True):
        for q, v in ((qidx, vscore), (None, None)):
            s1, l1, k1, l32 = ops.pan_class_scores(logits, q, v, 0.3, transform, 0.06)
            s2, l2, k2, _ = ref_ops.pan_class_scores(logits, q, v, 0.3, transform, 0.06)
            assert torch.equal(l1, l2) and torch.equal(k1, k2) and torch.equal(l32.long(), l2) and relerr(s1, s2) < 2e-6
    x = rnd(K, 37, 53, seed=3)
    x[:, 4, 4] = 1.0                                                  # ties -> class 0
    assert torch.equal(ops.argmax_labels(x), ref_ops.argmax_labels(x))
    assert torch.equal(ops.argmax_labels(x, class0=0.25), ref_ops.argmax_labels(x, class0=0.25))
    print(f"class score kernels K={K} nt={nt}: ok")


def test_box_refine(ops):
    Q, L = 900, 5
    g = torch.Generator().manual_seed(5)
    ref = torch.rand(Q, 4, generator=g).to(DEV)
    ref[0] = torch.tensor([0.0, 1.0, 1e-5, 0.99999])          # the eps clamps of inverse_sigmoid
    big = rnd(Q, 8, seed=6) * 2.0
    delta = big[:, 2:6]                                       # strided rows (ld 8)
    vr4 = torch.rand(L, 4, generator=g).to(DEV)
    for d in (delta, None):
        got_ref, got_in = ops.box_refine(d, ref, vr4)
        want_ref, want_in = ref_ops.box_refine(d, ref, vr4)
        assert got_in.shape == (Q, L, 4)
        assert relerr(got_ref, want_ref) < 1e-6 and relerr(got_in, want_in) < 1e-6


def test_language_side_epilogues(ops):
    """the element-wise tails of the single-token language side inside the small kernels (no tensor-library launches):
    gemv scale / add, head_gemv bf16 copy, vl_pool subtract"""
    x, w, b = rnd(1, 2048, seed=1), rnd(256, 2048, scale=1 / 45, seed=2), rnd(256, seed=3)
    sc, add = rnd(256, seed=4), rnd(1, 256, seed=5)
    got, got2 = ops.gemv(x, w, b, alpha=0.7, scale=sc, add=add)
    want, want2 = ref_ops.gemv(x, w, b, alpha=0.7, scale=sc, add=add)
    assert relerr(got, want) < 2e-5 and relerr(got2, want2) < 2e-5
    assert torch.equal(got2, add + got)                                    # out2 is add + the ROUNDED out
    only = ops.gemv(x, w, b, alpha=0.7, scale=sc)
    assert torch.equal(only, got)
    g3, g4 = ops.gemv(x, w, None, alpha=-0.125, add=add)
    w3, w4 = ref_ops.gemv(x, w, None, alpha=-0.125, add=add)
    assert relerr(g3, w3) < 2e-5 and relerr(g4, w4) < 2e-5
    xh, wh = rnd(8, 256, seed=6), rnd(8, 256, 256, scale=1 / 16, seed=7)
    u, uc = ops.head_gemv(xh, wh, bf16_copy=True)
    assert uc.dtype == torch.bfloat16 and torch.equal(uc, u.to(torch.bfloat16)) and torch.equal(u, ops.head_gemv(xh, wh))
    T = 5456
    S, xv, sub = rnd(T, 8, seed=8) * 3.0, rnd(T, 256, dtype=torch.bfloat16, seed=9), rnd(256, seed=10)
    e = relerr(ops.vl_pool(S, xv, sub), ref_ops.vl_pool(S, xv, sub))
    assert e < 2e-5, e


@pytest.mark.parametrize("C", [224, 1792, 2048])
@pytest.mark.parametrize("tdt,cdt", [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16), (torch.float32, None)])
def test_postnorm_residual(ops, C, tdt, cdt):
    """x <- x + LayerNorm(t) on the fp32 stream in place + the copy in the GEMM operand type (ViT-e post-norm blocks)"""
    M = 1037
    x = rnd(M, C, seed=1) * 3.0
    t = (rnd(M, C, seed=2) * 2.0 + 0.4).to(tdt)
    norm = (rnd(C, seed=3) + 1.0, rnd(C, seed=4), 1e-6)
    want = x.clone()
    wcopy = ref_ops.postnorm_residual(want, t, norm, copy_dtype=cdt)
    got = x.clone()
    copy = ops.postnorm_residual(got, t, norm, copy_dtype=cdt)
    assert relerr(got, want) < 2e-5
    if cdt is None:
        assert copy is None
    else:
        assert copy.dtype == cdt and torch.equal(copy, got.to(cdt))
    only = ops.postnorm_residual(got, None, None, copy_dtype=torch.bfloat16)      # t = None: only the copy
    assert torch.equal(only, got.to(torch.bfloat16))


@pytest.mark.parametrize("bf", H16)
def test_gather_rows_int64_indices(ops, bf):
    x = rnd(5000, 256, dtype=bf, seed=1)
    idx = torch.randint(0, 5000, (900,), generator=torch.Generator().manual_seed(2)).to(DEV)
    assert torch.equal(ops.gather_rows(x, idx), x[idx])
    assert torch.equal(ops.gather_rows(x, idx.to(torch.int32)), x[idx])
    m = torch.randint(0, 255, (100, 128, 128), generator=torch.Generator().manual_seed(3), dtype=torch.uint8).to(DEV)
    order = torch.randperm(100, generator=torch.Generator().manual_seed(4)).to(torch.int32).to(DEV)
    got = ops.gather_rows(m.view(100, -1).view(torch.float32), order).view(torch.uint8).view(m.shape)
    assert torch.equal(got, m[order.long()])                               # byte rows moved as 16-byte pieces: a pure copy
    # rows of any width (class-score rows [Q, K] with K = 133 / 1203: the panoptic branch gathers its kept queries' logits) and strided views
    for dt in (torch.float32, bf):
        for C in (133, 1203, 7):
            y = rnd(900, C, dtype=dt, seed=5)
            assert torch.equal(ops.gather_rows(y, idx[:300] % 900), y[idx[:300] % 900])
        z = rnd(900, 144, dtype=dt, seed=6)[:, :133]                              # row stride 144, 133 columns
        assert torch.equal(ops.gather_rows(z, idx[:300] % 900), z[idx[:300] % 900])


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
def test_query_init_and_finish(ops, dt):
    """two-stage query initialisation (deformable_transformer_vl.py:412-420, 629-645) in two launches"""
    from ape_amd.modeling.ape_deta.geometry import dim_t_table
    T, Q, E = 21824, 900, 256
    coords = rnd(T, 4, seed=1) * 3.0
    topk = torch.randint(0, T, (Q,), generator=torch.Generator().manual_seed(2)).to(DEV)
    dim_t = dim_t_table(128, 10000, DEV)
    ref, pe, t32 = ops.query_init(coords, topk, dim_t, dt)
    wref, wpe, wt32 = ref_ops.query_init(coords, topk, dim_t, dt)
    assert torch.equal(t32, wt32) and pe.dtype == dt and pe.shape == (Q, 512)
    assert (ref - wref).abs().max().item() < 1e-6
    # sin / cos of arguments up to 2 pi: device libm vs the tensor library's, a few ulp; bf16 adds one rounding
    assert (pe.float() - wpe.float()).abs().max().item() < T16(dt, 8e-3, 1e-5)
    pos, pix = rnd(Q, 2 * E, seed=3) * 2.0 + 0.3, rnd(Q, E, seed=4) * 1.5 - 0.2
    npos = (rnd(2 * E, seed=5) + 1.0, rnd(2 * E, seed=6), 1e-5)
    npix = (rnd(E, seed=7) + 1.0, rnd(E, seed=8), 1e-5)
    got = ops.query_finish(pos, pix, npos, npix, dt)
    want = ref_ops.query_finish(pos, pix, npos, npix, dt)
    for g, w, name in zip(got, want, ("query_pos", "query", "query + query_pos")):
        e = relerr(g, w)
        print(f"query_finish {name} {dt}: {e:.3e}")
        assert g.dtype == dt and e < TOL[dt], (name, e)
    assert torch.equal(got[2], (got[1].float() + got[0].float()).to(dt))   # from the rounded outputs, like the decoder's expression


@pytest.mark.parametrize("k", [1, 100, 300, 1000, 2500])
def test_det_records(ops, k):
    """boxes to the output frame + clip + keep + kept-first stable partition in one launch vs the tensor-level definition"""
    g = torch.Generator().manual_seed(k)
    b = torch.rand(k, 4, generator=g) * 900.0
    b[:, 2:] = b[:, :2] + torch.rand(k, 2, generator=g) * 300.0 - 20.0          # some empty boxes (x2 <= x1)
    scores = torch.rand(k, generator=g)
    scores[torch.rand(k, generator=g) < 0.2] = -1.0                            # empty slots
    classes = torch.randint(0, 1203, (k,), generator=g)
    query = torch.randint(0, 900, (k,), generator=g)
    frame = torch.tensor([0.75, 0.6, 0.75, 0.6, 640.0, 480.0, 640.0, 480.0])
    args = [t.to(DEV) for t in (b, scores, classes, query, frame)]
    rec, boxes, order = ops.det_records(*args)
    wrec, wboxes, worder = ref_ops.det_records(*args)
    assert torch.equal(order, worder) and torch.equal(rec, wrec) and torch.equal(boxes, wboxes)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_gemm_folded_layernorm(ops, dtype):
    """row_stats + gemm(rownorm=...) == LayerNorm(h) @ W^T + b  (the SwiGLU sub-LN folded into the down projection)"""
    M, C, Cp, N = 1000, 2730, 2752, 1024
    h = torch.zeros(M, Cp)
    h[:, :C] = torch.randn(M, C, generator=torch.Generator().manual_seed(1)) * 2.0 + 0.3
    h = h.to(dtype).to(DEV)
    g = (1.0 + 0.1 * torch.randn(C, generator=torch.Generator().manual_seed(2))).to(DEV)
    b = (0.1 * torch.randn(C, generator=torch.Generator().manual_seed(3))).to(DEV)
    w = (torch.randn(N, C, generator=torch.Generator().manual_seed(4)) / C ** 0.5).to(DEV)
    bias = rnd(N, seed=5)
    res = rnd(M, N, seed=6)
    eps = 1e-6
    rs, sh = ops.row_stats(h[:, :C], eps)
    rrs, rsh = ref_ops.row_stats(h[:, :C], eps)
    assert relerr(rs, rrs) < 1e-5 and relerr(sh, rsh) < 1e-4
    wf = torch.zeros(N, Cp, device=DEV)
    wf[:, :C] = w * g[None, :]
    wf = wf.to(dtype)
    c1 = wf.float().sum(1).contiguous()
    c2 = (w @ b + bias).contiguous()
    got = ops.gemm(h, wf, c2, residual=res, rownorm=(rs, sh, c1), out_dtype=torch.float32)
    want = torch.nn.functional.layer_norm(h[:, :C].float(), (C,), g, b, eps) @ w.t() + bias + res
    e = relerr(got, want)
    print(f"folded LayerNorm GEMM {dtype}: {e:.3e}")
    assert e < T16(dtype, 1.5e-2, 1e-4)
    # split-K path applies the row terms in the reduce kernel only
    if dtype in H16:
        got2 = ops.gemm(h, wf, c2, residual=res, rownorm=(rs, sh, c1), out_dtype=torch.float32, splitk=2, tile64=0)
        assert relerr(got2, got) < 1e-5


@pytest.mark.parametrize("dtype", H16)
def test_gemm_rowstats_in_launch(ops, dtype, monkeypatch):
    """gemm(rowstats=...): the folded LayerNorm's row statistics computed by the 256 x 128 tile kernel itself (ApeGemmArgs.rowstat_cols)
    == row_stats + gemm(rownorm=...) up to fp32 summation order == LayerNorm(a) @ W^T + b; fp32 / 16-bit outputs, with and without
    residual, a ragged last row tile, K padding, and the fallback where the tile kernel does not apply"""
    eps = 1e-6
    for M, C, Cp, N, mean in ((8192, 2730, 2752, 1024, 0.3), (8000, 1024, 1024, 1024, -0.2), (6500, 512, 512, 1280, 1.5)):
        h = torch.zeros(M, Cp)
        h[:, :C] = torch.randn(M, C, generator=torch.Generator().manual_seed(1)) * 2.0 + mean
        h = h.to(dtype).to(DEV)
        g = (1.0 + 0.1 * torch.randn(C, generator=torch.Generator().manual_seed(2))).to(DEV)
        b = (0.1 * torch.randn(C, generator=torch.Generator().manual_seed(3))).to(DEV)
        w = (torch.randn(N, C, generator=torch.Generator().manual_seed(4)) / C ** 0.5).to(DEV)
        bias = rnd(N, seed=5)
        res = rnd(M, N, seed=6)
        wf = torch.zeros(N, Cp, device=DEV)
        wf[:, :C] = w * g[None, :]
        wf = wf.to(dtype)
        c1 = wf.float().sum(1).contiguous()
        c2 = (w @ b + bias).contiguous()
        rs, sh = ops.row_stats(h[:, :C], eps)
        want = torch.nn.functional.layer_norm(h[:, :C].float(), (C,), g, b, eps) @ w.t() + bias
        for residual, odt in ((res, torch.float32), (None, dtype), (None, torch.float32)):
            two = ops.gemm(h, wf, c2, residual=residual, rownorm=(rs, sh, c1), out_dtype=odt, tile64=4)
            got = ops.gemm(h, wf, c2, residual=residual, rowstats=(C, eps, c1), out_dtype=odt)
            if not SELF:
                from ape_amd import _lib
                assert b"rowstat" in _lib.load().ape_hip_gemm_last_kernel(), (M, N, Cp)      # the case really took the in-launch path
            e2, e = relerr(got, two), relerr(got, want + (residual if residual is not None else 0))
            print(f"in-launch row statistics {dtype} {M}x{N}x{Cp} out {odt} residual {residual is not None}: vs row_stats path {e2:.2e}, vs LayerNorm definition {e:.2e}")
            assert e2 < (2e-5 if odt == torch.float32 else 4e-3) and e < T16(dtype, 1.5e-2, 1e-4)
    # where the tile kernel does not apply (few rows: another tiling) the statistics come from a row_stats launch -- same call, same result
    M, C, N = 1000, 512, 256
    h = (torch.randn(M, C, generator=torch.Generator().manual_seed(7)) + 0.5).to(dtype).to(DEV)
    wf = (torch.randn(N, C, generator=torch.Generator().manual_seed(8)) / C ** 0.5).to(dtype).to(DEV)
    c1, c2 = wf.float().sum(1).contiguous(), rnd(N, seed=9)
    rs, sh = ops.row_stats(h, eps)
    assert torch.equal(ops.gemm(h, wf, c2, rowstats=(C, eps, c1), out_dtype=torch.float32), ops.gemm(h, wf, c2, rownorm=(rs, sh, c1), out_dtype=torch.float32))
    monkeypatch.setenv("APE_NO_ROWSTAT", "1")
    M, C, N = 8192, 1024, 1024
    h = (torch.randn(M, C, generator=torch.Generator().manual_seed(7)) + 0.5).to(dtype).to(DEV)
    wf = (torch.randn(N, C, generator=torch.Generator().manual_seed(8)) / C ** 0.5).to(dtype).to(DEV)
    c1, c2 = wf.float().sum(1).contiguous(), rnd(N, seed=9)
    rs, sh = ops.row_stats(h, eps)
    assert torch.equal(ops.gemm(h, wf, c2, rowstats=(C, eps, c1), out_dtype=torch.float32), ops.gemm(h, wf, c2, rownorm=(rs, sh, c1), out_dtype=torch.float32))
    if not SELF:
        # the C ABI refuses the mode where no kernel implements it (a caller must not get a GEMM without the row terms)
        from ape_amd import _lib
        import ctypes
        a = _lib.GemmArgs()
        out = torch.empty((M, N), dtype=torch.float32, device=DEV)
        a.A, a.W, a.C, a.colvec = h.data_ptr(), wf.data_ptr(), out.data_ptr(), c1.data_ptr()
        a.M, a.N, a.K, a.lda, a.ldw, a.ldc = M, N, C, C, C, N
        a.in_dt, a.out_dt, a.alpha, a.rowstat_cols, a.rowstat_eps, a.tile64 = ops._dt(h), ops._dt(out), 1.0, C, eps, 0
        assert _lib.load().ape_hip_gemm(ctypes.byref(a), None) != 0 and b"rowstat_cols" in _lib.load().ape_hip_last_error()


@pytest.mark.parametrize("bf", H16)
@pytest.mark.parametrize("stagger", [0, 1])
@pytest.mark.parametrize("tile", [3, 4])
def test_gemm_p8(ops, tile, stagger, monkeypatch, bf):
    """256x256 / 256x128 eight-wave counted-wait kernel (gemm_p8.hip): every specialised epilogue, the generic one, ragged
    M / N edges, 1..many K tiles, transposed output (operand exchange), both barrier schedules"""
    monkeypatch.setenv("APE_GEMM_P8_STAGGER", str(stagger))

    def check(name, a, w, bias, tol=None, **kw):
        got = ops.gemm(a, w, bias, tile64=tile, **kw)
        if not SELF:
            from ape_amd import _lib
            assert b"p8" in _lib.load().ape_hip_gemm_last_kernel(), name      # the case really took the new kernel
        ref = ref_ops.gemm(a, w, bias, **kw)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        e = relerr(got, ref)
        odt = kw.get("out_dtype", bf)
        print(f"gemm p8 tile={tile} stagger={stagger} [{name}] M{a.shape[0]} N{w.shape[0]} K{a.shape[1]}: {e:.3e}")
        assert e < (tol or (TOL[bf] if odt == bf else 3e-4)), name

    for (M, N, K) in [(256, 256, 64), (512, 512, 128), (1000, 736, 320), (4096, 2048, 1024), (300, 136, 192), (87296, 256, 2048)]:
        a, w = rnd(M, K, dtype=bf, seed=1), rnd(N, K, dtype=bf, scale=K ** -0.5, seed=2)
        bias = rnd(N, seed=3)
        check("plain", a, w, bias)
        check("f32out_nobias", a, w, None, out_dtype=torch.float32)
        if M > 50000:
            check("res16", a, w, bias, residual=rnd(M, N, dtype=bf, seed=5))
            continue
        res32, res16 = rnd(M, N, seed=4), rnd(M, N, dtype=bf, seed=5)
        mask = (torch.arange(M) % 7 == 3).to(DEV)
        check("res32", a, w, bias, residual=res32, out_dtype=torch.float32)
        check("res16_relu", a, w, bias, residual=res16, act=ref_ops.ACT_RELU)
        check("gelu_generic", a, w, bias, act=ref_ops.ACT_GELU, out_dtype=torch.float32)
        check("alpha_clamp_mask", a, w, bias, alpha=0.37, clamp=0.8, rowmask=mask, mask_mode=ref_ops.MASK_ZERO_OUTPUT, out_dtype=torch.float32)
        check("trans", a, w, bias, trans_out=True, m_pad=(M + 63) // 64 * 64 + 64)
        check("trans_relu_f32", a, w, None, trans_out=True, act=ref_ops.ACT_RELU, out_dtype=torch.float32)
        if N % 16 == 0:                       # N/2 bf16 outputs per row must keep 16-byte rows (else the launcher falls back)
            check("swiglu", a, w, bias, act=ref_ops.ACT_SWIGLU)
            check("swiglu_f32", a, w, bias, act=ref_ops.ACT_SWIGLU, out_dtype=torch.float32)
        if N % 64 == 0:
            # RoPE, fast path (power-of-two table rows) and generic path (rows cycle every 100)
            cos, sin = rnd(128, 64, seed=7), rnd(128, 64, seed=8)
            check("rope_pow2", a, w, bias, rope=(cos, sin, 128, 64, N // 2 // 64 * 64), out_dtype=torch.float32)
            check("rope_bf16", a, w, bias, rope=(cos, sin, 128, 64, N // 2 // 64 * 64))
            # packed (cos, sin) pairs: the table rows go through LDS in the 256 x 256 tile kernel (pairs share an angle, as in the ViT)
            cp, sp = cos[:, 0::2].repeat_interleave(2, 1).contiguous(), sin[:, 0::2].repeat_interleave(2, 1).contiguous()
            packed = torch.stack([cp[:, 0::2], sp[:, 0::2]], -1).contiguous()
            check("rope_packed", a, w, bias, rope=(cp, sp, 128, 64, N // 2 // 64 * 64, packed), out_dtype=torch.float32)
            check("rope_packed_all_cols", a, w, bias, rope=(cp, sp, 128, 64, N // 64 * 64, packed))
            big_rows = max(M, 128)             # table rows >= M (global blocks): no wrap
            cb, sb = rnd(big_rows, 32, seed=17).repeat_interleave(2, 1).contiguous(), rnd(big_rows, 32, seed=18).repeat_interleave(2, 1).contiguous()
            check("rope_packed_rows_ge_M", a, w, bias, rope=(cb, sb, big_rows, 64, N // 64 * 64, torch.stack([cb[:, 0::2], sb[:, 0::2]], -1).contiguous()))
            check("rope_mod100", a, w, bias, rope=(cos[:100].contiguous(), sin[:100].contiguous(), 100, 64, N // 2 // 64 * 64), out_dtype=torch.float32)
        rs, sh, cv = rnd(M, seed=10).abs() + 0.5, rnd(M, seed=11), rnd(N, seed=12)
        check("rownorm_res32", a, w, bias, rownorm=(rs, sh, cv), residual=res32, out_dtype=torch.float32)
    # strided operands and output views
    big = rnd(1024, 3 * 256, dtype=bf, seed=7)
    w = rnd(512, 256, dtype=bf, scale=1 / 16, seed=8)
    out = torch.zeros(1024, 1024, dtype=bf, device=DEV)
    ops.gemm(big[:, 256:512], w, None, out=out[:, 256:768], tile64=tile)
    assert relerr(out[:, 256:768], ref_ops.gemm(big[:, 256:512], w, None)) < TOL[bf]
    assert out[:, :256].abs().max().item() == 0 and out[:, 768:].abs().max().item() == 0


@pytest.mark.parametrize("bf", H16)
def test_gemm_p8_persistent(ops, monkeypatch, bf):
    """the PERSISTENT flavour of the 256 x 256 tile kernel (one workgroup per CU walking several tiles, the next tile's first K tiles
    and bias staged under the current tile's epilogue, SwiGLU outputs stored behind the counted wait): taken by SwiGLU launches with
    more tiles than CUs -- the ViT's up-projection (vit_eva_clip.py:125-132) -- bit-identical to one workgroup per tile
    (APE_P8_PERSIST=0) and inside the GEMM tolerance of the torch definition; ragged M / N edges (partial row tiles, a half-empty last
    column tile whose waves take the generic epilogue), with and without bias, one and many K tiles"""
    if SELF:
        pytest.skip("kernel selection: HIP library only")
    from ape_amd import _lib
    lib = _lib.load()
    for (M, N, K, use_bias) in [(8192, 5504, 1024, True), (8000, 5504, 256, True), (4096, 4096 + 64, 64, False), (9000, 2176, 128, True), (16384, 5504, 1024, True)]:
        a, w = rnd(M, K, dtype=bf, seed=21), rnd(N, K, dtype=bf, scale=K ** -0.5, seed=22)
        bias = rnd(N, seed=23) if use_bias else None
        tiles = ((M + 255) // 256) * ((N + 255) // 256)
        assert tiles > 256
        monkeypatch.setenv("APE_P8_PERSIST", "0")
        plain = ops.gemm(a, w, bias, tile64=3, act=ref_ops.ACT_SWIGLU)
        assert b"persistent" not in lib.ape_hip_gemm_last_kernel()
        monkeypatch.setenv("APE_P8_PERSIST", "1")
        got = ops.gemm(a, w, bias, tile64=3, act=ref_ops.ACT_SWIGLU)
        assert b"persistent" in lib.ape_hip_gemm_last_kernel(), (M, N, K)
        assert torch.equal(got, plain), (M, N, K)
        if M <= 9000:
            e = relerr(got, ref_ops.gemm(a, w, bias, act=ref_ops.ACT_SWIGLU))
            print(f"gemm p8 persistent M{M} N{N} K{K}: {e:.3e}")
            assert e < TOL[bf]
        # outside the flavour's contract the launcher keeps one workgroup per tile
        ops.gemm(a, w, bias, tile64=3, act=ref_ops.ACT_SWIGLU, out_dtype=torch.float32)
        assert b"persistent" not in lib.ape_hip_gemm_last_kernel()
    monkeypatch.delenv("APE_P8_PERSIST")
    ops.gemm(a, w, bias, tile64=3, act=ref_ops.ACT_SWIGLU)
    assert b"persistent" in lib.ape_hip_gemm_last_kernel()            # the default


@pytest.mark.parametrize("bf", H16)
def test_gemm_p8_residual_prefetch(ops, monkeypatch, bf):
    """the 256 x 128 tile kernel requests a tile's fp32 RESIDUAL ahead of its main loop (inline-asm loads into registers the epilogue
    reads; the N = 1024 projections of the ViT, vit_eva_clip.py:264-268,125-132): bit-identical to the epilogue loading it
    (APE_P8_RESPF=0), for fp32 and 16-bit outputs, with the folded LayerNorm of the down projection, ragged M / N edges, repeated
    launches (a register read before its load has landed would differ from run to run)"""
    if SELF:
        pytest.skip("kernel-internal data path: HIP library only")
    # (1024, 256, 64), (2048, 1024, 64): ONE K tile on full tiles -- the main loop then has no counted wait that could retire the prefetch
    # (the launcher must not prefetch there)
    for (M, N, K) in [(8192, 1024, 1024), (8192, 1024, 2752 // 64 * 64), (4096 + 100, 1024, 512), (8192, 896 + 64, 256), (300, 384, 64), (1024, 256, 64), (2048, 1024, 64)]:
        a, w = rnd(M, K, dtype=bf, seed=41), rnd(N, K, dtype=bf, scale=K ** -0.5, seed=42)
        bias, res = rnd(N, seed=43), rnd(M, N, seed=44)
        rs, sh, cv = rnd(M, seed=45).abs() + 0.5, rnd(M, seed=46), rnd(N, seed=47)
        for kw in (dict(out_dtype=torch.float32), dict(out_dtype=bf), dict(out_dtype=torch.float32, rownorm=(rs, sh, cv)), dict(out_dtype=torch.float32, act=ref_ops.ACT_RELU)):
            monkeypatch.setenv("APE_P8_RESPF", "0")
            plain = ops.gemm(a, w, bias, residual=res, tile64=4, **kw)
            monkeypatch.setenv("APE_P8_RESPF", "1")
            for rep in range(3):
                got = ops.gemm(a, w, bias, residual=res, tile64=4, **kw)
                assert torch.equal(got, plain), (M, N, K, list(kw), rep)
        e = relerr(ops.gemm(a, w, bias, residual=res, tile64=4, out_dtype=torch.float32), ref_ops.gemm(a, w, bias, residual=res, out_dtype=torch.float32))
        print(f"gemm p8<128> residual prefetch M{M} N{N} K{K}: identical; vs the definition {e:.3e}")
        assert e < 3e-4


def test_gemm_half_outputs_saturate(ops):
    """every IEEE-half store of the GEMM kernels SATURATES at +-65504 instead of producing inf: the deformable attention's value projection
    relies on it (layers/multi_scale_deform_attn.py: no clamp= on the half value / offset projections since round 5; the reference's fp16
    evaluation overflows to inf there, multi_scale_deform_attn.py:262-264).  Pinned per kernel path: the K = 256 register-resident kernel
    (bf16 operands -> half output, and half operands), its LayerNorm-free residual flavour, and the 256 x 128 / 256 x 256 tile kernels"""
    if SELF:
        pytest.skip("kernel store path: HIP library only")
    big = 300.0
    for dt_in, (M, N, K), tile in [(torch.bfloat16, (4096, 256, 256), None), (torch.float16, (4096, 256, 256), None), (torch.float16, (4096, 512, 256), None),
                                   (torch.float16, (2048, 1024, 512), 4), (torch.float16, (2048, 1024, 512), 3)]:
        a = torch.full((M, K), big, device=DEV).to(dt_in)
        sign = torch.where(torch.arange(N, device=DEV) % 2 == 0, 1.0, -1.0)
        w = (sign[:, None] * torch.ones((N, K), device=DEV)).to(dt_in)          # every output = +-300 * K = +-76 800 (K = 256) > 65504
        got = ops.gemm(a, w, None, out_dtype=torch.float16, **({"tile64": tile} if tile is not None else {}))
        assert got.dtype == torch.float16 and bool(torch.isfinite(got).all()), (dt_in, M, N, K, tile)
        assert torch.equal(got.float(), (sign * 65504.0).expand(M, N)), (dt_in, M, N, K, tile)
    print("half outputs saturate at +-65504 on the kres and p8 paths")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
def test_geometry_kernel(ops, dt):
    """csrc/geometry.hip (per-image-size constants written into the graph's fixed buffers) == the tensor-level definition
    geometry.build_geometry + level embedding, for full, padded and extreme image sizes"""
    if SELF:
        pytest.skip("device kernel vs its tensor-level definition")
    from ape_amd.modeling.ape_deta import geometry as G
    S = 512
    shapes = [(S // st, S // st) for st in (4, 8, 16, 32, 64)]
    cfg = dict(num_pos_feats=128, temperature=10000, normalize=True, offset=-0.5, eps=1e-6, scale=2 * 3.141592653589793)
    lev = rnd(5, 256, seed=1)
    for (h, w) in [(512, 512), (384, 512), (512, 299), (480, 17), (33, 512), (1, 1), (511, 257)]:
        g = G.build_geometry(S, (h, w), shapes, torch.device(DEV), cfg)
        lp = (g.pos + lev[g.level_ids]).to(dt).contiguous()
        sg = G.StaticGeometry(G.build_geometry(S, (S, S), shapes, torch.device(DEV), cfg), "k", torch.zeros_like(lp))
        sg.generate(S, (h, w), cfg, lev)
        assert torch.equal(sg.mask, g.mask) and torch.equal(sg.mask_u8, g.mask_u8) and torch.equal(sg.invalid_u8, g.invalid_u8), (h, w)
        assert torch.equal(sg.valid_ratios, g.valid_ratios) and torch.equal(sg.vr4, g.vr4) and torch.equal(sg.box_scale, g.box_scale)
        fin = torch.isfinite(g.proposals)
        assert torch.equal(torch.isfinite(sg.proposals), fin), (h, w)           # same usable / unusable pattern
        e_prop = (sg.proposals[fin] - g.proposals[fin]).abs().max().item() if fin.any() else 0.0
        e_ref = (sg.enc_ref - g.enc_ref).abs().max().item()
        assert e_prop <= 2e-6 and e_ref <= 1e-6, (h, w, e_prop, e_ref)          # logf / division: last-bit differences
        got = next(iter(sg._lvl_pos.values())).float()
        usable = ~g.mask                                  # fully padded rows / columns: sin / cos of ~ -3e6 (chaotic), never attended
        e_all = (got - lp.float()).abs().max().item()
        e_use = (got[usable] - lp.float()[usable]).abs().max().item()
        print(f"geometry kernel {dt} {h}x{w}: lvl_pos max abs diff usable {e_use:.2e} all {e_all:.2e}")
        assert e_use <= (1e-6 if dt == torch.float32 else 8e-3), (h, w, e_use)


# ------------------------------------------------------------------------------------------------
# data-dependent selections (csrc/topk.hip) vs their sort / cumsum definitions: index outputs must be IDENTICAL
# ------------------------------------------------------------------------------------------------
def _qlogits(n, seed, lo=-8.0, hi=6.0, step=1 / 64):
    """logits on a grid coarse enough that distinct logits have distinct float32 sigmoids (no ulp-level ambiguity between two
    correct sigmoid implementations), with plenty of exact ties"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randint(int(lo / step), int(hi / step), (n,), generator=g).float() * step).to(DEV)


def test_enc_finalize(ops):
    T = 5000
    g = torch.Generator(device="cpu").manual_seed(0)
    cls2 = torch.randint(-20, 20, (T, 2), generator=g).float().div(4).to(DEV)            # ties between the two heads
    d = rnd(T, 8, seed=1)
    anchors = rnd(T, 4, seed=2, scale=2.0)
    anchors[::7] = float("inf")
    ec, eb, xy = ops.enc_finalize(cls2.contiguous(), d.contiguous(), anchors.contiguous())
    rc, rb, rxy = ref_ops.enc_finalize(cls2, d, anchors)
    assert torch.equal(ec, rc) and torch.equal(eb, rb)
    assert (xy - rxy).abs().max().item() < 1e-6


@pytest.mark.parametrize("shapes,k,nq,mode", [
    ([(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)], 1000, 900, "random"),
    ([(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)], 1000, 900, "ties"),
    ([(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)], 1000, 900, "fallback"),
    ([(64, 64), (32, 32), (16, 16), (8, 8), (4, 4)], 1000, 900, "random"),
    ([(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)], 1000, 300, "ties"),
    ([(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)], 1000, 100, "random"),
    ([(40, 27), (20, 14), (10, 7)], 300, 90, "random"),
    ([(320, 308), (160, 154), (80, 77), (40, 39), (20, 20)], 1000, 900, "random"),      # 32 elements per thread in the level and fallback segments
    ([(8, 8), (4, 4), (2, 2), (1, 1)], 1000, 900, "random"),                            # more queries than tokens
    ([(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)], 1000, 901, "random"),      # a quota that does not divide
])
def test_select_proposals(ops, shapes, k, nq, mode):
    T = sum(h * w for h, w in shapes)
    logit = _qlogits(T, 3, step=1 / 64 if mode != "ties" else 1.0)
    g = torch.Generator(device="cpu").manual_seed(4)
    c = torch.rand(T, 2, generator=g)
    wh = torch.rand(T, 2, generator=g) * (0.3 if mode != "fallback" else 0.0) + (0.02 if mode != "fallback" else 0.9)
    if mode == "fallback":
        c = c * 0.01 + 0.5                                   # near-identical boxes: NMS keeps a handful, the naive top-k takes over
    xyxy = torch.cat([c - wh / 2, c + wh / 2], 1).clamp(0, 1).to(DEV).contiguous()
    got = ops.select_proposals(logit, xyxy, shapes, k, nq, 0.9)
    ref = ref_ops.select_proposals(logit, xyxy, shapes, k, nq, 0.9)
    assert got.dtype == torch.int64 and got.shape == (nq,)
    assert torch.equal(got.cpu(), ref.cpu()), f"{(got.cpu() != ref.cpu()).sum().item()} of {nq} proposals differ"


# (900, 1203, 500): LVIS vocabulary with top-500 -> the 64-elements-per-thread stage-1 instantiation; (900, 1203, 900): (lists x k)
# beyond stage 2's LDS -> the intermediate merge level (no configuration raises from inside model.forward)
_DET_SHAPES = [(900, 80, 100), (900, 400, 300), (900, 1, 1), (300, 7, 500), (1024, 3, 100), (900, 1203, 500), (900, 1203, 900)]


# score_thresh 0.05: a strict comparison inside class_sort; padded: the logits are a view of a [Q, K + 3] buffer whose slack is NaN
@pytest.mark.parametrize("Q,K,topk,score_thresh,padded",
                         [pytest.param(Q, K, t, 0.0, False, id=f"{Q}-{K}-{t}") for Q, K, t in _DET_SHAPES]
                         + [pytest.param(Q, K, t, 0.05, False, id=f"{Q}-{K}-{t}-thresh0.05") for Q, K, t in _DET_SHAPES]
                         + [pytest.param(900, 80, 100, 0.0, True, id="900-80-100-padded"),
                            pytest.param(900, 80, 100, 0.05, True, id="900-80-100-thresh0.05-padded")])
def test_detections(ops, Q, K, topk, score_thresh, padded):
    g = torch.Generator(device="cpu").manual_seed(5)
    logits = (torch.randint(-600, 200, (Q, K), generator=g).float() / 64).to(DEV)
    if padded:
        buf = torch.full((Q, K + 3), float("nan"), device=DEV)
        buf[:, :K] = logits
        logits = buf[:, :K]
    if K > 2:
        logits[:, 1] = float("-inf")                         # a class switched off (evaluation-dataset mode)
    if Q > 10:
        logits[5, 0] = float("nan")                          # a non-finite row is dropped entirely (fast_rcnn.py:132-137)
    c = torch.rand(Q, 2, generator=g)
    wh = torch.rand(Q, 2, generator=g) * 0.4 + 0.02
    boxes = torch.cat([c, wh], 1).to(DEV).contiguous()
    if Q > 10:
        boxes[7, 2] = float("inf")
    scale = torch.tensor([1024.0, 683.0, 1024.0, 683.0], device=DEV)
    got = ops.detections(logits, boxes, scale, score_thresh, 0.7, topk)
    ref = ref_ops.detections(logits, boxes, scale, score_thresh, 0.7, topk)
    k = min(topk, Q * K)
    assert got["det_scores"].shape == (k,)
    assert torch.equal(got["det_query"].cpu(), ref["det_query"].cpu())
    assert torch.equal(got["det_classes"].cpu(), ref["det_classes"].cpu())
    assert (got["det_scores"] - ref["det_scores"]).abs().max().item() < 1e-6
    assert (got["det_boxes"] - ref["det_boxes"]).abs().max().item() < 1e-3


@pytest.mark.parametrize("bf", H16)
@pytest.mark.parametrize("M,HID", [(128, 64), (300, 128), (4096, 2048), (87296, 2048)])
def test_ffn_fused(ops, M, HID, bf):
    """y = x + relu(x W1^T + b1) W2^T + b2 in one kernel vs the two-GEMM definition at the same rounding points; both W2
    layouts (row-major: two ds_read_b64 per fragment; pre-permuted hidden columns: one ds_read_b128)"""
    from ape_amd.packing import permute_ffn_w2

    x = rnd(M, 256, dtype=bf, seed=1)
    res = rnd(M, 256, dtype=bf, seed=6)
    w1, b1 = rnd(HID, 256, dtype=bf, scale=1 / 16, seed=2), rnd(HID, seed=3)
    w2, b2 = rnd(256, HID, dtype=bf, scale=HID ** -0.5, seed=4), rnd(256, seed=5)
    ref = ref_ops.ffn_fused(x, w1, b1, w2, b2, residual=res)
    got = ops.ffn_fused(x, w1, b1, w2, b2, residual=res)
    e = relerr(got, ref)
    w2p = permute_ffn_w2(w2)
    assert relerr(ref_ops.ffn_fused(x, w1, b1, w2p, b2, residual=res, w2_permuted=True), ref) == 0.0
    gotp = ops.ffn_fused(x, w1, b1, w2p, b2, residual=res, w2_permuted=True)
    ep = relerr(gotp, ref)
    print(f"ffn_fused M{M} HID{HID}: {e:.3e} (row-major W2), {ep:.3e} (pre-permuted W2)")
    assert e < TOL[bf] and ep < TOL[bf]
    assert torch.equal(got, gotp)                      # the same MFMAs on the same operands
    assert relerr(ops.ffn_fused(x, w1, b1, w2, b2), ref_ops.ffn_fused(x, w1, b1, w2, b2)) < TOL[bf]
    # LayerNorm of the finished row in the epilogue (the transformer layer's post-FFN norm), incl. the rows past M of the last tile
    lw, lb = 1.0 + 0.1 * rnd(256, seed=7), 0.1 * rnd(256, seed=8)
    gotn = ops.ffn_fused(x, w1, b1, w2p, b2, residual=res, w2_permuted=True, norm=(lw, lb, 1e-5))
    refn = ref_ops.ffn_fused(x, w1, b1, w2, b2, residual=res, norm=(lw, lb, 1e-5))
    en = relerr(gotn, refn)
    print(f"ffn_fused + LayerNorm epilogue M{M} HID{HID}: {en:.3e}")
    assert en < TOL[bf] and torch.isfinite(gotn.float()).all()
    # both workgroup heights (128 / 192 rows; the launcher picks by M) give the same rows
    for rt in ("2", "3"):
        os.environ["APE_FFN_RT"] = rt
        try:
            assert torch.equal(ops.ffn_fused(x, w1, b1, w2p, b2, residual=res, w2_permuted=True, norm=(lw, lb, 1e-5)), gotn), rt
        finally:
            os.environ.pop("APE_FFN_RT")


@pytest.mark.parametrize("k,h,w,H,W,nthing,offset", [(40, 96, 128, 150, 200, 5, -1), (100, 64, 64, 64, 64, 3, 3), (7, 50, 70, 33, 91, 0, 0)])
def test_panoptic_merge(ops, k, h, w, H, W, nthing, offset):
    """csrc/masks.hip panoptic_* (pixel ownership + areas, the sequential walk, the map) vs the reference's loop
    (deformable_detr_segm_vl.py:921-998) restated in tests/ref_ops.py"""
    g = torch.Generator().manual_seed(k)
    K = 12
    # smooth blobs: low-resolution noise upsampled, so owners form regions and several queries overlap
    low = torch.randn(k, 6, 8, generator=g) * 4.0
    masks_full = torch.nn.functional.interpolate(low[None], size=(h + 5, w + 3), mode="bilinear", align_corners=False)[0].to(DEV).contiguous()
    masks = masks_full[:, :h, :w]                                       # a cropped view: row / query strides differ from the shape
    scores = torch.rand(k, generator=g).to(DEV)
    keep = (torch.rand(k, generator=g) > 0.3).to(DEV)
    classes = torch.randint(0, K, (k,), generator=g).to(DEV)
    isthing = (torch.arange(K) < nthing).to(DEV)
    kw = dict(prob=0.5, overlap_threshold=0.4, stuff_offset=offset)
    seg, info, count = ops.panoptic_merge(masks, scores, keep, classes, isthing, H, W, **kw)
    wseg, winfo, wcount = ref_ops.panoptic_merge(masks, scores, keep, classes, isthing, H, W, **kw)
    n, wn = int(count.item()), int(wcount.item())
    agree = (seg == wseg).float().mean().item()
    print(f"panoptic_merge k{k} {h}x{w} -> {H}x{W}: {n} segments (definition {wn}), pixel agreement {agree:.5f}")
    assert seg.dtype == torch.int32 and tuple(seg.shape) == (H, W)
    assert n == wn and torch.equal(info[:n].cpu(), winfo[:wn].cpu())
    assert agree > 0.999                                                # sigmoid / bilinear rounding at a threshold pixel
    none = torch.zeros_like(keep)
    seg, info, count = ops.panoptic_merge(masks, scores, none, classes, isthing, H, W, **kw)
    assert int(count.item()) == 0 and int(seg.abs().sum().item()) == 0


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("use_perm,use_bias,N", [(False, False, 256), (True, True, 256), (True, False, 384)])
def test_conv3x3_implicit_gemm(ops, dtype, use_perm, use_bias, N):
    """the 3 x 3 convolutions of the pyramid / mask head at 256 x 256 pixels as an implicit GEMM (the tile kernel stages its A operand
    from the shifted input rows, ApeGemmArgs.conv_*): bit-identical to im2col3x3 + gemm -- same tiles, same K order -- incl. the
    zero rows outside the image, rows addressed through a permutation, and a map with a padded row stride"""
    H = W = 256
    C = 256
    x_full = rnd(H * W + 7, C + 8, dtype=dtype, seed=1)
    x = x_full[:, :C]                                                        # row stride 264: a view, like the model's maps
    w = (rnd(N, 9 * C, seed=2) * (9 * C) ** -0.5).to(dtype)
    bias = rnd(N, seed=3) if use_bias else None
    perm = torch.randperm(H * W, generator=torch.Generator().manual_seed(4)).int().to(DEV) if use_perm else None
    if not SELF:
        assert ops.conv3x3_implicit_ok(x, w, H, W)
    got = ops.conv3x3(x, perm, H, W, w, bias)
    want = ops.gemm(ops.im2col3x3(x, perm, H, W), w, bias)
    assert tuple(got.shape) == (H * W, N) and got.dtype == dtype
    assert torch.equal(got, want), (got.float() - want.float()).abs().max().item()
    ref = ref_ops.conv3x3(x, perm, H, W, w, bias)
    e = relerr(got, ref)
    print(f"conv3x3 implicit {dtype} perm={use_perm} N={N}: identical to im2col + gemm; vs the definition {e:.2e}")
    assert e < T16(dtype, 1e-2, 1e-5)
    if not SELF:
        def timed(fn, reps=10):
            fn()
            s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                fn()
            t.record()
            t.synchronize()
            return s.elapsed_time(t) * 1e3 / reps
        print(f"   implicit {timed(lambda: ops.conv3x3(x, perm, H, W, w, bias)):.1f} us vs im2col + gemm "
              f"{timed(lambda: ops.gemm(ops.im2col3x3(x, perm, H, W), w, bias)):.1f} us")
        small = ops.conv3x3(x[:64 * 64 + 7], None, 64, 64, w, bias)          # too few tiles: the im2col path behind the same entry
        assert torch.equal(small, ops.gemm(ops.im2col3x3(x[:64 * 64 + 7], None, 64, 64), w, bias))


@pytest.mark.parametrize("dtype", H16)
def test_conv3x3_implicit_gemm_p3_map(ops, dtype):
    """the 128 x 128-pixel p3 convolution (vit_eva_clip.py:806-842): 64 row tiles are too few for 256 x 256 tiles, so the implicit
    flavour runs on 256 x 128 tiles (128 workgroups) -- bit-identical to im2col3x3 + the same tile kernel on the materialised operand"""
    H = W = 128
    C = N = 256
    x = rnd(H * W, C, dtype=dtype, seed=5)
    w = (rnd(N, 9 * C, seed=6) * (9 * C) ** -0.5).to(dtype)
    bias = rnd(N, seed=7)
    perm = torch.randperm(H * W, generator=torch.Generator().manual_seed(8)).int().to(DEV)
    got = ops.conv3x3(x, perm, H, W, w, bias)
    if not SELF:
        from ape_amd import _lib
        assert ops.conv3x3_implicit_ok(x, w, H, W)
        assert b"p8_kernel<128, true, conv3x3>" in _lib.load().ape_hip_gemm_last_kernel()
        want = ops.gemm(ops.im2col3x3(x, perm, H, W), w, bias, tile64=4)
        assert torch.equal(got, want), (got.float() - want.float()).abs().max().item()
    e = relerr(got, ref_ops.conv3x3(x, perm, H, W, w, bias))
    print(f"conv3x3 implicit p3 {dtype}: vs the definition {e:.2e}")
    assert e < T16(dtype, 1e-2, 1e-5)

