"""-m gpu: the selection kernels of csrc/topk.hip stage by stage against the plain definitions of tests/selection_refs.py, at
their chunk, tie and quota edges: all three stage-1 variants (8 / 32 / 64 elements per thread), the job limit, zero / one / two
merge levels, n == k and n == k + 1, 8191 / 8192 / 8193, constant / ascending / signed-zero / NaN / inf keys, short levels,
empty levels, every branch of the quota, score thresholds and padded logits.

Each stage is fed directly (proposal_quota and det_topk get synthetic keep flags: nothing here depends on the NMS kernels)
through the C-ABI, with ctypes wrappers local to this file.  Every index output must be IDENTICAL to the reference; floats that
are copies must be bit-equal; computed floats keep the bounds of test_detections (1e-6 on scores, 1e-3 on boxes scaled by
~1000).  Every output lies between two guard zones filled, like the output itself, with a sentinel: nothing outside the
documented extent may be written, everything inside it must be.  tests/test_selection_refs.py checks on the CPU that every case
has the property it is listed for."""
import ctypes
import os

import numpy as np
import pytest
import torch

import selection_refs as R

pytestmark = pytest.mark.gpu

# APE_TEST_SELFCHECK=1 runs this file on CPU with the kernels := their definitions (validates the test harness itself)
SELF = os.environ.get("APE_TEST_SELFCHECK") == "1"
DEV = "cpu" if SELF else "cuda"
GUARD = 64                                                   # elements on either side of an output; keeps 16-byte alignment
_SENT = {torch.int32: R.SENTINEL, torch.int64: R.SENTINEL, torch.float32: float(R.SENTINEL), torch.uint8: 0xAB}


@pytest.fixture(scope="module")
def lib():
    if SELF:
        return None
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from ape_amd import _lib

    return _lib.load()


def _p(t):
    from ape_amd.ops import _p as p

    return p(t)


def _stream():
    from ape_amd.ops import _stream as s

    return s()


class Out:
    """an output of `shape` between two guard zones, all of it pre-filled with the sentinel of its type"""

    def __init__(self, shape, dtype):
        self.shape, self.n, self.sentinel = tuple(shape), int(np.prod(shape)), _SENT[dtype]
        self.buf = torch.full((2 * GUARD + self.n,), self.sentinel, dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + self.n].view(self.shape)

    def fill(self, value):                                   # SELF mode
        self.view.copy_(torch.as_tensor(np.asarray(value)).to(self.view.dtype).reshape(self.shape))

    def read(self, label, untouched=False):
        b = self.buf.cpu()
        assert bool((b[:GUARD] == self.sentinel).all()) and bool((b[GUARD + self.n:] == self.sentinel).all()), f"{label}: written out of bounds"
        if untouched:
            assert bool((b == self.sentinel).all()), f"{label}: written although the call failed"
        return b[GUARD:GUARD + self.n].view(self.shape).numpy()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _levels_c(starts, ns):
    L = len(ns)
    return (ctypes.c_int * L)(*[int(s) for s in starts]), (ctypes.c_int * L)(*[int(n) for n in ns]), L


def _done(rc, lib, what):
    assert rc == 0, f"{what} failed (rc={rc}): {lib.ape_hip_last_error().decode()}"
    torch.cuda.synchronize()


def _ints(got, ref, label):
    got, ref = np.asarray(got).astype(np.int64), np.asarray(ref).astype(np.int64)
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    bad = np.flatnonzero(got.reshape(-1) != ref.reshape(-1))
    assert bad.size == 0, f"{label}: {bad.size} of {ref.size} differ, first at {bad[:5].tolist()}: got {got.reshape(-1)[bad[:5]].tolist()} " \
                          f"for {ref.reshape(-1)[bad[:5]].tolist()}"


def _bits(got, ref, label):
    got, ref = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(ref, dtype=np.float32)
    assert got.shape == ref.shape
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"{label}: a copied float differs"


# ------------------------------------------------------------------------------------------------ proposal_topk
def _run_proposal_topk(lib, logit, ns, k, k_alt):
    starts, T = R.level_starts(ns), int(sum(ns))
    cand, alt = Out((len(ns) * k,), torch.int32), Out((k_alt,), torch.int32)
    if SELF:
        if R.proposal_per(ns, k, k_alt) == 0:
            return -1, b"do not fit", cand, alt
        c, a = R.proposal_topk(logit, starts, ns, k, k_alt)
        cand.fill(c), alt.fill(a)
        return 0, b"", cand, alt
    sc, nc, L = _levels_c(starts, ns)
    x = _dev(logit)
    ws = torch.empty((lib.ape_hip_topk_workspace_words(T),), dtype=torch.int64, device=DEV)
    rc = lib.ape_hip_proposal_topk(_p(x), T, sc, nc, L, k, k_alt, _p(ws), _p(cand.view), _p(alt.view), _stream())
    torch.cuda.synchronize()
    return rc, lib.ape_hip_last_error() or b"", cand, alt


_TOPK = R.topk_cases()


@pytest.mark.parametrize("ns,k,k_alt,pattern", [c[1:] for c in _TOPK], ids=[c[0] for c in _TOPK])
def test_proposal_topk(lib, ns, k, k_alt, pattern):
    logit, ref_cand, ref_alt = R.topk_case(tuple(ns), k, k_alt, pattern)
    rc, msg, cand, alt = _run_proposal_topk(lib, logit, ns, k, k_alt)
    assert rc == 0, msg
    label = f"proposal_topk ns={ns} k={k} k_alt={k_alt} {pattern}"
    _ints(cand.read(label), ref_cand, label + " cand")
    _ints(alt.read(label), ref_alt, label + " alt")


def test_proposal_topk_too_large(lib):
    """a token count no chunk size fits is refused by the argument check: non-zero, a message, nothing launched or written"""
    ns, k, k_alt = R.TOPK_TOO_LARGE
    rc, msg, cand, alt = _run_proposal_topk(lib, np.zeros(ns[0], np.float32), ns, k, k_alt)
    assert rc != 0 and b"do not fit" in msg, (rc, msg)
    cand.read("cand", untouched=True), alt.read("alt", untouched=True)


# ------------------------------------------------------------------------------------------------ proposal_order
_ORDER_NAMES = ("boxes_b", "groups_b", "seg", "cand_a", "lv_a", "pos_b")


def _run_proposal_order(lib, cand, logit, xyxy, starts, ns):
    n, L = len(cand), len(ns)
    outs = [Out((n, 4), torch.float32), Out((n,), torch.int32), Out((L + 1,), torch.int32), Out((n,), torch.int32), Out((n,), torch.int32),
            Out((n,), torch.int32)]
    if SELF:
        for o, r in zip(outs, R.proposal_order(cand, logit, xyxy, starts, ns)):
            o.fill(r)
        return outs
    sc, nc, _ = _levels_c(starts, ns)
    c, x, b = _dev(cand, torch.int32), _dev(logit), _dev(xyxy)
    rc = lib.ape_hip_proposal_order(_p(c), n, _p(x), _p(b), sc, nc, L, *[_p(o.view) for o in outs], _stream())
    _done(rc, lib, "ape_hip_proposal_order")
    return outs


@pytest.mark.parametrize("n,L,pattern,spread", R.order_cases(), ids=lambda v: str(v))
def test_proposal_order(lib, n, L, pattern, spread):
    cand, logit, xyxy, starts, ns, ref = R.order_case(n, L, pattern, spread)
    outs = _run_proposal_order(lib, cand, logit, xyxy, starts, ns)
    label = f"proposal_order n={n} L={L} {pattern} {spread}"
    got = [o.read(f"{label} {name}") for o, name in zip(outs, _ORDER_NAMES)]
    for g, r, name in zip(got[1:], ref[1:], _ORDER_NAMES[1:]):
        _ints(g, r, f"{label} {name}")
    _bits(got[0], ref[0], f"{label} boxes_b")


# ------------------------------------------------------------------------------------------------ proposal_quota
def _run_proposal_quota(lib, cand_a, lv_a, pos_b, keep_b, alt, n_alt, starts, ns, nq):
    out = Out((nq,), torch.int64)
    if SELF:
        out.fill(R.proposal_quota(cand_a, lv_a, pos_b, keep_b, alt, n_alt, starts, ns, nq))
        return out
    sc, nc, L = _levels_c(starts, ns)
    ca, la, pb, kb, al = _dev(cand_a, torch.int32), _dev(lv_a, torch.int32), _dev(pos_b, torch.int32), _dev(keep_b), _dev(alt, torch.int32)
    rc = lib.ape_hip_proposal_quota(_p(ca), _p(la), _p(pb), _p(kb), len(cand_a), _p(al), n_alt, sc, nc, L, nq, _p(out.view), _stream())
    _done(rc, lib, "ape_hip_proposal_quota")
    return out


@pytest.mark.parametrize("keep", R.QUOTA_KEEPS)
@pytest.mark.parametrize("n,L,nq,n_alt", R.QUOTA_SHAPES)
def test_proposal_quota(lib, n, L, nq, n_alt, keep):
    cand_a, lv_a, pos_b, keep_b, alt, starts, ns, ref = R.quota_case(n, L, nq, n_alt, keep)
    out = _run_proposal_quota(lib, cand_a, lv_a, pos_b, keep_b, alt, n_alt, starts, ns, nq)
    label = f"proposal_quota n={n} L={L} nq={nq} n_alt={n_alt} keep={keep} ({int(keep_b.sum())} kept)"
    _ints(out.read(label), ref, label)


# ------------------------------------------------------------------------------------------------ det_sort
def _run_det_sort(lib, logits, boxes, scale, thresh):
    """logits: a [Q, K] torch view on DEV with unit inner stride (its row stride is passed on)"""
    Q, K = logits.shape
    outs = [Out((Q, 4), torch.float32), Out((Q,), torch.uint8), Out((K, Q), torch.float32), Out((K, Q), torch.int32), Out((K, Q), torch.uint8)]
    if SELF:
        for o, r in zip(outs, R.det_sort(logits.numpy(), boxes, scale, thresh)):
            o.fill(r)
        return outs
    from ape_amd.ops import _ld

    b, s = _dev(boxes), _dev(scale)
    rc = lib.ape_hip_det_sort(_p(logits), _ld(logits), Q, K, _p(b), _p(s), float(thresh), *[_p(o.view) for o in outs], _stream())
    _done(rc, lib, "ape_hip_det_sort")
    return outs


@pytest.mark.parametrize("thresh", R.SORT_THRESH)
@pytest.mark.parametrize("layout", ["padded", "contiguous"])
@pytest.mark.parametrize("Q,K", R.SORT_SHAPES)
def test_det_sort(lib, Q, K, layout, thresh):
    padded, boxes, scale, (r_xyxy, r_finite, r_sorted, r_order, r_valid) = R.sort_case(Q, K, thresh)
    logits = _dev(padded)[:, :K]
    if layout == "contiguous":
        logits = logits.contiguous()
    else:
        assert logits.stride(0) == K + R.SORT_PAD
    outs = _run_det_sort(lib, logits, boxes, scale, thresh)
    label = f"det_sort Q={Q} K={K} {layout} thresh={thresh}"
    xyxy, finite, sorted_, order, valid = [o.read(f"{label} {name}") for o, name in zip(outs, ("xyxy", "finite", "sorted", "order", "valid"))]
    _ints(finite, r_finite, label + " finite")
    _ints(order, r_order, label + " order")
    _ints(valid, r_valid, label + " valid")
    nan = np.isnan(r_sorted)
    assert np.array_equal(np.isnan(sorted_), nan), label + " sorted: NaN places"
    e_s = float(np.abs(np.where(nan, 0.0, sorted_.astype(np.float64) - r_sorted)).max())
    e_b = float(np.abs(xyxy.astype(np.float64) - r_xyxy).max())
    print(f"{label}: sorted err {e_s:.2e}, xyxy err {e_b:.2e}, {int(r_valid.sum())} of {r_valid.size} valid")
    assert e_s < 1e-6 and e_b < 1e-3, (label, e_s, e_b)


# ------------------------------------------------------------------------------------------------ det_topk
def _run_det_topk(lib, sorted_, keep, order, xyxy, K, Q, k):
    outs = [Out((k, 4), torch.float32), Out((k,), torch.float32), Out((k,), torch.int64), Out((k,), torch.int64)]
    if SELF:
        for o, r in zip(outs, R.det_topk(sorted_, keep, order, xyxy, Q, k)):
            o.fill(r)
        return outs
    s, kp, od, bx = _dev(sorted_), _dev(keep), _dev(order), _dev(xyxy)
    ws = torch.full((lib.ape_hip_topk_workspace_words(K * Q),), -1, dtype=torch.int64, device=DEV)
    rc = lib.ape_hip_det_topk(_p(s), _p(kp), _p(od), _p(bx), K, Q, k, _p(ws), *[_p(o.view) for o in outs], _stream())
    _done(rc, lib, "ape_hip_det_topk")
    levels = R.det_plan(K * Q, k)[2]
    if levels:
        # a merge level must write its lists into the SPARE third of the workspace (include/ape_hip.h: "+ half as many again for the
        # lists of an intermediate merge level"), never over the lists other workgroups of the same launch are still reading: in
        # place the result is right only as long as every reader happens to run before its list's writer.  No key here is NaN, so
        # no composite is all ones.
        lists = ws.numel() // 1024
        spare = lists - lists // 3
        first = ws[spare * 1024: spare * 1024 + k].cpu()
        assert bool((first != -1).all()), "det_topk: the merge level did not write into the spare part of the workspace"
    return outs


@pytest.mark.parametrize("K,Q,k,keep", R.det_topk_cases(), ids=lambda v: str(v))
def test_det_topk(lib, K, Q, k, keep):
    sorted_, kp, order, xyxy, (r_boxes, r_scores, r_classes, r_query) = R.det_topk_case(K, Q, k, keep)
    outs = _run_det_topk(lib, sorted_, kp, order, xyxy, K, Q, k)
    label = f"det_topk K={K} Q={Q} k={k} {keep} ({int(kp.sum())} kept, plan {R.det_plan(K * Q, k)})"
    boxes, scores, classes, query = [o.read(f"{label} {name}") for o, name in zip(outs, ("boxes", "scores", "classes", "query"))]
    _ints(query, r_query, label + " det_query")              # with fewer than k survivors the tail (score -1) is pinned as well
    _ints(classes, r_classes, label + " det_classes")
    _bits(scores, r_scores, label + " det_scores")           # copies of `sorted`, or exactly -1
    _bits(boxes, xyxy[r_query], label + " det_boxes")
