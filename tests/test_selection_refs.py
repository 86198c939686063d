"""CPU checks of tests/selection_refs.py: the stage definitions, chained through ref_ops' NMS, equal ref_ops.select_proposals /
ref_ops.detections exactly on every end-to-end case of tests/test_ops_gpu.py; the fp32 sigmoid is strictly increasing on every
grid a case draws from; and every case of tests/test_selection_gpu.py has the property it is there for (which stage-1 variant,
how many merge levels, how many survivors), checked by arithmetic from the constants of csrc/topk.hip.  No GPU needed."""
import numpy as np
import pytest
import torch

import ref_ops
import selection_refs as R


def test_rank_rule():
    v = np.array([-0.0, 0.0, -0.0, 0.0], np.float32)
    assert R.rank_desc(v).tolist() == [0, 1, 2, 3]                               # the two zeros are equal
    v = np.array([1.0, np.nan, np.inf, 1.0, -np.inf, np.nan, -0.0, 0.0], np.float32)
    assert R.rank_desc(v).tolist() == [1, 5, 2, 0, 3, 6, 7, 4]                   # NaN above +inf, ties by index
    rng = np.random.default_rng(0)
    for pattern in R.TOPK_PATTERNS + ("nan",):
        x = R.logit_pattern(pattern, 700, 300, seed=int(rng.integers(1 << 30)))
        assert np.array_equal(R.rank_desc(x), R.rank_desc_tuples(x)), pattern
        if pattern != "signed-zeros":                                            # torch.sort orders +-0 as equal too; checked apart below
            assert np.array_equal(R.rank_desc(x), torch.sort(torch.from_numpy(x), descending=True, stable=True)[1].numpy()), pattern
    z = torch.tensor([-0.0, 0.0, -0.0, 0.0])
    assert torch.sort(z, descending=True, stable=True)[1].tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("lo,hi,step", [(-8.0, 6.0, 1 / 64), (-8.0, 6.0, 1.0), (-600 / 64, 200 / 64, 1 / 64)], ids=["grid", "ties", "detections"])
def test_fp32_sigmoid_is_injective_on_the_grids(lo, hi, step):
    """ranking by the float64 sigmoid is ranking by ANY correct fp32 sigmoid only if the latter is strictly increasing"""
    x = torch.arange(int(round(lo / step)), int(round(hi / step))).float() * step
    a, b = torch.sigmoid(x), 1.0 / (1.0 + torch.exp(-x))
    assert bool((a[1:] > a[:-1]).all()) and bool((b[1:] > b[:-1]).all())
    assert (a - b).abs().max().item() <= 1.2e-7
    ref = torch.from_numpy(R.sigmoid64(x.numpy()))
    assert (a.double() - ref).abs().max().item() <= 1.2e-7 and (b.double() - ref).abs().max().item() <= 1.2e-7


def _on_grid(x):
    f = x[np.isfinite(x)].astype(np.float64)
    return bool(np.all(f * 64 == np.round(f * 64)) and np.all(f >= R.GRID_LO) and np.all(f < R.GRID_HI))


def test_every_pattern_stays_on_the_grid():
    for pattern in R.TOPK_PATTERNS + ("nan",):
        for T, k in ((1, 1), (301, 300), (8193, 1000), (16385, 1000)):
            x = R.logit_pattern(pattern, T, k, seed=11)
            assert x.dtype == np.float32 and x.shape == (T,) and _on_grid(x), (pattern, T)
            assert not np.any(np.isnan(x) & np.signbit(x)), "a negative NaN: its rank is not pinned"
    x = R.logit_pattern("signed-zeros", 4096, 1000, seed=11)
    assert np.any(np.signbit(x) & (x == 0)) and np.any(~np.signbit(x) & (x == 0))
    x = R.logit_pattern("kth-tie", 16385, 1000, seed=11)
    run = np.flatnonzero(x == 4.0)
    assert (x > 4.0).sum() == 997 and run.min() < 8192 <= run.max() and len(run) == 10      # the k-th place lies in a run across the chunk edge
    x = R.logit_pattern("ascending", 16385, 1000, seed=11)
    assert np.all(np.diff(x) >= 0) and R.rank_desc(x)[:1000].min() >= 16385 - 8192          # the whole top-k in the last chunk


# ------------------------------------------------------------------------------------------------ the chains
def _chain_select(logit, xyxy, shapes, k, nq, thr):
    ns = [h * w for h, w in shapes]
    starts, T, L = R.level_starts(ns), sum(ns), len(ns)
    kk, k_alt = min(k, T), min(nq, T)
    cand, alt = R.proposal_topk(logit.numpy(), starts, ns, kk, k_alt)
    boxes_b, groups_b, seg, cand_a, lv_a, pos_b = R.proposal_order(cand, logit.numpy(), xyxy.numpy(), starts, ns)
    n = L * kk
    max_seg = min(n, kk + sum(max(0, kk - m) for m in ns))
    keep_b = ref_ops.nms_segments(torch.from_numpy(boxes_b), torch.from_numpy(groups_b).to(torch.int32),
                                  torch.from_numpy(seg).to(torch.int32), max_seg, thr)
    return R.proposal_quota(cand_a, lv_a, pos_b, keep_b.numpy(), alt, k_alt, starts, ns, nq), int(keep_b.sum())


@pytest.mark.parametrize("shapes,k,nq,mode", R.E2E_PROPOSALS)
def test_stage_chain_equals_select_proposals(shapes, k, nq, mode):
    logit, xyxy = R.e2e_proposal_inputs(shapes, mode)
    got, kept = _chain_select(logit, xyxy, shapes, k, nq, 0.9)
    ref = ref_ops.select_proposals(logit, xyxy, shapes, k, nq, 0.9)
    assert np.array_equal(got, ref.numpy())
    assert (kept < nq) == (mode == "fallback" or nq > sum(h * w for h, w in shapes))      # the fallback list is used exactly where meant


@pytest.mark.parametrize("Q,K,topk,thresh,padded", R.E2E_DETECTIONS)
def test_stage_chain_equals_detections(Q, K, topk, thresh, padded):
    logits, boxes, scale = R.e2e_detection_inputs(Q, K)
    if padded:
        buf = torch.full((Q, K + 3), float("nan"))
        buf[:, :K] = logits
        logits = buf[:, :K]
    xyxy, finite, sorted_, order, valid = R.det_sort(logits.numpy(), boxes.numpy(), scale.numpy(), thresh)
    xyxy32 = torch.from_numpy(xyxy).float()
    keep = ref_ops.nms_classes(xyxy32, torch.from_numpy(order).to(torch.int32), 0.7, torch.from_numpy(valid).to(torch.uint8))
    k = min(topk, Q * K)
    det_boxes, det_scores, det_classes, det_query = R.det_topk(sorted_, keep.numpy(), order, xyxy32.numpy(), Q, k)
    ref = ref_ops.detections(logits, boxes, scale, thresh, 0.7, topk)
    assert np.array_equal(det_query, ref["det_query"].numpy()) and np.array_equal(det_classes, ref["det_classes"].numpy())
    assert np.abs(det_scores - ref["det_scores"].double().numpy()).max() < 1e-6
    assert np.abs(det_boxes - ref["det_boxes"].numpy()).max() < 1e-3
    if thresh > 0:
        assert 0 < int(valid.sum()) < int((R.det_sort(logits.numpy(), boxes.numpy(), scale.numpy(), 0.0)[4]).sum())


def test_e2e_additions_take_the_paths_they_are_for():
    big = [h * w for h, w in R.E2E_PROPOSALS[7][0]]
    assert R.topk_per(big[:1], [1000]) == 32 and R.topk_per([sum(big)], [900]) == 32 and R.proposal_per(big, 1000, 900) == 32
    assert all(R.proposal_per([h * w for h, w in s], min(k, sum(h * w for h, w in s)), min(nq, sum(h * w for h, w in s))) == 8
               for s, k, nq, _ in R.E2E_PROPOSALS[:7])                                                     # what the suite ran so far
    small = [h * w for h, w in R.E2E_PROPOSALS[8][0]]
    assert R.E2E_PROPOSALS[8][2] > sum(small)                                                             # nq > T
    assert R.E2E_PROPOSALS[9][2] % 5 != 0


# ------------------------------------------------------------------------------------------------ preconditions of the GPU cases
def test_proposal_topk_case_preconditions():
    C = R.THREADS
    for ns, k, k_alt, per, why in R.TOPK_SWITCH:
        n = ns[0]
        assert R.proposal_per(ns, k, k_alt) == per
        small = {32: 8, 64: 32}[per]
        if why == "size":
            assert -(-n // (small * C)) * k > R.STAGE2_MAX and -(-n // (per * C)) * k <= R.STAGE2_MAX
        else:                                                # every segment fits stage 2 at 8 per thread: only the job count forces 32
            assert -(-n // (8 * C)) * max(k, k_alt) <= R.STAGE2_MAX and 2 * -(-n // (8 * C)) > R.MAX_JOBS
            assert 2 * -(-n // (32 * C)) <= R.MAX_JOBS
    ns, k, k_alt = R.TOPK_TOO_LARGE
    assert R.proposal_per(ns, k, k_alt) == 0 and -(-ns[0] // (64 * C)) * k > R.STAGE2_MAX
    for _, ns, k, k_alt, _ in R.topk_cases():
        assert 1 <= k <= 1024 and 1 <= k_alt <= min(1024, sum(ns)) and k <= sum(ns) and R.proposal_per(ns, k, k_alt) > 0
    assert all(R.proposal_per((n,), k, min(n, 1024)) == 8 for n, k in R.TOPK_SINGLE)
    # 8193 = one full chunk + a chunk of 1 element: its stage-1 list has fewer than k entries and is zero-padded into stage 2
    assert 8193 - 8 * C == 1 and 16385 - 2 * 8 * C == 1
    assert R.TOPK_SHORT[1][0] < 1000 and R.TOPK_SHORT[1][0] + R.TOPK_SHORT[1][1] >= 1000       # a short first level: every filler lies above it
    logit, cand, alt = R.topk_case(R.TOPK_SHORT[1], 1000, 900, "grid")
    assert cand[5:1000].tolist() == list(range(5, 1000)) and sorted(cand[:5].tolist()) == [0, 1, 2, 3, 4]
    logit, cand, alt = R.topk_case(R.TOPK_SHORT[0], 1000, 900, "grid")
    assert cand[1000 + 300:2000].tolist() == list(range(0, 700))                               # level 1 (tokens 1500..1799): fillers from below
    assert cand[4000 + 1:5000].tolist() == list(range(0, 999))
    logit = R.logit_pattern("signed-zeros", 8193, 1000, seed=11)
    assert (logit > 0).sum() < 900                           # the zeros reach into the fallback list: their order decides it
    _, alt = R.proposal_topk(logit, [0], [8193], 1000, 900)
    z = alt[logit[alt] == 0]
    assert np.any(np.signbit(logit[z])) and np.all(np.diff(z) > 0)


def test_proposal_order_and_quota_case_preconditions():
    cases = R.order_cases()
    assert {c[0] for c in cases} == set(R.ORDER_N) and max(R.ORDER_N) == R.ORDER_MAX
    assert {(c[0], c[2]) for c in cases} >= {(n, p) for n in R.ORDER_N for p in R.ORDER_PATTERNS}
    assert {(c[1], c[3]) for c in cases if c[0] == 8192} == {(L, s) for L in (1, 3, 5) for s in R.ORDER_SPREADS}
    *_, ref = R.order_case(8192, 5, "grid", "empty-levels")
    seg = ref[2]
    assert seg[1] == seg[2] and seg[4] == seg[5] == 8192 and seg[1] > 0
    *_, ref = R.order_case(8192, 5, "grid", "one-level")
    assert ref[2].tolist() == [0, 0, 0, len(ref[3]), len(ref[3]), len(ref[3])]
    for n, L, nq, n_alt in R.QUOTA_SHAPES:
        for keep in R.QUOTA_KEEPS:
            cand_a, lv_a, pos_b, keep_b, alt, starts, ns, out = R.quota_case(n, L, nq, n_alt, keep)
            kept = int(keep_b.sum())
            assert sorted(pos_b.tolist()) == list(range(n)) and len(alt) == n_alt and len(out) == nq
            want = {"all": n, "none": 0, "exactly-nq": min(n, nq), "nq-1": min(n, nq - 1), "one-per-level": L}.get(keep)
            assert want is None or kept == want, (n, L, nq, keep, kept)
            if keep == "one-level":
                assert kept == int((lv_a == L - 1).sum()) > 0
            if keep == "one-level-empty":
                assert kept == int((lv_a != 0).sum()) and (L == 1) == (kept == 0)
    shapes = set(R.QUOTA_SHAPES)
    assert any(nq % L for n, L, nq, _ in shapes) and any(nq > n for n, L, nq, _ in shapes) and any(nq > 1024 for n, L, nq, _ in shapes)
    assert any(n_alt < nq for n, L, nq, n_alt in shapes) and any(n_alt > n for n, L, nq, n_alt in shapes)
    assert int(R.quota_case(5000, 5, 900, 900, "exactly-nq")[3].sum()) == 900 and int(R.quota_case(5000, 5, 900, 900, "nq-1")[3].sum()) == 899


def test_det_sort_case_preconditions():
    g = R.grid_points().astype(np.float64)
    s = R.sigmoid64(g)
    for th in R.SORT_THRESH:
        t = float(np.float32(th))
        away = np.abs(s - t)
        assert np.all((away >= 1e-4) | ((g == 0) & (th == 0.5))), th          # only the exact 0.5 of a zero logit may sit on a threshold
    assert R.sigmoid64(np.float32(0.0)) == 0.5
    for Q, K in R.SORT_SHAPES:
        padded, boxes, scale, ref = R.sort_case(Q, K, 0.5)
        lg = padded[:, :K]
        assert np.isnan(padded[:, K:]).all() and _on_grid(lg)
        xyxy, finite, sorted_, order, valid = ref
        if Q > 10:
            assert (lg == 0).mean() > 0.15 and not finite[5] and not finite[7] and finite[3] and int(finite.sum()) == Q - 2
            assert not valid[sorted_ == 0.5].any() and (sorted_ == 0.5).sum() > 0.15 * Q * K and valid.any()
            assert xyxy[3, 0] > xyxy[3, 2]
        assert all(sorted(order[c].tolist()) == list(range(Q)) for c in range(K))


def test_det_topk_case_preconditions():
    plans = {(K * Q, k): R.det_plan(K * Q, k) for K, Q, ks in R.TOPK_DET for k in ks}
    assert plans[(360000, 300)] == (32, False, 0)
    assert plans[(852992, 1024)] == (64, True, 1) and plans[(9438208, 1024)] == (64, True, 2)
    assert plans[(9438208, 100)] == (64, True, 1)
    # k = 100 misses stage 2 by size as well (145 lists x 100); with k = 64 the lists fit (9280 <= 12288) and only the job limit sets
    # the merge flag: no merge level runs
    assert -(-9438208 // 65536) == 145 > R.MAX_JOBS and 145 * 64 <= R.STAGE2_MAX < 145 * 100 and plans[(9438208, 64)] == (64, True, 0)
    assert plans[(65537, 1024)] == (8, False, 0) and plans[(8193, 100)] == (8, False, 0)
    for K, Q, ks in R.TOPK_DET:
        assert all(1 <= k <= min(1024, K * Q) for k in ks) and K * Q < 2 ** 31
    for K, Q, k, keep in R.det_topk_cases():
        if K * Q >= R.DET_LARGE:
            continue
        s, kp, order, xyxy, ref = R.det_topk_case(K, Q, k, keep)
        kept = int(kp.sum())
        assert all(sorted(order[c].tolist()) == list(range(Q)) for c in range(0, K, max(1, K // 7)))
        if keep == "k-1":
            assert kept == k - 1 and ref[1][-1] == -1.0 and (k == 1 or ref[1][-2] > 0)
        if keep == "none":
            assert kept == 0 and np.all(ref[1] == -1.0) and ref[2].tolist() == [i // Q for i in range(k)]
        if keep == "random30" and K * Q > 1000:
            assert kept > k
        if keep == "edge-ties" and K * Q > 20000:
            assert kept > k and (ref[1] == 0.75).sum() == k // 3 and (ref[1] == 0.5).sum() == k - k // 3
