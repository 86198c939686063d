"""Plain definitions of the selection stages of csrc/topk.hip, one per C-ABI entry, and the seeded cases their tests share.

Every definition is written from the stage's contract (include/ape_hip.h, DESIGN.md "Tie rule") with explicit loops and one
ranking function over float64 values; none of them uses tests/ref_ops.py, whose select_proposals / detections state the same
pipeline end to end with cumsum / scatter (tests/test_selection_refs.py chains the stages and demands the same result).

The ranking rule, everywhere: descending value; equal values go to the LOWEST index; -0.0 == +0.0; a positive NaN ranks above
+inf (as in torch.sort).  Where a NEGATIVE NaN ranks is NOT pinned: no case here contains one.

Scores are ranked by the float64 sigmoid of the fp32 logit.  That equals the order of any correct fp32 sigmoid only where the
fp32 sigmoid is strictly increasing, which holds on the grid every case draws its logits from ([-8, 6), step 1/64:
tests/test_selection_refs.py asserts it for torch.sigmoid and for 1 / (1 + exp(-x))).  Above about 16 the two saturate
differently; such logits are out of scope and appear in no rank-deciding position (+inf, whose sigmoid is exactly 1, does).
"""
import functools
import itertools

import numpy as np

F64 = np.float64

# the constants of csrc/topk.hip the cases are sized by: 1024 threads; 8 / 32 / 64 elements per thread in stage 1;
# stage 2 holds 12 288 composites in LDS; at most 96 stage-1 jobs per proposal selection; proposal_order / quota take 8192
THREADS, PERS, STAGE2_MAX, MAX_JOBS, ORDER_MAX = 1024, (8, 32, 64), 12288, 96, 8192
GRID_LO, GRID_HI, GRID_STEP = -8.0, 6.0, 1 / 64           # tests/test_ops_gpu.py::_qlogits
SENTINEL = -7777


def grid_points(step=GRID_STEP):
    return (np.arange(int(GRID_LO / step), int(GRID_HI / step)) * step).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the definitions
def rank_desc(values):
    """indices of `values` in descending order: ties (and -0.0 / +0.0) by lowest index, NaN first"""
    v = np.asarray(values, dtype=F64).reshape(-1)
    nan = np.isnan(v)
    if nan.any():                                            # lexsort: last key first; it is stable, so the index decides last
        return np.lexsort((np.where(nan, 0.0, -v), ~nan))
    return np.argsort(-v, kind="stable")                     # -(-0.0) == -(+0.0)


def rank_desc_tuples(values):
    """the same as a sort of (is-not-NaN, -value, index) tuples -- the form rank_desc is checked against"""
    v = [float(x) for x in np.asarray(values, dtype=F64).reshape(-1)]
    return np.array(sorted(range(len(v)), key=lambda i: (0, 0.0, i) if v[i] != v[i] else (1, -v[i], i)), dtype=np.int64)


def sigmoid64(x):
    x = np.asarray(x, dtype=np.float32).astype(F64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def level_starts(ns):
    return [int(sum(ns[:i])) for i in range(len(ns))]


def level_of(starts, idx):
    idx = np.asarray(idx, dtype=np.int64)
    lv = np.zeros(idx.shape, dtype=np.int64)
    for s in starts[1:]:
        lv += idx >= s
    return lv


def proposal_topk(logit, starts, ns, k, k_alt):
    """-> cand [L*k]: per level its best k tokens by sigmoid score, a short level filled up with the lowest token indices
    outside it (their masked score is zero); alt [k_alt]: the best tokens of all by raw logit"""
    logit = np.asarray(logit, dtype=np.float32)
    T = logit.size
    cand = []
    for s, n in zip(starts, ns):
        own = [s + int(i) for i in rank_desc(sigmoid64(logit[s:s + n]))[:k]]
        outside = (t for t in range(T) if not s <= t < s + n)
        cand += own + list(itertools.islice(outside, k - len(own)))
    alt = rank_desc(logit.astype(F64))[:k_alt]
    return np.array(cand, dtype=np.int64), alt.astype(np.int64)


def proposal_order(cand, logit, xyxy, starts, ns):
    """A order = candidates by descending raw logit (ties: position in cand); B order = level-major, A order inside a level.
    -> boxes_b [n,4], groups_b [n], seg [L+1] (B order); cand_a [n], lv_a [n], pos_b [n] (A order; pos_b = place in B)"""
    cand = np.asarray(cand, dtype=np.int64)
    logit, xyxy = np.asarray(logit, dtype=np.float32), np.asarray(xyxy, dtype=np.float32)
    n, L = cand.size, len(ns)
    cand_a = cand[rank_desc(logit[cand].astype(F64))]
    lv_a = level_of(starts, cand_a)
    pos_b, groups_b, boxes_b = np.empty(n, np.int64), np.empty(n, np.int64), np.empty((n, 4), np.float32)
    seg, b = [0], 0
    for l in range(L):
        for a in np.flatnonzero(lv_a == l):
            pos_b[a], groups_b[b], boxes_b[b] = b, l, xyxy[cand_a[a]]
            b += 1
        seg.append(b)
    return boxes_b, groups_b, np.array(seg, dtype=np.int64), cand_a, lv_a, pos_b


def proposal_quota(cand_a, lv_a, pos_b, keep_b, alt, n_alt, starts, ns, nq):
    """the NMS survivors in A order -- or, with fewer than nq of them, the first min(n, n_alt) entries of alt: per level the
    first nq // L, then the best of the rest up to nq, all in their order; -> out [nq], zero where nothing is left"""
    n, L = len(cand_a), len(ns)
    items = [(int(cand_a[a]), int(lv_a[a])) for a in range(n) if keep_b[pos_b[a]] != 0]
    if len(items) < nq:
        toks = [int(alt[a]) for a in range(min(n, n_alt))]
        items = list(zip(toks, [int(l) for l in level_of(starts, toks)]))
    quota, taken, chosen = nq // L, [0] * L, [False] * len(items)
    for i, (_, l) in enumerate(items):
        if taken[l] < quota:
            chosen[i] = True
            taken[l] += 1
    need = nq - sum(chosen)
    for i in range(len(items)):
        if need > 0 and not chosen[i]:
            chosen[i] = True
            need -= 1
    picked = [t for (t, _), c in zip(items, chosen) if c][:nq]
    return np.array(picked + [0] * (nq - len(picked)), dtype=np.int64)


def det_sort(logits, boxes, scale, thresh):
    """logits [Q,K], boxes [Q,4] cxcywh, scale [4] -> xyxy [Q,4] float64 (corners * scale, clipped; zero on a non-finite row),
    finite [Q], sorted [K,Q] float64 sigmoid scores by rank, order [K,Q] query of each rank, valid [K,Q] (score > thresh, the
    float32 threshold the kernel receives, and a finite row)"""
    lg = np.asarray(logits, dtype=np.float32)
    Q, K = lg.shape
    s = sigmoid64(lg)
    b, sc = np.asarray(boxes, dtype=np.float32).astype(F64), np.asarray(scale, dtype=np.float32).astype(F64)
    with np.errstate(invalid="ignore"):
        xyxy = np.stack([b[:, 0] - 0.5 * b[:, 2], b[:, 1] - 0.5 * b[:, 3], b[:, 0] + 0.5 * b[:, 2], b[:, 1] + 0.5 * b[:, 3]], 1) * sc
    finite = np.isfinite(xyxy).all(1) & np.isfinite(s).all(1)
    xyxy = np.where(finite[:, None], np.minimum(np.maximum(xyxy, 0.0), sc), 0.0)
    order = np.stack([rank_desc(s[:, c]) for c in range(K)])
    sorted_ = np.stack([s[order[c], c] for c in range(K)])
    with np.errstate(invalid="ignore"):
        valid = (sorted_ > float(np.float32(thresh))) & finite[order]
    return xyxy, finite, sorted_, order, valid


def det_topk(sorted_, keep, order, xyxy, Q, k):
    """the best k (class, rank) pairs among the kept ones, a suppressed pair scoring -1 -> det_boxes, det_scores, det_classes,
    det_query"""
    masked = np.where(np.asarray(keep).reshape(-1) != 0, np.asarray(sorted_).reshape(-1).astype(F64), -1.0)
    flat = rank_desc(masked)[:k]
    query = np.asarray(order).reshape(-1)[flat].astype(np.int64)
    return np.asarray(xyxy)[query], masked[flat], flat // Q, query


# ------------------------------------------------------------------------------------------------ what the host code decides
def topk_per(seg_n, seg_k):
    """elements per thread of stage 1 (0: none fits), from the documented rule: the smallest of 8 / 32 / 64 with which every
    segment's ceil(n / (per * 1024)) * k fits stage 2 and all segments together need at most 96 jobs"""
    for per in PERS:
        chunks = [-(-n // (per * THREADS)) for n in seg_n]
        if all(c * k <= STAGE2_MAX for c, k in zip(chunks, seg_k)) and sum(chunks) <= MAX_JOBS:
            return per
    return 0


def proposal_per(ns, k, k_alt):
    return topk_per(list(ns) + [int(sum(ns))], [k] * len(ns) + [k_alt])


def det_plan(total, k):
    """-> (per, merge flag, merge levels) of det_topk"""
    per = topk_per([total], [k])
    if per:
        return per, False, 0
    lists, levels = -(-total // (64 * THREADS)), 0
    while lists * k > STAGE2_MAX:
        lists, levels = -(-lists // (STAGE2_MAX // k)), levels + 1
    return 64, True, levels


# ------------------------------------------------------------------------------------------------ cases: logit patterns
def _grid(rng, n, lo=GRID_LO, hi=GRID_HI, step=GRID_STEP):
    return (rng.integers(int(lo / step), int(hi / step), n).astype(np.float32) * np.float32(step)).astype(np.float32)


def _chunk_edge(T):
    return 8192 if T > 8200 else T // 2


def logit_pattern(pattern, T, k, seed):
    """[T] float32 logits; every finite value lies on the 1/64 grid of [-8, 6)"""
    rng = np.random.default_rng(seed)
    if pattern == "grid":
        return _grid(rng, T)
    if pattern == "ties":
        return _grid(rng, T, step=1.0)
    if pattern == "const":
        return np.full(T, 1.25, np.float32)
    if pattern in ("ascending", "descending"):               # weakly monotonic over all 896 grid points: the best sit in the last / first chunk
        x = grid_points()[(np.arange(T, dtype=np.int64) * 896) // T]
        return x.copy() if pattern == "ascending" else x[::-1].copy()
    if pattern == "kth-tie":                                 # k - 3 large values, then 4.0 on a run across the k-th place and a chunk edge
        x = _grid(rng, T, hi=3.0)
        e = _chunk_edge(T)
        run = np.arange(max(0, e - 2), min(T, e + 8))
        rest = np.setdiff1d(np.arange(T), run)
        big = rng.permutation(rest)[:max(0, k - 3)]
        x[big] = _grid(rng, big.size, lo=4.5)
        x[run] = 4.0
        return x
    if pattern == "specials":
        x = _grid(rng, T)
        pos = rng.permutation(T)[:9]
        for i, p in enumerate(pos):
            x[p] = (np.inf, -np.inf, np.nan)[i % 3]
        return x
    if pattern == "nan":
        x = _grid(rng, T)
        x[rng.permutation(T)[:max(1, T // 50)]] = np.nan
        return x
    if pattern == "signed-zeros":                            # +-0.0 interleaved, a few other values around them
        x = np.where(rng.integers(0, 2, T) == 1, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        other = rng.permutation(T)[:T // 8]
        x[other] = _grid(rng, other.size)
        return x
    raise KeyError(pattern)


TOPK_PATTERNS = ("grid", "ties", "const", "ascending", "descending", "kth-tie", "specials", "signed-zeros")
TOPK_SINGLE = ((1, 1), (300, 300), (301, 300), (1024, 1024), (1025, 1024), (8191, 1000), (8192, 1000), (8193, 1000), (16385, 1000))
TOPK_SHORT = ((1500, 300, 70, 20, 1), (5, 3000))             # k = 1000; the second: a short FIRST level, fillers from above it
# (ns, k, k_alt, elements per thread expected, why)
TOPK_SWITCH = (((98305,), 1000, 1000, 32, "size"), ((393217,), 1024, 1024, 64, "size"), ((401409,), 100, 100, 32, "jobs"))
TOPK_TOO_LARGE = ((786433,), 1024, 1024)
_K_ALT = (1, 900, 1024)


def topk_cases():
    """[(id, ns, k, k_alt, pattern)]"""
    out = []
    for i, (n, k) in enumerate(TOPK_SINGLE):
        for j, pat in enumerate(TOPK_PATTERNS):
            out.append((f"{n}-{k}-{pat}", (n,), k, min(n, _K_ALT[(i + j) % 3]), pat))
    for i, ns in enumerate(TOPK_SHORT):
        for j, pat in enumerate(TOPK_PATTERNS):
            out.append(("+".join(map(str, ns)) + f"-{pat}", ns, 1000, min(sum(ns), _K_ALT[(i + j + 1) % 3]), pat))
    for ns, k, k_alt, _, _ in TOPK_SWITCH:
        for pat in ("grid", "ties"):
            out.append((f"{ns[0]}-{k}-{pat}", ns, k, k_alt, pat))
    return out


@functools.lru_cache(maxsize=4)
def topk_case(ns, k, k_alt, pattern):
    logit = logit_pattern(pattern, int(sum(ns)), k, seed=11)
    cand, alt = proposal_topk(logit, level_starts(ns), ns, k, k_alt)
    return logit, cand, alt


# ------------------------------------------------------------------------------------------------ cases: proposal_order
ORDER_N = (1, 2, 1023, 1024, 1025, 2048, 5000, 5120, 8191, 8192)
ORDER_PATTERNS = ("grid", "ties", "const", "signed-zeros", "nan")
ORDER_LEVELS = {1: (3000,), 3: (2000, 700, 300), 5: (1500, 800, 400, 200, 100)}
ORDER_SPREADS = ("uniform", "one-level", "empty-levels")


def order_cases():
    """[(n, L, pattern, spread)]: every n with every pattern, L and spread rotating; n = 1 and n = 8192 with every L x spread"""
    out = []
    for i, n in enumerate(ORDER_N):
        for j, pat in enumerate(ORDER_PATTERNS):
            out.append((n, (1, 3, 5)[(i + j) % 3], pat, ORDER_SPREADS[(i + 2 * j) % 3]))
    for n in (1, 8192):
        for L in (1, 3, 5):
            for spread in ORDER_SPREADS:
                if (n, L, "grid", spread) not in out:
                    out.append((n, L, "grid", spread))
    return out


@functools.lru_cache(maxsize=4)
def order_case(n, L, pattern, spread):
    """-> cand [n] (arbitrary tokens, duplicates included), logit [T], xyxy [T,4], starts, ns, reference outputs"""
    ns = ORDER_LEVELS[L]
    starts, T = level_starts(ns), sum(ns)
    rng = np.random.default_rng(1000 * n + 10 * L + ORDER_SPREADS.index(spread))
    allowed = np.ones(T, bool)
    if spread == "one-level":
        allowed[:] = level_of(starts, np.arange(T)) == L // 2
    elif spread == "empty-levels" and L > 1:                 # L = 3: level 1 stays empty; L = 5: levels 1 and 4 (seg[l] == seg[l+1])
        lv = level_of(starts, np.arange(T))
        allowed[:] = (lv != 1) & ((lv != 4) | (L < 5))
    cand = rng.choice(np.flatnonzero(allowed), size=n, replace=True).astype(np.int64)
    logit = logit_pattern(pattern, T, 0, seed=n + L)
    xyxy = rng.random((T, 4), dtype=np.float32)
    return cand, logit, xyxy, starts, ns, proposal_order(cand, logit, xyxy, starts, ns)


# ------------------------------------------------------------------------------------------------ cases: proposal_quota
QUOTA_SHAPES = ((5000, 5, 900, 900), (5000, 5, 901, 901), (900, 3, 100, 100), (340, 4, 900, 85), (5000, 5, 1500, 1500), (300, 1, 300, 300),
                (200, 2, 300, 300), (8192, 5, 900, 900))    # (n, L, nq, n_alt)
QUOTA_KEEPS = ("all", "none", "exactly-nq", "nq-1", "one-level", "one-level-empty", "one-per-level")
QUOTA_LEVELS = {1: (3000,), 2: (2200, 800), 3: (2000, 700, 300), 4: (1700, 800, 350, 150), 5: (1500, 800, 400, 200, 100)}


@functools.lru_cache(maxsize=4)
def quota_case(n, L, nq, n_alt, keep):
    """-> cand_a, lv_a, pos_b (a random permutation, as in production), keep_b, alt [n_alt], starts, ns, reference out [nq]"""
    ns = QUOTA_LEVELS[L]
    starts, T = level_starts(ns), sum(ns)
    rng = np.random.default_rng(100 * n + nq + QUOTA_KEEPS.index(keep))
    cand_a = rng.integers(0, T, n).astype(np.int64)
    lv_a = level_of(starts, cand_a)
    pos_b = rng.permutation(n).astype(np.int64)
    alt = rng.integers(0, T, n_alt).astype(np.int64)
    kept = np.zeros(n, bool)
    if keep == "all":
        kept[:] = True
    elif keep in ("exactly-nq", "nq-1"):
        kept[rng.permutation(n)[:min(n, nq - (keep == "nq-1"))]] = True
    elif keep == "one-level":
        kept[:] = lv_a == L - 1
    elif keep == "one-level-empty":
        kept[:] = lv_a != 0
    elif keep == "one-per-level":
        for l in range(L):
            kept[np.flatnonzero(lv_a == l)[:1]] = True
    keep_b = np.zeros(n, np.uint8)
    keep_b[pos_b[kept]] = 1
    return cand_a, lv_a, pos_b, keep_b, alt, starts, ns, proposal_quota(cand_a, lv_a, pos_b, keep_b, alt, n_alt, starts, ns, nq)


# ------------------------------------------------------------------------------------------------ cases: det_sort
SORT_SHAPES = ((1, 1), (63, 65), (64, 64), (65, 63), (900, 130), (1024, 3))           # (Q, K)
SORT_THRESH = (0.0, 0.05, 0.5)
SORT_SCALE = (1024.0, 683.0, 1024.0, 683.0)
SORT_PAD = 3


@functools.lru_cache(maxsize=4)
def sort_case(Q, K, thresh):
    """-> logits [Q, K + 3] (the slack columns NaN; [:, :K] is the padded view, a contiguous copy of it the other layout),
    boxes, scale, reference outputs.  About a third of the logits are exactly 0: their score is exactly 0.5 in any arithmetic,
    which thresh = 0.5 must reject (the comparison is strict)."""
    rng = np.random.default_rng(7 * Q + K)
    lg = _grid(rng, Q * K).reshape(Q, K)
    lg[rng.random((Q, K)) < 0.3] = 0.0
    if K > 2:
        lg[:, 1] = -np.inf                                   # a class switched off
    if Q > 1:
        lg[Q // 2, 0] = np.inf
    if Q > 10:
        lg[5, K // 2] = np.nan                               # a non-finite row is dropped entirely
    boxes = np.concatenate([rng.random((Q, 2), dtype=np.float32), rng.random((Q, 2), dtype=np.float32) * 0.4 + 0.02], 1).astype(np.float32)
    if Q > 10:
        boxes[7, 2] = np.inf
    if Q > 3:
        boxes[3, 2] = -0.2                                   # negative width: finite, x1 > x2
    padded = np.full((Q, K + SORT_PAD), np.nan, np.float32)
    padded[:, :K] = lg
    scale = np.array(SORT_SCALE, np.float32)
    return padded, boxes, scale, det_sort(lg, boxes, scale, thresh)


# ------------------------------------------------------------------------------------------------ cases: det_topk
# (K, Q, ks): total = K * Q pairs; the k of one total share one input and one reference ranking (its prefixes)
TOPK_DET = ((1, 1, (1,)), (4, 25, (100,)), (1, 101, (100,)), (1, 8191, (100,)), (8, 1024, (100,)), (3, 2731, (100,)), (65537, 1, (1024,)),
            (400, 900, (300,)), (833, 1024, (1024,)), (9217, 1024, (1024, 100, 64)))
DET_KEEPS = ("random30", "k-1", "none", "edge-ties")
DET_LARGE = 9217 * 1024                                      # only "random30": 9.4 M pairs, one reference sort


def det_topk_cases():
    """[(K, Q, k, keep)]"""
    return [(K, Q, k, keep) for K, Q, ks in TOPK_DET for keep in (DET_KEEPS if K * Q < DET_LARGE else DET_KEEPS[:1]) for k in ks]


@functools.lru_cache(maxsize=1)
def det_topk_input(K, Q, kmax, keep):
    """-> sorted [K,Q] float32 (per class descending, on the grid j / 4096: with 30 % kept the best k of a large total are ties
    of the top one or two values, spread over every chunk and merge group, so the index decides across all their edges), keep
    [K,Q] uint8, order [K,Q] int32 (a permutation per class), xyxy [Q,4], and the reference for kmax"""
    total = K * Q
    rng = np.random.default_rng(total + DET_KEEPS.index(keep))
    s = -np.sort(-(rng.integers(1, 4096, (K, Q)).astype(np.float32) / np.float32(4096)), axis=1)
    kp = np.zeros(total, np.uint8)
    if keep == "random30":
        kp[rng.random(total) < 0.3] = 1
    elif keep == "k-1":
        ends = np.array([0, total - 1] if total > 1 else [0], dtype=np.int64)          # the first and the last pair among them
        kp[np.concatenate([ends, 1 + rng.permutation(max(0, total - 2))])[:kmax - 1]] = 1
    elif keep == "edge-ties":                                # one value everywhere, 0.75 on the LAST kmax // 3 kept pairs: the best come from the
        s[:] = 0.5                                           # last chunk, the rest of the k are the lowest kept indices, many next to an edge
        edges = [m * c + d for c in (8192, 32768, 65536, 12 * 65536) for m in range(1, total // c + 1) for d in (-1, 0)]
        pos = np.union1d(np.array([e for e in edges if 0 <= e < total] + [0, total - 1], dtype=np.int64), rng.permutation(total)[:2 * kmax])
        kp[pos] = 1
        s.reshape(-1)[pos[len(pos) - kmax // 3:]] = 0.75
    a = next(a for a in range(max(2, Q // 3), Q + 2) if np.gcd(a, Q) == 1)
    order = ((np.arange(Q, dtype=np.int64)[None, :] * a + np.arange(K, dtype=np.int64)[:, None]) % Q).astype(np.int32)
    xyxy = rng.random((Q, 4), dtype=np.float32) * 1000
    kp = kp.reshape(K, Q)
    return s, kp, order, xyxy, det_topk(s, kp, order, xyxy, Q, kmax)


def det_topk_case(K, Q, k, keep):
    kmax = max(next(ks for K2, Q2, ks in TOPK_DET if (K2, Q2) == (K, Q)))
    s, kp, order, xyxy, ref = det_topk_input(K, Q, kmax, keep)
    return s, kp, order, xyxy, tuple(r[:k] for r in ref)


# ------------------------------------------------------------------------------------------------ cases: end to end
# the inputs of tests/test_ops_gpu.py::test_select_proposals / test_detections, restated with numpy-free torch so that the seeds
# agree: (shapes, k, nq, mode) and (Q, K, topk, score_thresh, padded)
E2E_PROPOSALS = (
    ([(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)], 1000, 900, "random"),
    ([(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)], 1000, 900, "ties"),
    ([(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)], 1000, 900, "fallback"),
    ([(64, 64), (32, 32), (16, 16), (8, 8), (4, 4)], 1000, 900, "random"),
    ([(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)], 1000, 300, "ties"),
    ([(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)], 1000, 100, "random"),
    ([(40, 27), (20, 14), (10, 7)], 300, 90, "random"),
    ([(320, 308), (160, 154), (80, 77), (40, 39), (20, 20)], 1000, 900, "random"),
    ([(8, 8), (4, 4), (2, 2), (1, 1)], 1000, 900, "random"),
    ([(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)], 1000, 901, "random"),
)
E2E_DETECTIONS = tuple((Q, K, topk, th, False) for Q, K, topk in ((900, 80, 100), (900, 400, 300), (900, 1, 1), (300, 7, 500), (1024, 3, 100),
                                                                  (900, 1203, 500), (900, 1203, 900)) for th in (0.0, 0.05)) + \
    ((900, 80, 100, 0.0, True), (900, 80, 100, 0.05, True))


def e2e_proposal_inputs(shapes, mode):
    import torch

    T = sum(h * w for h, w in shapes)
    step = 1 / 64 if mode != "ties" else 1.0
    g = torch.Generator(device="cpu").manual_seed(3)
    logit = torch.randint(int(-8.0 / step), int(6.0 / step), (T,), generator=g).float() * step
    g = torch.Generator(device="cpu").manual_seed(4)
    c = torch.rand(T, 2, generator=g)
    wh = torch.rand(T, 2, generator=g) * (0.3 if mode != "fallback" else 0.0) + (0.02 if mode != "fallback" else 0.9)
    if mode == "fallback":
        c = c * 0.01 + 0.5
    return logit, torch.cat([c - wh / 2, c + wh / 2], 1).clamp(0, 1).contiguous()


def e2e_detection_inputs(Q, K):
    import torch

    g = torch.Generator(device="cpu").manual_seed(5)
    logits = torch.randint(-600, 200, (Q, K), generator=g).float() / 64
    if K > 2:
        logits[:, 1] = float("-inf")
    if Q > 10:
        logits[5, 0] = float("nan")
    c = torch.rand(Q, 2, generator=g)
    wh = torch.rand(Q, 2, generator=g) * 0.4 + 0.02
    boxes = torch.cat([c, wh], 1).contiguous()
    if Q > 10:
        boxes[7, 2] = float("inf")
    return logits, boxes, torch.tensor([1024.0, 683.0, 1024.0, 683.0])
