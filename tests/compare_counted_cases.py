"""What the abundance-weighted comparison's tests share: the references in Python integers -- the per-pair walk that gives (shared,
total, dot, min_sum), the squared norms, the float formulas -- and the case builders, which take their values and round figures from
tests/compare_cases and attach counts (tests/test_compare_counted_cases.py re-derives the references by a second formulation on the
CPU, tests/test_gpu_compare_counted.py runs the cases)."""
import math

import numpy as np

from tests import compare_cases as CC

U64, U32 = np.uint64, np.uint32
MAX = (1 << 64) - 1
CMAX = (1 << 32) - 1  # the largest count


# ---- the references, in Python integers ----
def ones(sets):
    return [np.ones(len(s), U32) for s in sets]


def ref_pair(a, ca, b, cb, limit):
    """(shared, total, dot, min_sum) of one pair: the first `limit` distinct values of the union ascending (0: all); over those both
    sets hold, the sum of the products of the two counts, cut at 2^64 - 1, and the sum of their minima"""
    da = {int(v): int(c) for v, c in zip(a, ca)}
    db = {int(v): int(c) for v, c in zip(b, cb)}
    walked = sorted(set(da) | set(db))
    if limit:
        walked = walked[:limit]
    both = [v for v in walked if v in da and v in db]
    return len(both), len(walked), min(sum(da[v] * db[v] for v in both), MAX), sum(min(da[v], db[v]) for v in both)


def ref_compare(A, CA, B, CB, limit):
    """lists of sorted distinct u64 arrays and their u32 counts (None: every count 1) -> shared, total (u32), dot, min_sum (u64)"""
    CA = ones(A) if CA is None else CA
    CB = ones(B) if CB is None else CB
    shape = (len(A), len(B))
    sh, tt, dt, ms = np.zeros(shape, U32), np.zeros(shape, U32), np.zeros(shape, U64), np.zeros(shape, U64)
    for i in range(len(A)):
        for j in range(len(B)):
            sh[i, j], tt[i, j], dt[i, j], ms[i, j] = ref_pair(A[i], CA[i], B[j], CB[j], limit)
    return sh, tt, dt, ms


def ref_sumsq(C):
    return np.array([min(sum(int(c) * int(c) for c in cs), MAX) for cs in C], U64)


def ref_totals(C):
    return np.array([sum(int(c) for c in cs) for cs in C], U64)


def ref_cosine(dot, qa, qb):
    """float64 [n_a, n_b]: dot / (sqrt(qa[i]) * sqrt(qb[j])); 0.0 where a norm is 0, NaN where dot or either norm is saturated"""
    out = np.zeros(dot.shape, np.float64)
    for i in range(dot.shape[0]):
        for j in range(dot.shape[1]):
            d, a, b = int(dot[i, j]), int(qa[i]), int(qb[j])
            if MAX in (d, a, b):
                out[i, j] = math.nan
            elif a and b:
                out[i, j] = float(d) / (math.sqrt(float(a)) * math.sqrt(float(b)))
    return out


def ref_angular(cos):
    return np.array([[math.nan if math.isnan(x) else 1.0 - 2.0 * math.acos(min(x, 1.0)) / math.pi for x in row] for row in cos], np.float64).reshape(cos.shape)


def ref_weighted_jaccard(ms, ta, tb):
    out = np.zeros(ms.shape, np.float64)
    for i in range(ms.shape[0]):
        for j in range(ms.shape[1]):
            den = float(int(ta[i])) + float(int(tb[j])) - float(int(ms[i, j]))
            out[i, j] = float(int(ms[i, j])) / den if den else 0.0
    return out


def ref_bray_curtis(ms, ta, tb):
    out = np.zeros(ms.shape, np.float64)
    for i in range(ms.shape[0]):
        for j in range(ms.shape[1]):
            den = float(int(ta[i])) + float(int(tb[j]))
            out[i, j] = 1.0 - 2.0 * float(int(ms[i, j])) / den if den else 0.0
    return out


# ---- counts for the sets of tests/compare_cases ----
def attach(sets, lo, hi, seed):
    """random counts lo .. hi, one array per set"""
    rng = np.random.default_rng(seed)
    return [rng.integers(lo, hi + 1, len(s)).astype(U32) for s in sets]


def flat(counts):
    return np.concatenate(counts) if counts and sum(len(c) for c in counts) else np.zeros(0, U32)


# ---- the cases ----
def hand_case():
    """compare_cases.hand_case with counts; limit -> (dot, min_sum), written out.  shared and total are compare_cases'."""
    A, B, plain = CC.hand_case()           # A = {1 3 5 7} {} {2 3}      B = {3 4 5} {7}
    CA = [np.array([2, 3, 1, 4], U32), np.zeros(0, U32), np.array([5, 2], U32)]
    CB = [np.array([2, 7, 6], U32), np.array([3], U32)]
    want = {
        0: ([[3 * 2 + 1 * 6, 4 * 3], [0, 0], [2 * 2, 0]], [[2 + 1, 3], [0, 0], [2, 0]]),  # 3 and 5 | 7 | - | - | 3 | -
        1: ([[0, 0], [0, 0], [0, 0]], [[0, 0], [0, 0], [0, 0]]),                          # one value walked, never a shared one
        2: ([[3 * 2, 0], [0, 0], [2 * 2, 0]], [[2, 0], [0, 0], [2, 0]]),                  # 1 3 | 1 3 | 3 4 | 7 | 2 3 | 2 3
        3: ([[3 * 2, 0], [0, 0], [2 * 2, 0]], [[2, 0], [0, 0], [2, 0]]),                  # 1 3 4 | 1 3 5 | 3 4 5 | 7 | 2 3 4 | 2 3 7
        100: ([[12, 12], [0, 0], [4, 0]], [[3, 3], [0, 0], [2, 0]]),
    }
    return A, CA, B, CB, plain, want


def saturation_cases():
    """(A, CA, B, CB, dot, min_sum): counts of 2^32 - 1.  With M = 2^32 - 1: M * M = 2^64 - 2^33 + 1 fits; M * M + M = 2^64 - 2^32
    fits; 2 * M * M does not.  Row 0 holds a saturated cell between unsaturated ones; row 1 saturates on its second value and walks a
    third (saturation is kept); min_sum stays exact everywhere."""
    M = CMAX
    A = [CC.u64([10, 20]), CC.u64([10, 20, 30])]
    CA = [np.array([M, M], U32), np.array([M, M, 7], U32)]
    B = [CC.u64([10]), CC.u64([10, 20]), CC.u64([10, 20]), CC.u64([5, 10, 20, 30])]
    CB = [np.array([M], U32), np.array([M, M], U32), np.array([M, 1], U32), np.array([9, M, M, 3], U32)]
    dot = [[M * M, MAX, M * M + M, MAX], [M * M, MAX, M * M + M, MAX]]
    ms = [[M, 2 * M, M + 1, 2 * M], [M, 2 * M, M + 1, 2 * M + 3]]
    assert M * M == (1 << 64) - (1 << 33) + 1 and M * M + M == (1 << 64) - (1 << 32) < MAX < 2 * M * M
    return A, CA, B, CB, dot, ms


def limit_landings():
    """compare_cases.limit_landings with counts: (a, ca, b, cb, limit, shared, total, dot, min_sum).  In the first pair 20 has the counts
    3 and 5 and 40 the counts 2 and 7: a limit that lands on a shared value includes its product and minimum, the limit one before
    leaves them out."""
    out = []
    for a, b, limit, sh, tt in CC.limit_landings():
        ca, cb = (np.arange(len(a)) % 4 + 1).astype(U32), (np.arange(len(b)) % 3 + 5).astype(U32)
        if len(a) == 5 and int(a[1]) == 20:
            ca, cb = np.array([1, 3, 1, 2, 1], U32), np.array([1, 5, 1, 7, 1], U32)
            dot, ms = {2: (0, 0), 3: (15, 3), 4: (15, 3), 6: (29, 5), 8: (29, 5), 9: (29, 5)}[limit]
        else:
            dot, ms = ref_pair(a, ca, b, cb, limit)[2:]
        out.append((a, ca, b, cb, limit, sh, tt, dot, ms))
    return out


def pool_counts(masks, lo, hi, seed):
    """for compare_cases.small_pool_sets: dense [n, 64] count vectors (0: the set does not hold the value) and the per-set count arrays"""
    rng = np.random.default_rng(seed)
    bits = ((masks[:, None] >> np.arange(64, dtype=U64)[None, :]) & U64(1)).astype(np.int64)
    dense = bits * rng.integers(lo, hi + 1, bits.shape)
    return dense, [row[row > 0].astype(U32) for row in dense]


def dense_compare(da, db):
    """limit 0 on dense count vectors over one pool ([n, P], 0: absent) -> shared, total, dot, min_sum: the second formulation"""
    da, db = np.asarray(da, np.int64), np.asarray(db, np.int64)
    ha, hb = (da > 0).astype(np.int64), (db > 0).astype(np.int64)
    shared = ha @ hb.T
    total = ha.sum(1)[:, None] + hb.sum(1)[None, :] - shared
    ms = np.zeros(shared.shape, np.int64)
    for k in range(da.shape[1]):
        ms += np.minimum(da[:, k][:, None], db[:, k][None, :])
    return shared.astype(U32), total.astype(U32), (da @ db.T).astype(U64), ms.astype(U64)


def repeated_sequences(length=20_000, repeat=3_000):
    """compare_cases.mutated_sequences, each with its own first `repeat` bases appended: what lies there occurs twice"""
    return [s + s[:repeat] for s in CC.mutated_sequences(length)]
