"""CPU: the references of tests/compare_counted_cases.py against a second, independent formulation -- sets as dense count vectors over
a small pool, dot as an integer matrix product, min_sum as a dense minimum, the limit as a cut of the union's running count -- and the
hand, landing and saturation cases as they are written out."""
import math

import numpy as np
import pytest

from tests import compare_cases as CC
from tests import compare_counted_cases as WC

U64, U32 = np.uint64, np.uint32


def dense_pair(va, vb, limit):
    """one pair on dense count vectors: keep the pool positions up to the limit-th value of the union, then count there"""
    union = (va > 0) | (vb > 0)
    keep = union & (np.cumsum(union) <= limit) if limit else union
    a, b = va * keep, vb * keep
    both = (a > 0) & (b > 0)
    return int(both.sum()), int(keep.sum()), int((a * b).sum()), int(np.minimum(a, b).sum())


@pytest.mark.parametrize("seed", range(4))
def test_the_walk_equals_the_dense_formulation(seed):
    rng = np.random.default_rng(seed)
    P, na, nb = 14, 7, 6
    pool = np.sort(rng.choice(1 << 60, P, replace=False).astype(U64))
    VA = rng.integers(0, 6, (na, P)) * (rng.random((na, P)) < 0.6)
    VB = rng.integers(0, 6, (nb, P)) * (rng.random((nb, P)) < 0.6)
    VA[0] = 0  # an empty set
    A, CA = [pool[v > 0] for v in VA], [v[v > 0].astype(U32) for v in VA]
    B, CB = [pool[v > 0] for v in VB], [v[v > 0].astype(U32) for v in VB]
    for limit in (0, 1, 2, 3, 5, 8, P, P + 1):
        sh, tt, dt, ms = WC.ref_compare(A, CA, B, CB, limit)
        for i in range(na):
            for j in range(nb):
                assert (int(sh[i, j]), int(tt[i, j]), int(dt[i, j]), int(ms[i, j])) == dense_pair(VA[i], VB[j], limit), (limit, i, j)
        plain = CC.ref_compare(A, B, limit)  # shared and total are the unweighted compare's
        assert np.array_equal(sh, plain[0]) and np.array_equal(tt, plain[1])
    # limit 0 in one piece: a matrix product and a dense minimum
    sh, tt, dt, ms = WC.ref_compare(A, CA, B, CB, 0)
    for got, want in zip(WC.dense_compare(VA, VB), (sh, tt, dt, ms)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert np.array_equal(dt, (VA @ VB.T).astype(U64))
    assert np.array_equal(WC.ref_sumsq(CA), (VA * VA).sum(1).astype(U64)) and np.array_equal(WC.ref_totals(CA), VA.sum(1).astype(U64))
    # an uncounted operand counts 1: dot = min_sum = shared when both are, the other's counts summed over the intersection when one is
    sh1, tt1, dt1, ms1 = WC.ref_compare(A, None, B, None, 0)
    assert np.array_equal(dt1, sh1.astype(U64)) and np.array_equal(ms1, sh1.astype(U64)) and np.array_equal(sh1, sh) and np.array_equal(tt1, tt)
    half = WC.ref_compare(A, CA, B, None, 0)
    assert np.array_equal(half[2], (VA @ (VB > 0).T).astype(U64)) and np.array_equal(half[3], sh.astype(U64))


def test_the_hand_case_as_written():
    A, CA, B, CB, plain, want = WC.hand_case()
    assert [s.tolist() for s in A] == [[1, 3, 5, 7], [], [2, 3]] and [s.tolist() for s in B] == [[3, 4, 5], [7]]
    assert set(want) == set(plain) == {0, 1, 2, 3, 100}
    for limit, (dot, ms) in want.items():
        sh, tt, dt, m = WC.ref_compare(A, CA, B, CB, limit)
        assert sh.tolist() == plain[limit][0] and tt.tolist() == plain[limit][1], limit
        assert dt.tolist() == dot and m.tolist() == ms, limit
    assert want[0][0] == [[12, 12], [0, 0], [4, 0]] and want[0] == want[100]
    assert WC.ref_sumsq(CA).tolist() == [4 + 9 + 1 + 16, 0, 25 + 4] and WC.ref_totals(CB).tolist() == [15, 3]


def test_saturation_by_hand():
    A, CA, B, CB, dot, ms = WC.saturation_cases()
    M = WC.CMAX
    assert dot[0] == [18446744065119617025, WC.MAX, 18446744069414584320, WC.MAX]  # M * M, saturated, M * M + M, saturated
    sh, tt, dt, m = WC.ref_compare(A, CA, B, CB, 0)
    assert [[int(x) for x in r] for r in dt] == dot and [[int(x) for x in r] for r in m] == ms
    assert sh.tolist() == [[1, 2, 2, 2], [1, 2, 2, 3]]
    # the unsaturated cells beside the saturated one are exact, and a saturated sum stays saturated when more is added
    assert int(dt[0, 0]) < WC.MAX and int(dt[0, 2]) < WC.MAX and int(dt[1, 3]) == WC.MAX and ms[1][3] == 2 * M + 3
    assert WC.ref_sumsq([np.array([M, M], U32), np.array([M], U32), np.zeros(0, U32)]).tolist() == [WC.MAX, M * M, 0]
    # min_sum cannot overflow: fewer than 2^32 values of counts below 2^32
    assert (1 << 32) * M < WC.MAX


def test_limit_landings_as_written():
    cases = WC.limit_landings()
    assert len(cases) == len(CC.limit_landings())
    for a, ca, b, cb, limit, sh, tt, dot, ms in cases:
        assert WC.ref_pair(a, ca, b, cb, limit) == (sh, tt, dot, ms), (a, b, limit)
    first = {c[4]: c[7:] for c in cases[:6]}
    assert first[2] == (0, 0) and first[3] == (3 * 5, 3) and first[6] == (3 * 5 + 2 * 7, 3 + 2)  # on the shared value: in; one before: out


def test_the_float_formulas():
    dot = np.array([[12, 0, WC.MAX], [5, 9, 1]], U64)
    qa, qb = np.array([16, 9], U64), np.array([9, 0, 4], U64)
    cos = WC.ref_cosine(dot, qa, qb)
    assert cos[0, 0] == 1.0 and cos[0, 1] == 0.0 and math.isnan(cos[0, 2]) and cos[1, 0] == 5 / 9 and cos[1, 1] == 0.0 and cos[1, 2] == 1 / 6
    assert math.isnan(WC.ref_cosine(np.array([[1]], U64), np.array([WC.MAX], U64), np.array([1], U64))[0, 0])
    ang = WC.ref_angular(np.array([[1.0, 0.0, math.nan, 1.0000000000000002, 0.5]]))
    assert ang[0, 0] == 1.0 and ang[0, 1] == 0.0 and math.isnan(ang[0, 2]) and ang[0, 3] == 1.0 and ang[0, 4] == pytest.approx(1 / 3, rel=1e-15)
    ms, ta, tb = np.array([[3, 0], [0, 0]], U64), np.array([5, 0], U64), np.array([4, 0], U64)
    assert WC.ref_weighted_jaccard(ms, ta, tb).tolist() == [[3 / 6, 0.0], [0.0, 0.0]]
    assert WC.ref_bray_curtis(ms, ta, tb).tolist() == [[1 - 6 / 9, 1.0], [1.0, 0.0]]


def test_the_builders_claims():
    caps = CC.read_caps()
    assert caps["CMP_W_BLOCKS_PER_CU"] == 3 and caps["CMP_BLOCKS_PER_CU"] == 4 and caps["CMP_WINDOW"] == 128
    sets, masks = CC.small_pool_sets(50, seed=31)
    dense, counts = WC.pool_counts(masks, 1, 3, 5)
    assert dense.shape == (50, 64) and all(np.array_equal(np.nonzero(d)[0].astype(U64), s) for d, s in zip(dense, sets))
    assert all(len(c) == len(s) and c.min() >= 1 and c.max() <= 3 for c, s in zip(counts, sets))
    got = WC.dense_compare(dense[:9], dense[9:20])
    want = WC.ref_compare(sets[:9], counts[:9], sets[9:20], counts[9:20], 0)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    seqs = WC.repeated_sequences(2000, 300)
    assert len(seqs) == 5 and all(len(s) == 2300 and s[2000:] == s[:300] for s in seqs)
    c = WC.attach([np.arange(5), np.arange(0)], 1, 5, 3)
    assert [len(x) for x in c] == [5, 0] and c[0].dtype == U32 and 1 <= c[0].min() and c[0].max() <= 5 and WC.flat(c).shape == (5,)
