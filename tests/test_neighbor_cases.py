"""CPU: the model of the sparse all-pairs comparison (tests/neighbor_cases.py) -- the rule applied to compare_cases.ref_compare against a
direct per-pair walk, on random small collections and on the rule's edges, and the wrong models a test built on it must catch."""
import numpy as np
import pytest

from tests import compare_cases as CC
from tests import neighbor_cases as NC

U64, U32 = np.uint64, np.uint32
CAPS = CC.read_caps()


def random_small(rng, n, most):
    """n small sets that like to hold 0 and 2^64-1, some of them empty"""
    pool = np.array([0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 1 << 32, 1 << 63, CC.MAX - 1, CC.MAX], U64)
    return [np.sort(rng.choice(pool, int(rng.integers(0, most + 1)), replace=False)) for _ in range(n)]


PARAMS = [dict(), dict(min_shared=0), dict(min_shared=2), dict(min_shared=99), dict(num=1, den=2), dict(num=1, den=1), dict(num=0, den=7),
          dict(upper=True), dict(min_shared=2, num=1, den=3, upper=True)]


@pytest.mark.parametrize("seed", range(4))
def test_model_equals_the_pair_walk(seed):
    rng = np.random.default_rng(900 + seed)
    A, B = random_small(rng, 7, 9), random_small(rng, 5, 9)
    for limit in (0, 1, 3, 6, 100):
        for p in PARAMS:
            assert NC.same(NC.ref_neighbors(A, B, limit, **p), NC.walk_neighbors(A, B, limit, **p)), (limit, p)
            assert NC.same(NC.ref_neighbors(A, A, limit, **p), NC.walk_neighbors(A, A, limit, **p)), (limit, p)


def test_walk_pair_on_the_limit_landings_and_extremes():
    for a, b, limit, shared, total in CC.limit_landings():
        assert NC.walk_pair(a, b, limit) == (shared, total) == CC.ref_pair(a, b, limit)
    sets, _, _ = CC.extreme_values(CAPS["CMP_WINDOW"])
    for a in sets:
        for b in sets:
            for limit in (0, 1, 2, 4):
                assert NC.walk_pair(a, b, limit) == CC.ref_pair(a, b, limit)
    assert NC.walk_pair(CC.u64([0, CC.MAX]), CC.u64([0, CC.MAX]), 0) == (2, 2) and NC.walk_pair(CC.u64([]), CC.u64([]), 0) == (0, 0)


def edge_pair():
    """a pair with shared 2, total 8 and an identical pair (shared == total == 5), an empty set among them"""
    a, b = CC.u64([10, 20, 30, 40, 50]), CC.u64([5, 20, 35, 40, 60])
    return [a, CC.u64([]), b], [b, a]


def test_the_rule_at_its_edges():
    A, B = edge_pair()
    sh, tt = CC.ref_compare(A, B, 0)
    assert (sh[0, 0], tt[0, 0]) == (2, 8) and (sh[0, 1], tt[0, 1]) == (5, 5) and sh[1].tolist() == [0, 0]
    # a threshold met exactly is kept, one step above it is dropped
    for num, den, kept in ((2, 8, True), (1, 4, True), (3, 8, False), (2, 7, False), ((1 << 30) // 4, 1 << 30, True), ((1 << 30) // 4 + 1, 1 << 30, False)):
        o, t, s, tot = NC.ref_neighbors(A, B, 0, num=num, den=den)
        assert (0 in t[int(o[0]):int(o[1])].tolist()) is kept, (num, den)
        assert NC.same((o, t, s, tot), NC.walk_neighbors(A, B, 0, num=num, den=den))
    # num == den: identical sets only; num == 0 with den != 0: every sharing pair, as without the condition
    o, t, s, tot = NC.ref_neighbors(A, B, 0, num=5, den=5)
    assert o.tolist() == [0, 1, 1, 2] and t.tolist() == [1, 0] and s.tolist() == [5, 5] and tot.tolist() == [5, 5]
    assert NC.same(NC.ref_neighbors(A, B, 0, num=0, den=9), NC.ref_neighbors(A, B, 0))
    # min_shared: met exactly, 0 taken as 1, nothing shared never listed
    assert NC.ref_neighbors(A, B, 0, min_shared=2)[1].tolist() == [0, 1, 0, 1] and NC.ref_neighbors(A, B, 0, min_shared=3)[1].tolist() == [1, 0]
    assert NC.same(NC.ref_neighbors(A, B, 0, min_shared=0), NC.ref_neighbors(A, B, 0, min_shared=1))
    assert NC.ref_neighbors(A, B, 0)[0].tolist() == [0, 2, 2, 4]  # the empty row lists nothing
    # the products do not wrap: shared and total near 2^32 against a denominator near 2^32
    big = (1 << 32) - 1
    assert NC.keeps(big - 1, big, 0, 1, 1, big - 1, big) and not NC.keeps(big - 2, big, 0, 1, 1, big - 1, big)
    # under a limit the total is the walked count, not |a| + |b| - shared
    o, t, s, tot = NC.ref_neighbors(A, B, 3)
    assert tot.tolist() == [3] * len(tot) and s.tolist() == [1, 3, 3, 1]  # (a, b), (a, a); (b, b), (b, a)


def test_upper_keeps_j_above_i_only():
    A, _ = edge_pair()
    A = A + [A[0]]
    full, up = NC.ref_neighbors(A, A, 0), NC.ref_neighbors(A, A, 0, upper=True)
    rows = lambda x: {(i, int(x[1][p])): (int(x[2][p]), int(x[3][p])) for i in range(len(A)) for p in range(int(x[0][i]), int(x[0][i + 1]))}
    f, u = rows(full), rows(up)
    assert all(j > i for i, j in u) and {(i, j): v for (i, j), v in f.items() if j > i} == u
    assert {**u, **{(j, i): v for (i, j), v in u.items()}} == {k: v for k, v in f.items() if k[0] != k[1]}  # the result and its transpose: the off-diagonal


def test_expected_tiles():
    R = CAPS["CMP_ROWS"]
    for n, T in ((1, 1), (R, 1), (R + 1, 2), (2 * R + 1, 3), (46400, 2900)):
        assert NC.expected_tiles(n, n, False, CAPS) == (T * T, 0)
        assert NC.expected_tiles(n, n, True, CAPS) == (T * (T + 1) // 2, T * (T - 1) // 2)
    # 33 x 17: tile rows 1 and 2 lose (1, 0), (2, 0), (2, 1); 17 x 33: only (1, 0); one column of tiles: all but the first
    assert NC.expected_tiles(33, 17, True, CAPS) == (3, 3) and NC.expected_tiles(17, 33, True, CAPS) == (5, 1) and NC.expected_tiles(33, 1, True, CAPS) == (1, 2)
    brute = lambda na, nb: sum(1 for r in range(-(-na // R)) for c in range(-(-nb // R)) if c * R + R - 1 <= r * R)
    for na, nb in ((33, 17), (17, 33), (100, 40), (40, 100), (49, 49)):
        assert NC.expected_tiles(na, nb, True, CAPS)[1] == brute(na, nb)
    assert NC.plan_figures("k_cmp_tile_nb, 3 x 2 pairs, tiles=12 skipped=3 rounds=40 runs=2") == dict(tiles=12, skipped=3, rounds=40, runs=2)


def test_top_rows():
    o, t, s = np.array([0, 4, 4, 5], U64), np.array([1, 3, 4, 9, 2], U32), np.array([5, 7, 5, 7, 1], U32)
    assert [x.tolist() for x in NC.top_rows(o, t, s, 3)] == [[0, 3, 3, 4], [3, 9, 1, 2], [7, 7, 5, 1]]


# ---- wrong models: each differs from the walk on a case the tests run ----
def test_wrong_models_are_caught():
    A, B = edge_pair()
    right = NC.walk_neighbors(A, B, 0, num=2, den=8)

    def strict(sh, tt, num, den):  # > where the rule says >=
        o, t = np.zeros(sh.shape[0] + 1, U64), []
        for i in range(sh.shape[0]):
            t += [j for j in range(sh.shape[1]) if sh[i, j] >= 1 and int(sh[i, j]) * den > num * int(tt[i, j])]
            o[i + 1] = len(t)
        return o, np.array(t, U32)

    sh, tt = CC.ref_compare(A, B, 0)
    assert not NC.same(strict(sh, tt, 2, 8), right[:2])
    # j >= i where the rule says j > i: the diagonal slips in
    S = A + [A[0]]
    up = NC.walk_neighbors(S, S, 0, upper=True)
    loose = NC.filter_matrices(*CC.ref_compare(S, S, 0))
    loose_up = [(i, int(loose[1][p])) for i in range(len(S)) for p in range(int(loose[0][i]), int(loose[0][i + 1])) if int(loose[1][p]) >= i]
    assert len(loose_up) > len(up[1]) and (0, 0) in loose_up
    # total taken as |a| + |b| - shared under a limit
    sh3, tt3 = CC.ref_compare(A, B, 3)
    sizes = np.add.outer([len(a) for a in A], [len(b) for b in B]).astype(U32) - sh3
    assert not NC.same(NC.filter_matrices(sh3, sizes), NC.walk_neighbors(A, B, 3))
    # columns not ascending
    o, t, s, tot = NC.walk_neighbors(A, B, 0)
    assert not NC.same((o, t[::-1], s[::-1], tot[::-1]), (o, t, s, tot))
