"""CPU: the references and the case builders of tests/compare_cases.py -- ref_compare against a brute-force loop over Python sets, the
restatement of k_cmp_tile's round rule against ref_compare, and every builder's claim re-derived from its sets alone."""
import itertools

import numpy as np
import pytest

from tests import compare_cases as CC

U64 = np.uint64
CAPS = CC.read_caps()
R, COLS, W = CAPS["CMP_ROWS"], CAPS["CMP_COLS"], CAPS["CMP_WINDOW"]


def brute(A, B, limit):
    sh, tt = np.zeros((len(A), len(B)), np.uint32), np.zeros((len(A), len(B)), np.uint32)
    for i, a in enumerate(A):
        for j, b in enumerate(B):
            sa, sb = set(int(v) for v in a), set(int(v) for v in b)
            walked = sorted(sa | sb)
            if limit:
                walked = walked[:limit]
            tt[i, j] = len(walked)
            sh[i, j] = sum(1 for v in walked if v in sa and v in sb)
    return sh, tt


def random_small(rng, n, most):
    """n small sets that like to hold 0, 2^64-2 and 2^64-1"""
    pool = np.array([0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 1 << 32, 1 << 63, CC.MAX - 2, CC.MAX - 1, CC.MAX], U64)
    return [np.sort(rng.choice(pool, int(rng.integers(0, most + 1)), replace=False)) for _ in range(n)]


def test_caps_are_read_from_the_kernel_file():
    assert set(CAPS) >= {"CMP_ROWS", "CMP_COLS", "CMP_WINDOW", "CMP_BLOCKS_PER_CU", "CMP_BT_SMALL", "CMP_BT_BLOCKS_PER_CU"}
    assert R * COLS == 256 and W >= 8 and (R + COLS) * W * 8 * 2 <= 160 * 1024  # two workgroups' windows fit a CU's LDS


def test_ref_compare_against_python_sets():
    rng = np.random.default_rng(1)
    for _ in range(20):
        A, B = random_small(rng, 4, 12), random_small(rng, 3, 12)
        for limit in (0, 1, 2, 3, 7, 12, 30):
            got, want = CC.ref_compare(A, B, limit), brute(A, B, limit)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), limit
    assert [list(s) for s in CC.ref_bottom([CC.u64([5, 1, 9]), CC.u64([]), CC.u64([4])], 2)] == [[1, 5], [], [4]]


@pytest.mark.parametrize("window", [1, 2, 3, 4, 5])
def test_round_rule_is_exact(window):
    rng = np.random.default_rng(100 + window)
    most_rounds = 0
    for _ in range(40):
        A, B = random_small(rng, int(rng.integers(1, 5)), 14), random_small(rng, int(rng.integers(1, 5)), 14)
        for limit in (0, 1, 2, 3, window, window + 1, 2 * window + 1, 40):
            rounds, sh, tt = CC.tile_rounds(A, B, limit, window)
            want = CC.ref_compare(A, B, limit)
            assert np.array_equal(sh, want[0]) and np.array_equal(tt, want[1]), (limit, A, B)
            assert 1 <= rounds <= sum(len(s) // window for s in A + B) + 1  # every round but the last moves some cursor by a full window
            most_rounds = max(most_rounds, rounds)
    assert most_rounds >= 3


def test_hand_case():
    A, B, want = CC.hand_case()
    assert sorted(want) == [0, 1, 2, 3, 100] and any(len(s) == 0 for s in A)
    for limit, (sh, tt) in want.items():
        got = brute(A, B, limit)
        assert got[0].tolist() == sh and got[1].tolist() == tt, limit


def test_window_edges_claims():
    A, B, claim = CC.window_edges(W)
    assert [len(s) for s in A] == claim["sizes"] == [len(s) for s in B] == [0, 1, W - 1, W, W + 1, 2 * W, 2 * W + 1, 3 * W + 5]
    assert len(np.unique(np.concatenate(A + B))) <= claim["pool"] == 4 * W
    assert claim["limits"][:6] == [0, 1, W - 1, W, W + 1, 2 * W + 1] and claim["limits"][6] > claim["pool"]
    assert all(np.all(np.diff(s.astype(object)) > 0) for s in A + B if len(s) > 1)
    # the sizes take the rule through one round and through several
    assert CC.tile_rounds(A[:4], B[:4], 0, W)[0] == 1 and CC.tile_rounds(A, B, 0, W)[0] >= 3


def test_tile_edges_claims():
    A, B, claim = CC.tile_edges(R, COLS)
    assert claim["shapes"] == list(itertools.product((1, R - 1, R, R + 1, 2 * R + 1), (1, COLS - 1, COLS, COLS + 1, 2 * COLS + 1)))
    assert len(A) >= 2 * R + 1 and len(B) >= 2 * COLS + 1 and all(15 <= len(s) <= 25 and np.all(s[1:] > s[:-1]) for s in A + B)
    assert CC.n_tiles(1, 1, CAPS) == 1 and CC.n_tiles(R + 1, COLS, CAPS) == 2 and CC.n_tiles(2 * R + 1, 2 * COLS + 1, CAPS) == 9
    sh, _ = CC.ref_compare(A[:5], B[:5], 0)
    assert sh.max() > 0  # the pool is small enough for the sets to share values


def test_extreme_values_claims():
    S, T, claim = CC.extreme_values(W)
    assert S is T
    has = [(0 in [int(v) for v in s[:1]], CC.MAX in [int(v) for v in s[-1:]]) for s in S]
    assert {(True, True), (True, False), (False, True), (False, False)} <= set(has)
    assert any(s.tolist() == [CC.MAX] for s in S)
    e = S[claim["edge_index"]]
    assert len(e) == W + 1 and int(e[W - 1]) == CC.MAX - 1 and int(e[W]) == CC.MAX
    assert 0 in claim["limits"] and W in claim["limits"] and W + 1 in claim["limits"]
    sh, tt = brute(S, S, 0)
    assert all(sh[i, i] == tt[i, i] == len(S[i]) for i in range(len(S)))


def test_skew_claims():
    cases = CC.skew_cases(W)
    A, B = cases["low"]
    assert len(A[0]) == 5 * W and int(A[0][-1]) < min(int(s[0]) for s in B)
    assert CC.tile_rounds(A, B, 0, W)[0] == 5  # four full windows of the low set alone, then everything else
    A, B = cases["gap"]
    assert len(A[0]) == 3 * W and all(not np.any((s >= A[0][0]) & (s <= A[0][-1])) for s in B)
    assert all(int(s[0]) < int(A[0][0]) and int(s[-1]) > int(A[0][-1]) for s in B)
    assert CC.tile_rounds(A, B, 0, W)[0] == 3
    A, B = cases["dense"]
    assert len(A) == 1 and len(A[0]) == 10 * W and len(B) == 15 and all(len(s) == 3 for s in B)
    assert CC.tile_rounds(A, B, 0, W)[0] == 10
    At, Bt = cases["dense_t"]
    assert At is B and len(Bt) == 1 and Bt[0] is A[0]


def test_limit_landings_claims():
    for a, b, limit, sh, tt in CC.limit_landings():
        got = brute([a], [b], limit)
        assert (int(got[0][0, 0]), int(got[1][0, 0])) == (sh, tt), (a, b, limit)
    a, b = CC.limit_landings()[0][:2]
    union, both = sorted(set(a.tolist()) | set(b.tolist())), set(a.tolist()) & set(b.tolist())
    assert union[2] in both and union[1] not in both and union[2] in both and union[3] not in both and len(union) == 8


def test_mash_shape_claims():
    sets, claim = CC.mash_shape()
    assert len(sets) == 40 and all(len(s) == 1000 for s in sets) and len(np.unique(np.concatenate(sets))) <= 3000 and claim["limit"] == 1000
    assert CC.tile_rounds(sets[:R], sets[:COLS], 1000, W)[0] >= 3


def test_small_pool_sets_and_the_mask_reference():
    sets, masks = CC.small_pool_sets(300)
    assert all(2 <= len(s) <= 3 and int(s[-1]) < 64 for s in sets) and {len(s) for s in sets} == {2, 3}
    sh, tt = CC.mask_compare(masks[:40], masks[:30])
    want = CC.ref_compare(sets[:40], sets[:30], 0)
    assert np.array_equal(sh, want[0]) and np.array_equal(tt, want[1])


def test_bottom_sets_and_sequences():
    sets, sizes = CC.bottom_sets()
    assert sizes == list(range(71)) + [1025] and [len(s) for s in sets] == sizes
    seqs = CC.mutated_sequences(length=5000)
    assert len(seqs) == 5 and all(len(s) == 5000 and set(s) <= set(b"ACGT") for s in seqs) and seqs[0] == seqs[1]
    diff = [sum(x != y for x, y in zip(seqs[0], s)) / 5000 for s in seqs]
    assert diff[1] == 0 and 0.003 < diff[2] < 0.02 and 0.03 < diff[3] < 0.07 and diff[4] > 0.6
