"""CPU: the cases of tests/neighbor_counted_cases.py are what they claim.  Every expectation the GPU test uses is re-derived by a second
formulation -- compare_counted_cases.dense_compare on dense count vectors, no walk -- and the conditions that make a case worth running
are asserted here, where a change to a builder shows at once."""
import numpy as np
import pytest

from tests import compare_cases as CC
from tests import compare_counted_cases as WC
from tests import neighbor_cases as NC
from tests import neighbor_counted_cases as NW

CAPS = CC.read_caps()
R, COLS, W = CAPS["CMP_ROWS"], CAPS["CMP_COLS"], CAPS["CMP_WINDOW"]
NAMES = sorted(NW.cases())


@pytest.mark.parametrize("name", NAMES)
def test_the_model_agrees_with_the_dense_formulation(name):
    """limit 0: the walk's four matrices are dense_compare's, cell for cell -- so every filtered expectation is too"""
    case = NW.cases()[name]
    want = WC.dense_compare(*NW.densify(case))
    got = NW.reference(case, 0)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g.astype(np.uint64), w.astype(np.uint64)), name
    for limit, p in case.runs:
        if limit == 0:
            assert NC.same(NW.expected(case, 0, p), NW.filter_weighted(*want, **NW.rule(p))), (name, p)


def test_limited_runs_against_the_pair_walk():
    """the runs with a limit have no dense formulation: shared and total from neighbor_cases.walk_pair (another walk), and the weights of a
    limited pair are those of the pair's sets cut to the values up to the last one walked"""
    for name, case in NW.cases().items():
        A, CA, B, CB = NW.operands(case)
        for limit, p in case.runs:
            if limit == 0:
                continue
            sh, tt, dt, ms = NW.reference(case, limit)
            for i in range(len(A)):
                for j in range(len(B)):
                    assert (int(sh[i, j]), int(tt[i, j])) == NC.walk_pair(A[i], B[j], limit), (name, i, j)
                    last = np.union1d(A[i], B[j])[:limit][-1:]  # the last value walked (none: two empty sets)
                    ka, kb = A[i] <= (last[0] if len(last) else 0), B[j] <= (last[0] if len(last) else 0)
                    cut = WC.ref_pair(A[i][ka], CA[i][ka], B[j][kb], CB[j][kb], 0) if len(last) else (0, 0, 0, 0)
                    assert (int(dt[i, j]), int(ms[i, j])) == cut[2:], (name, i, j)


@pytest.mark.parametrize("name", NAMES)
def test_every_run_keeps_and_drops_what_it_should(name):
    case = NW.cases()[name]
    A, CA, B, CB = NW.operands(case)
    for limit, p in case.runs:
        sh, tt, dt, ms = NW.reference(case, limit)
        off, tgt, s, t, d, m = NW.expected(case, limit, p)
        assert len(tgt) >= 1, (name, p, "keeps nothing")
        if NW.thresholded(p):  # the threshold decides something: a pair that shares a value is dropped
            r = NW.rule(p)
            dropped = sum(1 for i in range(sh.shape[0]) for j in range(sh.shape[1]) if sh[i, j] and not NC.keeps(sh[i, j], tt[i, j], i, j, **r))
            assert dropped >= 1, (name, p, "drops no pair that shares a value")
        if CA is not None and CB is not None:  # the weights say something shared does not: one kept pair with dot != min_sum != shared
            assert np.any((d != m) & (m != s.astype(np.uint64))), (name, p)
        elif CA is not None or CB is not None:  # one side counts 1 per value: every minimum is 1, the products are the other side's counts
            assert np.array_equal(m, s.astype(np.uint64)) and np.any(d != m), (name, p)
        if CA is None and CB is None:
            assert np.array_equal(d, s.astype(np.uint64)) and np.array_equal(m, s.astype(np.uint64)), name


def test_the_shapes_reach_the_paths_they_are_for():
    cases = NW.cases()
    A, CA, B, CB = NW.operands(cases["window_edges"])
    assert sorted(len(s) for s in A) == [0, 1, W - 1, W, W + 1, 2 * W, 2 * W + 1, 3 * W + 5]
    assert CC.tile_rounds(A, B, 0, W)[0] > 2  # several rounds: values staged but not consumed are staged again, with their counts
    for name in ("skew_low", "skew_gap", "skew_dense", "skew_dense_t"):
        a, _, b, _ = NW.operands(cases[name])
        assert CC.tile_rounds(a, b, 0, W)[0] >= 3 and len(a) <= R and len(b) <= COLS, name  # one tile, one set many windows ahead
    for n in (15, 16, 17, 33):
        case = cases["tiles_%d" % n]
        assert len(case.A) == n and case.B is None and [p for _, p in case.runs] == [{}, dict(upper=True)]
        up = NW.expected(case, 0, dict(upper=True))
        rows = np.repeat(np.arange(n), np.diff(up[0]).astype(np.int64))
        assert (up[1] > rows).all() and len(up[1])  # no (i, i), nothing below the diagonal
        full = NW.expected(case, 0, {})
        assert len(full[1]) == 2 * len(up[1]) + n  # every set of the case is non-empty: the diagonal is kept without upper
    assert NC.expected_tiles(33, 33, True, CAPS) == (6, 3) and NC.expected_tiles(17, 17, True, CAPS) == (3, 1)
    # the second run and the stride loop
    rules = cases["rules_40"]
    assert all(len(NW.expected(rules, 0, p)[1]) > 8 for _, p in rules.runs)
    assert len(rules.A) == 40 and CC.n_tiles(40, 40, CAPS) == 9 > 2 * 2  # a cap of 2: five and four tiles a workgroup
    assert [p for _, p in rules.runs] == NW.ALL_RULES and len(NW.ALL_RULES) == 6
    big = cases["pool_70x50"]
    assert (len(big.A), len(big.B)) == (70, 50) and CC.n_tiles(70, 50, CAPS) == 20


def test_hand_saturation_and_landings_are_written_out():
    """the three cases the GPU test takes straight from compare_counted_cases: their written-out numbers are the walk's"""
    A, CA, B, CB, plain, want = WC.hand_case()
    for limit, (dot, ms) in want.items():
        sh, tt, dt, mm = WC.ref_compare(A, CA, B, CB, limit)
        assert sh.tolist() == plain[limit][0] and tt.tolist() == plain[limit][1] and dt.tolist() == dot and mm.tolist() == ms
        kept = NW.filter_weighted(sh, tt, dt, mm)
        assert len(kept[1]) == int(np.count_nonzero(sh)) and (limit != 1 or len(kept[1]) == 0)
    A, CA, B, CB, dot, ms = WC.saturation_cases()
    sh, tt, dt, mm = WC.ref_compare(A, CA, B, CB, 0)
    assert dt.tolist() == dot and mm.tolist() == ms and (sh > 0).all() and WC.MAX in dt and int(mm[1, 3]) == 2 * WC.CMAX + 3
    on = [(limit, sh, dot) for a, ca, b, cb, limit, sh, tt, dot, m in WC.limit_landings() if len(a) == 5 and int(a[1]) == 20]
    assert (3, 1, 15) in on and (2, 0, 0) in on and (6, 2, 29) in on  # on a shared value: included; one before: not
