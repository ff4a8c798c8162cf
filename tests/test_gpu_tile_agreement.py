"""GPU: the four tile kernels of compare.hip (k_cmp_tile, k_cmp_tile_w and k_cmp_tile_nb, instantiations of one body, and
k_cmp_tile_nb_w, which keeps a copy of it) on one set of operands, every result compared for exact equality with the others: the sparse end keeps the non-zero cells of the dense end, row by
row in column order; with upper the cells above the diagonal; the counts change neither shared nor total; the weights of a kept pair
are those of its cell.  17 x 33 sets (a partial last tile row and column) and 33 sets against themselves, set sizes below, at and above
the window and beyond two rounds, from a pool of 600 values, at the limits 0, 1, 128 and 200.  The dense cells themselves are held
against the references of tests/compare_cases.py and tests/compare_counted_cases.py."""
import functools

import numpy as np
import pytest

from tests import compare_cases as CC
from tests import compare_counted_cases as WC
from tests import neighbor_cases as NC
from tests import neighbor_counted_cases as NW

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
CAPS = CC.read_caps()
SIZES = (0, 1, 127, 128, 129, 257, 300)
LIMITS = (0, 1, 128, 200)
N_A, N_B, POOL = 17, 33, 600
assert CAPS["CMP_WINDOW"] == 128 and N_A % CAPS["CMP_ROWS"] and N_B % CAPS["CMP_COLS"] and N_B > 2 * CAPS["CMP_COLS"]


@functools.lru_cache(None)
def operands():
    """A (17 sets), B (33 sets) and their counts 1 .. 9: every size of SIZES occurs in both"""
    rng = np.random.default_rng(41)
    pool = np.sort(rng.choice(1 << 40, POOL, replace=False).astype(U64))
    sets = [np.sort(rng.choice(pool, SIZES[k % len(SIZES)], replace=False)) for k in rng.permutation(N_A + N_B)]
    A, B = sets[:N_A], sets[N_A:]
    assert {len(s) for s in A} == set(SIZES) == {len(s) for s in B}
    return A, WC.attach(A, 1, 9, 42), B, WC.attach(B, 1, 9, 43)


@pytest.fixture(scope="module")
def dev(engine):
    """the operands on the device, without and with their counts"""
    A, CA, B, CB = operands()
    (oa, va), (ob, vb) = CC.collection(A), CC.collection(B)
    return dict(a=engine.sets_from_arrays(oa, va), b=engine.sets_from_arrays(ob, vb), ac=engine.sets_from_arrays_counted(oa, va, WC.flat(CA)),
                bc=engine.sets_from_arrays_counted(ob, vb, WC.flat(CB)))


def hits(h):
    return (h.offsets, h.target, h.shared, h.total) + ((h.dot, h.min_sum) if h.has_weights() else ())


def figures(h, kernel, n_a, n_b, upper):
    plan = h.plan()["plan"]
    fig = NC.plan_figures(plan)
    assert f": {kernel}," in plan and (fig["tiles"], fig["skipped"]) == NC.expected_tiles(n_a, n_b, upper, CAPS), plan


@pytest.mark.parametrize("limit", LIMITS)
def test_dense_against_sparse(dev, limit):
    A, _, B, _ = operands()
    cmp = dev["a"].compare(dev["b"], limit)
    sh, tt = cmp.fetch()
    want = CC.ref_compare(A, B, limit)
    assert np.array_equal(sh, want[0]) and np.array_equal(tt, want[1]) and "k_cmp_tile," in cmp.plan()["plan"]
    h = dev["a"].neighbors(dev["b"], limit, min_shared=1)
    assert NC.same(hits(h), NC.filter_matrices(sh, tt)) and int(h.offsets[-1]) == int(np.count_nonzero(sh))
    figures(h, "k_cmp_tile_nb", N_A, N_B, False)


@pytest.mark.parametrize("limit", LIMITS)
def test_upper(dev, limit):
    sh, tt = dev["b"].compare(dev["b"], limit).fetch()
    h = dev["b"].neighbors(None, limit, upper=True)
    assert NC.same(hits(h), NC.filter_matrices(sh, tt, upper=True))
    assert int(h.offsets[-1]) == int(np.count_nonzero(np.triu(sh, 1))) and all(int(t) > i for i in range(N_B) for t in h.target[int(h.offsets[i]):int(h.offsets[i + 1])])
    figures(h, "k_cmp_tile_nb", N_B, N_B, True)
    hw = dev["bc"].neighbors_counted(None, limit, upper=True)
    dt, ms = dev["bc"].compare_counted(dev["bc"], limit).fetch_weights()
    assert NC.same(hits(hw), NW.filter_weighted(sh, tt, dt, ms, upper=True))
    figures(hw, "k_cmp_tile_nb_w", N_B, N_B, True)


@pytest.mark.parametrize("limit", LIMITS)
def test_weighted_against_unweighted(dev, limit):
    A, CA, B, CB = operands()
    sh, tt = dev["a"].compare(dev["b"], limit).fetch()
    cw = dev["ac"].compare_counted(dev["bc"], limit)
    got = cw.fetch() + cw.fetch_weights()
    assert np.array_equal(got[0], sh) and np.array_equal(got[1], tt) and "k_cmp_tile_w," in cw.plan()["plan"]
    assert all(np.array_equal(g, w) for g, w in zip(got, WC.ref_compare(A, CA, B, CB, limit)))
    ones = dev["a"].compare_counted(dev["b"], limit)  # no counts at all: both count windows are filled with ones
    assert all(np.array_equal(x.astype(U64), sh.astype(U64)) for x in ones.fetch_weights()) and np.array_equal(ones.fetch()[0], sh) and np.array_equal(ones.fetch()[1], tt)
    half = dev["ac"].compare_counted(dev["b"], limit)  # one uncounted operand: min_sum is shared again, dot the sum of a's counts there
    assert np.array_equal(half.fetch()[0], sh) and np.array_equal(half.fetch()[1], tt) and np.array_equal(half.fetch_weights()[1], sh.astype(U64))
    if limit == LIMITS[-1]:
        assert all(np.array_equal(g, w) for g, w in zip(half.fetch() + half.fetch_weights(), WC.ref_compare(A, CA, B, None, limit)))


@pytest.mark.parametrize("limit", LIMITS)
def test_weighted_sparse_against_weighted_dense(dev, limit):
    for a, b in (("ac", "bc"), ("ac", "b"), ("a", "bc")):
        cw = dev[a].compare_counted(dev[b], limit)
        want = NW.filter_weighted(*(cw.fetch() + cw.fetch_weights()))
        hw = dev[a].neighbors_counted(dev[b], limit)
        assert hw.has_weights() and NC.same(hits(hw), want), (a, b)
        figures(hw, "k_cmp_tile_nb_w", N_A, N_B, False)
        assert NC.same(hits(dev[a].neighbors(dev[b], limit)), want[:4]), (a, b)  # the counts take no part in what is kept
