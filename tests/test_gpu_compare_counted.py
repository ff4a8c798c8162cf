"""GPU: the abundance-weighted all-pairs comparison (bsk_sets_compare_counted; compare.hip's k_cmp_tile_w) and bsk_sets_sumsq against the
Python-integer references of tests/compare_counted_cases.py -- every cell of all four matrices.  The plan's figures are asserted against
the restatement of the round rule in tests/compare_cases.py, and shared / total against Sets.compare on the same operands."""
import ctypes as C
import functools

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import compare_cases as CC
from tests import compare_counted_cases as WC
from tests.compare_cases import collection

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
CAPS = CC.read_caps()
R, COLS, W, PER_CU = CAPS["CMP_ROWS"], CAPS["CMP_COLS"], CAPS["CMP_WINDOW"], CAPS["CMP_W_BLOCKS_PER_CU"]


@functools.lru_cache(None)
def cus():
    hip = C.CDLL("libamdhip64.so")
    hip.hipDeviceGetAttribute.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
    v = C.c_int()
    assert hip.hipDeviceGetAttribute(C.byref(v), 63, 0) == 0 and v.value > 0  # hipDeviceAttributeMultiprocessorCount
    return v.value


def load(engine, sets, counts=None):
    offs, vals = collection(sets)
    return engine.sets_from_arrays(offs, vals) if counts is None else engine.sets_from_arrays_counted(offs, vals, WC.flat(counts))


def figures(cmp):
    p = cmp.plan()
    return p["tiles"], p["rounds"], p["max_rounds"]


def same(cmp, want, what):
    for name, got, w, dtype in (("total", cmp.total, want[1], U32), ("shared", cmp.shared, want[0], U32), ("dot", cmp.dot, want[2], U64), ("min_sum", cmp.min_sum, want[3], U64)):
        assert got.dtype == dtype and got.shape == np.asarray(w).shape, (what, name)
        assert np.array_equal(got, np.asarray(w, dtype)), (what, name, np.argwhere(got != np.asarray(w, dtype))[:5])


def check(engine, A, CA, B, CB, limit, what="", dA=None, dB=None, reuse=None, rounds=True, want=None, plain=True):
    """A x B with counts on the device: the plan's figures as the restatement counts them, every cell of the four matrices, and shared /
    total / figures equal to the unweighted compare's"""
    dA = dA if dA is not None else load(engine, A, CA)
    dB = dB if dB is not None else (dA if B is A and CB is CA else load(engine, B, CB))
    cmp = dA.compare_counted(dB, limit, reuse)
    assert cmp.weighted and cmp.info() == dict(n_a=len(A), n_b=len(B), limit=limit), what
    got = figures(cmp)
    assert got[0] == CC.n_tiles(len(A), len(B), CAPS), (what, got)
    if rounds:
        assert got == CC.plan_figures(A, B, limit, CAPS), (what, limit, got)
    text = cmp.plan()["plan"]
    assert "k_cmp_tile_w" in text and f"{R} x {COLS}" in text and f"windows of {W} values" in text and text.startswith("bsk_sets_compare_counted"), text
    same(cmp, want if want is not None else WC.ref_compare(A, CA, B, CB, limit), (what, limit))
    if plain:
        un = dA.compare(dB, limit)
        assert not un.weighted and np.array_equal(un.shared, cmp.shared) and np.array_equal(un.total, cmp.total) and figures(un) == got, (what, limit)
    return cmp


def test_hand_case(engine):
    A, CA, B, CB, plain, want = WC.hand_case()
    dA, dB = load(engine, A, CA), load(engine, B, CB)
    for limit in (0, 1, 2, 3, 100):
        dot, ms = want[limit]
        cmp = check(engine, A, CA, B, CB, limit, "hand", dA, dB, want=(plain[limit][0], plain[limit][1], dot, ms))
        assert figures(cmp) == (1, 1, 1)
    cmp = dA.compare_counted(dB)
    assert dA.sumsq().tolist() == [30, 0, 29] and dB.sumsq().tolist() == [89, 9] and dA.totals().tolist() == [10, 0, 7] and dB.totals().tolist() == [15, 3]
    assert cmp.cosine().tolist() == [[12 / (np.sqrt(30.0) * np.sqrt(89.0)), 12 / (np.sqrt(30.0) * 3.0)], [0.0, 0.0], [4 / (np.sqrt(29.0) * np.sqrt(89.0)), 0.0]]
    assert cmp.weighted_jaccard().tolist() == [[3 / 22, 3 / 10], [0.0, 0.0], [2 / 20, 0.0]]
    assert cmp.bray_curtis().tolist() == [[1 - 6 / 25, 1 - 6 / 13], [1.0, 1.0], [1 - 4 / 22, 1.0]]
    with pytest.raises(ValueError):
        dA.compare_counted(dB, limit=2).cosine()


def test_window_edges(engine):
    """counts follow their values through the rounds and through restaging"""
    A, B, claim = CC.window_edges(W)
    CA, CB = WC.attach(A, 1, 5, 41), WC.attach(B, 1, 5, 42)
    dA, dB = load(engine, A, CA), load(engine, B, CB)
    cmp = None
    for limit in claim["limits"]:
        cmp = check(engine, A, CA, B, CB, limit, "window edges", dA, dB, reuse=cmp)
    assert figures(check(engine, A, CA, B, CB, 0, "window edges", dA, dB, plain=False))[2] >= 3


def test_skew(engine):
    for name, (A, B) in CC.skew_cases(W).items():
        CA, CB = WC.attach(A, 1, 9, 43), WC.attach(B, 1, 9, 44)
        for limit in (0, W + 3):
            check(engine, A, CA, B, CB, limit, "skew " + name)
    A, B = CC.skew_cases(W)["low"]
    assert figures(check(engine, A, WC.attach(A, 1, 9, 43), B, WC.attach(B, 1, 9, 44), 0, "skew low", plain=False)) == (1, 5, 5)
    A, B = CC.skew_cases(W)["dense"]
    assert figures(check(engine, A, WC.attach(A, 1, 9, 43), B, WC.attach(B, 1, 9, 44), 0, "skew dense", plain=False)) == (1, 10, 10)


def test_tile_edges(engine):
    A, B, claim = CC.tile_edges(R, COLS)
    CA, CB = WC.attach(A, 1, 1000, 45), WC.attach(B, 1, 1000, 46)
    dA, dB = {}, {}
    full = WC.ref_compare(A, CA, B, CB, 0), WC.ref_compare(A, CA, B, CB, 7)
    cmp = None
    for na, nb in claim["shapes"]:
        if na not in dA:
            dA[na] = load(engine, A[:na], CA[:na])
        if nb not in dB:
            dB[nb] = load(engine, B[:nb], CB[:nb])
        for k, limit in enumerate((0, 7)):
            want = tuple(m[:na, :nb] for m in full[k])
            cmp = check(engine, A[:na], CA[:na], B[:nb], CB[:nb], limit, f"tile edges {na} x {nb}", dA[na], dB[nb], reuse=cmp, rounds=False, want=want, plain=(na, nb) in ((R + 1, COLS - 1), (2 * R + 1, 2 * COLS + 1)))
            tiles = -(-na // R) * -(-nb // COLS)
            assert figures(cmp) == (tiles, tiles, 1)


def test_where_the_limit_lands(engine):
    for a, ca, b, cb, limit, sh, tt, dot, ms in WC.limit_landings():
        cmp = check(engine, [a], [ca], [b], [cb], limit, "limit landing")
        assert (int(cmp.shared[0, 0]), int(cmp.total[0, 0]), int(cmp.dot[0, 0]), int(cmp.min_sum[0, 0])) == (sh, tt, dot, ms), (a, b, limit)


def test_saturation(engine):
    A, CA, B, CB, dot, ms = WC.saturation_cases()
    cmp = check(engine, A, CA, B, CB, 0, "saturation")
    M = WC.CMAX
    assert [[int(x) for x in r] for r in cmp.dot] == dot and [[int(x) for x in r] for r in cmp.min_sum] == ms
    assert int(cmp.dot[0, 0]) == M * M and int(cmp.dot[0, 1]) == WC.MAX and int(cmp.min_sum[0, 1]) == 2 * M and int(cmp.dot[0, 2]) == M * M + M
    # the norms saturate too, and the cosine says so: NaN in the saturated cells and in the rows and columns of a saturated norm
    dA, dB = load(engine, A, CA), load(engine, B, CB)
    assert dA.sumsq().tolist() == [WC.MAX, WC.MAX] and dB.sumsq().tolist() == [M * M, WC.MAX, M * M + 1, WC.MAX]
    assert np.isnan(dA.compare_counted(dB).cosine()).all()
    one = load(engine, [A[0][:1]], [CA[0][:1]])
    cos = one.compare_counted(dB).cosine()
    assert abs(cos[0, 0] - 1.0) <= 1e-15 and np.isnan(cos[0, 1]) and np.isnan(cos[0, 3]) and cos[0, 2] == float(M * M) / (np.sqrt(float(M * M)) * np.sqrt(float(M * M + 1)))


def test_operand_kinds(engine):
    A, B, _ = CC.tile_edges(R, COLS)
    CA, CB = WC.attach(A, 1, 7, 47), WC.attach(B, 1, 7, 48)
    check(engine, A, CA, B, None, 0, "counted x uncounted")
    check(engine, A, None, B, CB, 0, "uncounted x counted")
    check(engine, A, None, B, CB, 9, "uncounted x counted")
    cmp = check(engine, A, None, B, None, 0, "uncounted x uncounted")
    assert np.array_equal(cmp.dot, cmp.shared.astype(U64)) and np.array_equal(cmp.min_sum, cmp.shared.astype(U64)) and cmp.shared.any()
    check(engine, A[:1], CA[:1], B, CB, 0, "one against many")
    check(engine, A, CA, B[:1], CB[:1], 5, "many against one")
    dA = load(engine, A, CA)
    cmp = check(engine, A, CA, A, CA, 0, "a is b", dA, dA)
    assert np.array_equal(np.diag(cmp.dot), dA.sumsq()) and np.array_equal(np.diag(cmp.min_sum), dA.totals())
    assert np.array_equal(cmp.dot, cmp.dot.T) and np.array_equal(cmp.min_sum, cmp.min_sum.T)
    assert np.allclose(np.diag(cmp.cosine()), 1.0, rtol=0, atol=1e-15)  # x / (sqrt(x) * sqrt(x)): three roundings
    check(engine, A, CA, A, CA, 9, "a is b", dA, dA)
    # the float mirrors on real norms
    dB = load(engine, B, CB)
    cmp = dA.compare_counted(dB)
    qa, qb, ta, tb = WC.ref_sumsq(CA), WC.ref_sumsq(CB), WC.ref_totals(CA), WC.ref_totals(CB)
    assert np.array_equal(dA.sumsq(), qa) and np.array_equal(dB.totals(), tb)
    assert np.allclose(cmp.cosine(), WC.ref_cosine(cmp.dot, qa, qb), rtol=1e-15, atol=0)
    assert np.allclose(cmp.weighted_jaccard(), WC.ref_weighted_jaccard(cmp.min_sum, ta, tb), rtol=1e-15, atol=0)
    assert np.allclose(cmp.bray_curtis(), WC.ref_bray_curtis(cmp.min_sum, ta, tb), rtol=1e-15, atol=0)


def test_extreme_values(engine):
    S_, _, claim = CC.extreme_values(W)
    Cs = WC.attach(S_, 1, 1 << 20, 49)
    d = load(engine, S_, Cs)
    for limit in claim["limits"]:
        check(engine, S_, Cs, S_, Cs, limit, "extreme values", d, d)
    e = claim["edge_index"]
    # the set whose window boundary falls between 2^64-2 and 2^64-1 takes a second round: its last count comes with the second window
    cmp = check(engine, [S_[e]], [Cs[e]], [S_[e], S_[4]], [Cs[e], Cs[4]], 0, "window boundary at the top")
    assert figures(cmp)[2] == 2 and int(cmp.dot[0, 1]) == int(Cs[e][-1]) * int(Cs[4][0])


def test_more_tiles_than_one_pass_of_the_grid(engine):
    tiles_wanted = cus() * PER_CU + 3
    ty = int(np.ceil(np.sqrt(tiles_wanted)))
    tx = -(-tiles_wanted // ty)
    na, nb = ty * R - 3, tx * COLS - 5
    assert CC.n_tiles(na, nb, CAPS) >= tiles_wanted
    A, ma = CC.small_pool_sets(na, seed=31)
    B, mb = CC.small_pool_sets(nb, seed=32)
    va, CA = WC.pool_counts(ma, 1, 3, 51)
    vb, CB = WC.pool_counts(mb, 1, 3, 52)
    dA, dB = load(engine, A, CA), load(engine, B, CB)
    cmp = dA.compare_counted(dB, 0)
    assert figures(cmp) == (ty * tx, ty * tx, 1)
    same(cmp, WC.dense_compare(va, vb), "beyond one pass")
    assert cmp.dot.max() > cmp.shared.max()  # counts above 1 took part
    cmp = dA.compare_counted(dB, 2, reuse=cmp)
    assert figures(cmp) == (ty * tx, ty * tx, 1) and np.all(cmp.total == 2)
    rng = np.random.default_rng(33)
    cells = [(int(i), int(j)) for i, j in zip(rng.integers(0, na, 2000), rng.integers(0, nb, 2000))]
    for i0, j0 in ((0, 0), (0, nb - COLS), (na - R, 0), (na - R, nb - COLS)):  # the corner tiles
        cells += [(i0 + i, j0 + j) for i in range(R) for j in range(COLS)]
    for i, j in cells:
        assert (int(cmp.shared[i, j]), int(cmp.total[i, j]), int(cmp.dot[i, j]), int(cmp.min_sum[i, j])) == WC.ref_pair(A[i], CA[i], B[j], CB[j], 2), (i, j)


def test_object_rules(engine):
    lib = engine.lib
    A, B, _ = CC.tile_edges(R, COLS)
    CA, CB = WC.attach(A, 1, 7, 53), WC.attach(B, 1, 7, 54)
    dA, dB = load(engine, A[:4], CA[:4]), load(engine, B[:3], CB[:3])
    want = WC.ref_compare(A[:4], CA[:4], B[:3], CB[:3], 0)
    cmp = dA.compare_counted(dB, 0)
    same(cmp, want, "first")
    pd, pm = C.c_void_p(), C.c_void_p()
    assert lib.bsk_compare_weights_device(cmp.h, C.byref(pd), C.byref(pm)) == L.OK and pd.value and pm.value and pd.value != pm.value
    ps, pt = cmp.device()
    assert ps and pt and len({ps, pt, pd.value, pm.value}) == 4
    # weighted -> compare into the same object: unweighted, the weights refused, shared / total right
    un = dA.compare(dB, 0, reuse=cmp)
    assert un is cmp and cmp.weighted is False and "k_cmp_tile," in cmp.plan()["plan"]
    assert lib.bsk_compare_weights_device(cmp.h, C.byref(pd), C.byref(pm)) == L.OK and pd.value is None and pm.value is None
    dt, ms = np.full(12, 7, U64), np.full(12, 7, U64)
    assert lib.bsk_compare_fetch_weights(engine.ctx, cmp.h, 0, 4, dt.ctypes.data, ms.ctypes.data, 12) == L.ERR_ARG and list(dt) == [7] * 12
    with pytest.raises(Exception):
        cmp.fetch_weights()
    with pytest.raises(ValueError):
        cmp.dot
    assert np.array_equal(cmp.shared, want[0]) and np.array_equal(cmp.total, want[1])
    # ... and compare_counted again into it, larger and smaller
    for a, ca, b, cb in ((A, CA, B, CB), (A[:4], CA[:4], B[:3], CB[:3])):
        cmp = check(engine, a, ca, b, cb, 0, "reuse", reuse=cmp, rounds=False, plain=False)
    # fetch_weights: row ranges, either array, the cap
    for first, n in ((0, 4), (1, 2), (3, 1), (4, 0), (2, 0)):
        d, m = cmp.fetch_weights(first, n)
        assert d.dtype == U64 and np.array_equal(d, want[2][first:first + n]) and np.array_equal(m, want[3][first:first + n])
        s, t = cmp.fetch(first, n)  # bsk_compare_fetch on a weighted result
        assert np.array_equal(s, want[0][first:first + n]) and np.array_equal(t, want[1][first:first + n])
    assert lib.bsk_compare_fetch_weights(engine.ctx, cmp.h, 1, 2, None, ms.ctypes.data, 6) == L.OK and np.array_equal(ms[:6], want[3][1:3].ravel())
    assert lib.bsk_compare_fetch_weights(engine.ctx, cmp.h, 1, 2, dt.ctypes.data, None, 6) == L.OK and np.array_equal(dt[:6], want[2][1:3].ravel())
    assert lib.bsk_compare_fetch_weights(engine.ctx, cmp.h, 1, 2, dt.ctypes.data, ms.ctypes.data, 5) == L.ERR_ARG
    assert lib.bsk_compare_fetch_weights(engine.ctx, cmp.h, 3, 2, dt.ctypes.data, ms.ctypes.data, 12) == L.ERR_ARG
    assert lib.bsk_compare_fetch_weights(engine.ctx, cmp.h, 5, 0, dt.ctypes.data, ms.ctypes.data, 12) == L.ERR_ARG
    # a foreign context: BSK_ERR_ARG, *cmp kept
    other = S.Engine(0)
    foreign = load(other, B[:3], CB[:3])
    h = C.c_void_p(cmp.h.value)
    assert lib.bsk_sets_compare_counted(engine.ctx, dA.h, foreign.h, 0, C.byref(h)) == L.ERR_ARG and h.value == cmp.h.value
    assert lib.bsk_sets_compare_counted(other.ctx, foreign.h, foreign.h, 0, C.byref(h)) == L.ERR_ARG and h.value == cmp.h.value
    assert lib.bsk_compare_fetch_weights(other.ctx, cmp.h, 0, 4, dt.ctypes.data, ms.ctypes.data, 12) == L.ERR_ARG
    q = np.zeros(4, U64)
    assert lib.bsk_sets_sumsq(engine.ctx, foreign.h, 0, 1, q.ctypes.data) == L.ERR_ARG
    foreign.close()
    other.close()
    same(cmp, want, "after the refused calls")
    # too many cells: BSK_ERR_UNSUPPORTED before anything is allocated, the object released
    rows, cols = load(engine, [np.zeros(0, U64)] * 65536), load(engine, [np.zeros(0, U64)] * 32769)
    h = C.c_void_p(cmp.h.value)
    cmp.h = None  # (the library releases it)
    assert lib.bsk_sets_compare_counted(engine.ctx, rows.h, cols.h, 0, C.byref(h)) == L.ERR_UNSUPPORTED and h.value is None
    fresh = C.c_void_p()
    assert lib.bsk_sets_compare_counted(engine.ctx, rows.h, cols.h, 0, C.byref(fresh)) == L.ERR_UNSUPPORTED and fresh.value is None  # nothing was made
    with pytest.raises(Exception):
        rows.compare_counted(cols)


def test_empty_operands(engine):
    A, _, _ = CC.tile_edges(R, COLS)
    CA = WC.attach(A, 1, 7, 55)
    dA, none = load(engine, A[:5], CA[:5]), load(engine, [])
    for a, b, shape in ((none, dA, (0, 5)), (dA, none, (5, 0)), (none, none, (0, 0))):
        cmp = a.compare_counted(b, 3)
        assert cmp.weighted and cmp.info() == dict(n_a=shape[0], n_b=shape[1], limit=3) and figures(cmp) == (0, 0, 0)
        assert cmp.shared.shape == shape and cmp.dot.shape == shape and cmp.min_sum.shape == shape and cmp.dot.dtype == U64
        assert a.compare_counted(b).cosine().shape == shape
    empties = [np.zeros(0, U64)] * 3
    cmp = check(engine, empties, None, A[:2], CA[:2], 0, "empty sets")
    assert not cmp.dot.any() and not cmp.min_sum.any() and np.array_equal(cmp.total, [[len(A[0]), len(A[1])]] * 3)
    assert not cmp.cosine().any() and not cmp.weighted_jaccard().any()


# ---- bsk_sets_sumsq ----
def test_sumsq(engine):
    lib = engine.lib
    sets, sizes = CC.bottom_sets()
    counts = WC.attach(sets, 1, 100_000, 56)
    want = WC.ref_sumsq(counts)
    d = load(engine, sets, counts)  # 49 values a set on average: a wavefront a set
    got = d.sumsq()
    assert got.dtype == U64 and np.array_equal(got, want)
    small = load(engine, sets[:21], counts[:21])  # sizes 0 .. 20, 10 on average: eight lanes a set
    assert np.array_equal(small.sumsq(), want[:21])
    assert np.array_equal(load(engine, sets).sumsq(), np.array(sizes, U64))  # an uncounted object: the sizes
    # saturation: two values of count 2^32 - 1, on either path, beside sets that do not saturate
    M = WC.CMAX
    sat_sets = [CC.u64([1, 2]), CC.u64([3]), CC.u64([]), CC.u64([4, 5, 6])]
    sat_counts = [np.array([M, M], U32), np.array([M], U32), np.zeros(0, U32), np.array([M, 1, M], U32)]
    assert [int(x) for x in load(engine, sat_sets, sat_counts).sumsq()] == [WC.MAX, M * M, 0, WC.MAX]
    long_set = [np.arange(1, 201, dtype=U64)] + sat_sets
    long_counts = [np.full(200, M, U32)] + sat_counts
    assert [int(x) for x in load(engine, long_set, long_counts).sumsq()] == [WC.MAX, WC.MAX, M * M, 0, WC.MAX]
    # range rules: those of bsk_sets_totals
    n = len(sets)
    for first, count in ((0, n), (3, 5), (n - 1, 1), (n, 0), (7, 0)):
        q = np.full(count + 1, 99, U64)
        assert lib.bsk_sets_sumsq(engine.ctx, d.h, first, count, q.ctypes.data) == L.OK and q[count] == 99
        assert np.array_equal(q[:count], want[first:first + count])
    q = np.full(4, 99, U64)
    for first, count in ((n, 1), (n + 1, 0), (0, n + 1), (5, n)):
        assert lib.bsk_sets_sumsq(engine.ctx, d.h, first, count, q.ctypes.data) == L.ERR_ARG
    assert lib.bsk_sets_sumsq(engine.ctx, d.h, 0, 2, None) == L.ERR_ARG and list(q) == [99] * 4
    assert load(engine, []).sumsq().shape == (0,)


@pytest.mark.parametrize("size", [5, 40])
def test_sumsq_beyond_one_pass_of_its_grid(engine, size):
    """more sets than one pass of the capped grid (16 workgroups a CU), on the eight-lane path and on the wavefront path"""
    lanes = 8 if size <= 16 else 64
    n_sets = cus() * 16 * (256 // lanes) + 77
    rng = np.random.default_rng(size)
    sizes = rng.integers(size, 2 * size, n_sets) if lanes == 64 else rng.integers(0, size + 1, n_sets)
    offs = np.zeros(n_sets + 1, U64)
    offs[1:] = np.cumsum(sizes)
    N = int(offs[-1])
    assert (N <= 16 * n_sets) == (lanes == 8)
    vals = np.arange(N, dtype=U64) * U64(7919) + U64(11)
    counts = rng.integers(1, 1 << 16, N).astype(U32)
    got = engine.sets_from_arrays_counted(offs, vals, counts).sumsq()
    csum = np.concatenate([np.zeros(1, U64), np.cumsum(counts.astype(U64) ** U64(2), dtype=U64)])  # below 2^64: 2^32 per value, fewer than 2^32 values
    assert np.array_equal(got, (csum[offs[1:].astype(np.int64)] - csum[offs[:-1].astype(np.int64)]).astype(U64))


# ---- end to end through the Python mirror ----
def test_mutated_genomes_end_to_end(engine):
    seqs = WC.repeated_sequences()
    res = engine.run(engine.batch(seqs), engine.params(L.MINIMIZER, 21, w=11))
    sets = res.counted_sets()
    assert sets.counted
    offs, vals = sets.fetch()
    host, counts = CC.split(offs, vals), CC.split(offs, sets.fetch_counts())
    assert len(host) == 5 and all(len(s) > 2000 for s in host) and all(c.max() > 1 for c in counts)
    cmp = sets.compare_counted()
    want = WC.ref_compare(host, counts, host, counts, 0)
    same(cmp, want, "end to end")
    qa, ta = WC.ref_sumsq(counts), WC.ref_totals(counts)
    assert np.array_equal(sets.sumsq(), qa) and np.array_equal(sets.totals(), ta)
    ref = WC.ref_cosine(want[2], qa, qa)
    cos = cmp.cosine()
    assert np.all(np.abs(cos - ref) <= 1e-12 * np.abs(ref))
    ang = cmp.angular_similarity()
    assert np.all(np.abs(ang - WC.ref_angular(ref)) <= 1e-7)  # (acos is steep at 1: the diagonal's last bit is 1e-8 of an angle)
    assert ang[0, 1] >= 1.0 - 1e-7 and ang[0, 1] > ang[0, 2] > ang[0, 3] > ang[0, 4] >= 0.0  # falls with the mutation rate, lowest against the unrelated one
    assert np.array_equal(cmp.dot, cmp.dot.T) and np.array_equal(np.diag(cmp.dot), qa) and np.array_equal(np.diag(cmp.min_sum), ta)
    wj = cmp.weighted_jaccard()
    assert wj[0, 1] == 1.0 and wj[0, 1] > wj[0, 2] > wj[0, 3] > wj[0, 4] and np.allclose(cmp.bray_curtis(), 1.0 - 2.0 * wj / (1.0 + wj), rtol=1e-12, atol=1e-15)
