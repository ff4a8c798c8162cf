"""GPU: the weighted sparse all-pairs comparison (bsk_sets_neighbors_counted; compare.hip's k_cmp_tile_nb_w) -- all six arrays of every
result compared for exact equality with the model of tests/neighbor_counted_cases.py (ref_compare filtered by filter_matrices), the first
four also with Sets.neighbors and the weights with the cells of Sets.compare_counted on the same operands; the tiles run and skipped as
the plan reports them; the second run, the stride loop, the re-use chain, the empties and determinism."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import compare_cases as CC
from tests import compare_counted_cases as WC
from tests import neighbor_cases as NC
from tests import neighbor_counted_cases as NW
from tests.compare_cases import collection

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
CAPS = CC.read_caps()
R, COLS, W = CAPS["CMP_ROWS"], CAPS["CMP_COLS"], CAPS["CMP_WINDOW"]
NONE = 0xFFFFFFFF  # a min_shared above every cell


def load(engine, sets, counts=None):
    offs, vals = collection(sets)
    return engine.sets_from_arrays(offs, vals) if counts is None else engine.sets_from_arrays_counted(offs, vals, WC.flat(counts))


def arrays(h):
    return h.offsets, h.target, h.shared, h.total, h.dot, h.min_sum


def blob(xs):
    return b"".join(np.ascontiguousarray(x).tobytes() for x in xs)


def pointers(engine, h):
    """the device addresses of all six arrays"""
    pt, pd, pm = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert engine.lib.bsk_hits_totals_device(h.h, C.byref(pt)) == L.OK and engine.lib.bsk_hits_weights_device(h.h, C.byref(pd), C.byref(pm)) == L.OK
    return h.device() + (pt.value, pd.value, pm.value)


def grid_stats(engine):
    out = (C.c_uint64 * 2)()
    assert engine.lib.bsk_ctx_grid_stats(engine.ctx, out) == L.OK
    return int(out[0]), int(out[1])


def figures(h):
    return NC.plan_figures(h.plan()["plan"])


@contextlib.contextmanager
def switch(engine, name, value):
    before = os.environ.get(name)
    os.environ[name] = value
    try:
        engine.reload_options()
        yield
    finally:
        if before is None:
            del os.environ[name]
        else:
            os.environ[name] = before
        engine.reload_options()


def call(engine, dA, dB, n_a, n_b, limit, want, what, reuse=None, **p):
    """one call: types, sizes, all six arrays against `want`, the plan's kernel and tiles"""
    h = dA.neighbors_counted(dB, limit, reuse=reuse, **p)
    got = arrays(h)
    assert h.has_totals() and h.has_weights(), what
    assert [x.dtype for x in got] == [U64, U32, U32, U32, U64, U64], what
    assert h.info() == dict(n_queries=n_a, n_hits=len(got[1])) and len(got[0]) == n_a + 1 and all(len(x) == len(got[1]) for x in got[2:]), what
    differ = [k for k, (g, w) in enumerate(zip(got, want)) if not np.array_equal(np.asarray(g).astype(U64), np.asarray(w).astype(U64))]
    assert NC.same(got, want), (what, limit, p, "arrays that differ", differ)
    plan = h.plan()
    fig = figures(h)
    assert plan["plan"].startswith("bsk_sets_neighbors_counted: k_cmp_tile_nb_w,") and plan["n_large_queries"] == 0, plan
    assert (fig["tiles"], fig["skipped"]) == NC.expected_tiles(n_a, n_b, p.get("upper", False), CAPS), (what, plan)
    assert fig["rounds"] >= fig["tiles"] and fig["runs"] in (1, 2), plan
    return h


class Device:
    """a case of neighbor_counted_cases on the device"""

    def __init__(self, engine, name):
        self.engine, self.name, self.case = engine, name, NW.cases()[name]
        self.A, self.CA, self.B, self.CB = NW.operands(self.case)
        self.dA = load(engine, self.A, self.CA)
        self.dB = self.dA if self.case.B is None else load(engine, self.B, self.CB)

    def check(self, limit, reuse=None, **p):
        return call(self.engine, self.dA, self.dB, len(self.A), len(self.B), limit, NW.expected(self.case, limit, p), self.name, reuse=reuse, **p)

    def runs(self):
        h = None
        for limit, p in self.case.runs:
            h = self.check(limit, reuse=h, **p)
        return h


# ---- 1 .. 3: the written-out cases ----
def test_hand_case(engine):
    A, CA, B, CB, plain, want = WC.hand_case()
    dA, dB = load(engine, A, CA), load(engine, B, CB)
    h = None
    for limit in (0, 1, 2, 3, 100):
        sh, tt = (np.array(x, U32) for x in plain[limit])
        dot, ms = (np.array(x, U64) for x in want[limit])
        h = call(engine, dA, dB, 3, 2, limit, NW.filter_weighted(sh, tt, dot, ms), "hand", reuse=h)
    assert [x.tolist() for x in arrays(h)] == [[0, 2, 2, 3], [0, 1, 0], [2, 1, 1], [5, 4, 4], [12, 12, 4], [3, 3, 2]]
    h = dA.neighbors_counted(dB, reuse=h)
    assert h.cosine().tolist() == [12 / (np.sqrt(30.0) * np.sqrt(89.0)), 12 / (np.sqrt(30.0) * 3.0), 4 / (np.sqrt(29.0) * np.sqrt(89.0))]
    assert h.weighted_jaccard().tolist() == [3 / 22, 3 / 10, 2 / 20] and h.bray_curtis().tolist() == [1 - 6 / 25, 1 - 6 / 13, 1 - 4 / 22]
    cmp = dA.compare_counted(dB)
    i, j = h.query().astype(int), h.target.astype(int)
    assert np.array_equal(h.angular_similarity(), cmp.angular_similarity()[i, j]) and np.array_equal(h.cosine(), cmp.cosine()[i, j])
    with pytest.raises(ValueError):
        dA.neighbors_counted(dB, limit=2).cosine()
    with pytest.raises(ValueError):
        dA.neighbors(dB).cosine()
    assert h.fetch_weights(2, 1)[0].tolist() == [4] and h.fetch_weights(0, 1)[1].tolist() == [3, 3] and len(h.fetch_weights(1, 1)[0]) == 0


def test_saturation(engine):
    A, CA, B, CB, dot, ms = WC.saturation_cases()
    sh, tt = CC.ref_compare(A, B, 0)
    h = call(engine, load(engine, A, CA), load(engine, B, CB), 2, 4, 0, NW.filter_weighted(sh, tt, np.array(dot, U64), np.array(ms, U64)), "saturation")
    assert h.info()["n_hits"] == 8 and h.dot.tolist() == dot[0] + dot[1] and h.min_sum.tolist() == ms[0] + ms[1]
    assert int(h.dot[7]) == WC.MAX and int(h.min_sum[7]) == 2 * WC.CMAX + 3  # saturated on the second value, a third walked: kept, and min_sum exact
    assert np.isnan(h.cosine()).all() and not np.isnan(h.weighted_jaccard()).any()  # both sets of A have a saturated norm


def test_limit_landings(engine):
    h = None
    for a, ca, b, cb, limit, shared, total, dot, ms in WC.limit_landings():
        want = ([0, 1], [0], [shared], [total], [dot], [ms]) if shared else ([0, 0], [], [], [], [], [])
        h = call(engine, load(engine, [a], [ca]), load(engine, [b], [cb]), 1, 1, limit, want, "limit landings", reuse=h)


# ---- 4 .. 7, 13: the cases of neighbor_counted_cases ----
@pytest.mark.parametrize("name", ["window_edges", "skew_dense", "skew_dense_t", "skew_gap", "skew_low"])
def test_windows(engine, name):
    """sizes around the window; one set many windows ahead of its partner: a value staged again brings its count again"""
    Device(engine, name).runs()


@pytest.mark.parametrize("n", [15, 16, 17, 33])
def test_tiles_with_and_without_upper(engine, n):
    dev = Device(engine, "tiles_%d" % n)
    full = dev.check(0)
    up = dev.check(0, upper=True)  # (tiles= and skipped= against neighbor_cases.expected_tiles: in call())
    T = -(-n // R)
    assert figures(up)["skipped"] == T * (T - 1) // 2
    assert (up.target.astype(np.int64) > up.query().astype(np.int64)).all() and len(full.target) == 2 * len(up.target) + n


@pytest.mark.parametrize("name", ["kinds_cc", "kinds_cu", "kinds_uc", "kinds_uu"])
def test_operand_kinds(engine, name):
    dev = Device(engine, name)
    assert dev.dA.counted == (dev.CA is not None) and dev.dB.counted == (dev.CB is not None)
    h = dev.runs()
    if name == "kinds_uu":
        assert len(h.shared) and np.array_equal(h.dot, h.shared.astype(U64)) and np.array_equal(h.min_sum, h.shared.astype(U64))


def test_rules_against_neighbors_and_compare_counted(engine):
    dev = Device(engine, "rules_40")
    cmp = dev.dA.compare_counted(dev.dB)
    dot, ms = cmp.dot.copy(), cmp.min_sum.copy()
    h = plain = None
    for limit, p in dev.case.runs:
        h = dev.check(limit, reuse=h, **p)
        plain = dev.dA.neighbors(dev.dB, limit, reuse=plain, **p)
        assert not plain.has_weights() and plain.dot is None and plain.min_sum is None
        assert blob(arrays(h)[:4]) == blob((plain.offsets, plain.target, plain.shared, plain.total)), p  # bit-identical
        i, j = h.query().astype(int), h.target.astype(int)
        assert np.array_equal(h.dot, dot[i, j]) and np.array_equal(h.min_sum, ms[i, j]), p


def test_small_pool_70_by_50(engine):
    dev = Device(engine, "pool_70x50")
    full = WC.dense_compare(*dev.case.dense)
    h = call(engine, dev.dA, dev.dB, 70, 50, 0, NW.filter_weighted(*full), "70 x 50")
    i, j = h.query().astype(int), h.target.astype(int)
    ta, tb, qa, qb = WC.ref_totals(dev.CA), WC.ref_totals(dev.CB), WC.ref_sumsq(dev.CA), WC.ref_sumsq(dev.CB)
    assert h.weighted_jaccard() == pytest.approx(WC.ref_weighted_jaccard(full[3], ta, tb)[i, j], rel=1e-15)
    assert h.bray_curtis() == pytest.approx(WC.ref_bray_curtis(full[3], ta, tb)[i, j], rel=1e-15)
    assert h.cosine() == pytest.approx(WC.ref_cosine(full[2], qa, qb)[i, j], rel=1e-15)


# ---- 8, 9: the room and the stride loop ----
def test_the_second_run(engine):
    dev = Device(engine, "rules_40")
    plain = dev.check(0)
    want = blob(arrays(plain))
    assert plain.info()["n_hits"] > 8 and figures(plain)["runs"] == 1
    with switch(engine, "BSK_NB_ROOM", "8"):
        small = dev.check(0)
        assert figures(small)["runs"] == 2 and blob(arrays(small)) == want
        again = dev.check(0, reuse=small)  # the object holds the room now
        assert figures(again)["runs"] == 1 and blob(arrays(again)) == want
        # the room of a re-used object is the smallest of its FIVE arrays: hits of the unweighted call hold three of the size, no weights
        three = dev.dA.neighbors(dev.dB)
        assert figures(three)["runs"] == 2
        five = dev.check(0, reuse=three)
        assert figures(five)["runs"] == 2 and blob(arrays(five)) == want
    assert figures(dev.check(0))["runs"] == 1


def test_the_stride_loop_under_a_grid_cap(engine):
    dev = Device(engine, "rules_40")
    want = blob(arrays(dev.check(0)))
    with switch(engine, "BSK_GRID_CAP", "2"):
        s0, c0 = grid_stats(engine)
        capped = dev.check(0)  # nine tiles on two workgroups, five and four each: cursors, s_wk and s_base re-used from tile to tile
        s1, c1 = grid_stats(engine)
        assert s1 > s0 and c1 > c0, "the cap cut no grid"
        assert blob(arrays(capped)) == want and figures(capped)["tiles"] == 9
        up = figures(dev.check(0, upper=True))  # ... and a workgroup that skips tiles between those it runs
        assert (up["tiles"], up["skipped"]) == (6, 3)


# ---- 10: one object through a chain of entries ----
def test_the_reuse_chain(engine):
    lib, ctx = engine.lib, engine.ctx
    dev, small = Device(engine, "rules_40"), Device(engine, "tiles_15")
    h = dev.check(0)
    first = pointers(engine, h)
    assert all(first)
    ix = dev.dB.index()
    s = ix.search(dev.dA, reuse=h)  # a search into it: neither totals nor weights
    assert s is h and not h.has_weights() and not h.has_totals() and h.dot is None and h.min_sum is None and h.total is None
    pd, pm = C.c_void_p(1), C.c_void_p(1)
    assert lib.bsk_hits_weights_device(h.h, C.byref(pd), C.byref(pm)) == L.OK and pd.value is None and pm.value is None
    buf = np.zeros(4096, U64)
    assert lib.bsk_hits_fetch_weights(ctx, h.h, 0, 40, buf.ctypes.data, buf.ctypes.data, buf.size) == L.ERR_ARG and not buf.any()
    assert b"no weights" in lib.bsk_last_error(ctx)
    with pytest.raises(ValueError):
        h.cosine()
    h = small.check(0, reuse=h)  # smaller operands: nothing grows, nothing moves
    assert pointers(engine, h) == first
    top = h.top(2)
    assert not top.has_weights() and not top.has_totals() and top.dot is None and top.total is None
    assert NC.same((top.offsets, top.target, top.shared), NC.top_rows(h.offsets, h.target, h.shared, 2))
    weighted = small.check(0)
    assert h.top(2, reuse=weighted) is weighted and not weighted.has_weights() and not weighted.has_totals()  # top() INTO weighted hits
    plain = small.dA.neighbors(small.dB, reuse=h)
    assert plain is h and h.has_totals() and not h.has_weights() and h.dot is None
    assert NC.same((h.offsets, h.target, h.shared, h.total), NW.expected(small.case, 0, {})[:4])
    # fetch_weights: the range and cap rules of bsk_hits_fetch_totals
    g = small.check(0, reuse=h)
    n = g.info()["n_hits"]
    assert np.array_equal(g.fetch_weights(3, 5)[0], g.dot[int(g.offsets[3]):int(g.offsets[8])])
    assert lib.bsk_hits_fetch_weights(ctx, g.h, 0, 16, buf.ctypes.data, None, buf.size) == L.ERR_ARG
    assert lib.bsk_hits_fetch_weights(ctx, g.h, 15, 1, buf.ctypes.data, None, buf.size) == L.ERR_ARG
    assert lib.bsk_hits_fetch_weights(ctx, g.h, 0, 15, buf.ctypes.data, None, n - 1) == L.ERR_ARG and not buf.any()
    assert lib.bsk_hits_fetch_weights(ctx, g.h, 15, 0, None, None, 0) == L.OK
    assert lib.bsk_hits_fetch_weights(ctx, g.h, 0, 15, None, buf.ctypes.data, n) == L.OK and np.array_equal(buf[:n], g.min_sum)
    # the slot: a refused call leaves it; hits of another context stay where they are
    keep = C.c_void_p(g.h.value)
    for bad in (L.NeighborParams(1, 2, 0, 0), L.NeighborParams(1, 0, 3, 2)):
        assert lib.bsk_sets_neighbors_counted(ctx, small.dA.h, small.dB.h, 0, C.byref(bad), C.byref(keep)) == L.ERR_ARG and keep.value == g.h.value
        assert lib.bsk_last_error(ctx).startswith(b"bsk_sets_neighbors_counted:")
    other = S.Engine(0)
    try:
        theirs = load(other, small.A[:3], small.CA[:3])  # (weighted hits keep their operands: both go before their engine does)
        foreign = theirs.neighbors_counted()
        slot = C.c_void_p(foreign.h.value)
        assert lib.bsk_sets_neighbors_counted(ctx, small.dA.h, small.dB.h, 0, None, C.byref(slot)) == L.ERR_ARG and slot.value == foreign.h.value
        assert b"another context" in lib.bsk_last_error(ctx)
        assert lib.bsk_hits_fetch_weights(ctx, foreign.h, 0, 0, None, None, 0) == L.ERR_ARG
        assert foreign.info()["n_queries"] == 3 and foreign.has_weights()
        foreign.close()
        theirs.close()
    finally:
        other.close()
    assert g.cluster().info()["n_items"] == 15  # bsk_hits_cluster reads weighted hits as any others


# ---- 11, 12 ----
def test_empties(engine):
    dev = Device(engine, "tiles_15")
    none = load(engine, [], [])
    hollow = load(engine, [np.zeros(0, U64)] * 5, [np.zeros(0, U32)] * 5)
    h = None
    for a, b, rows in ((none, dev.dA, 0), (dev.dA, none, 15), (none, none, 0), (hollow, hollow, 5), (hollow, dev.dA, 5), (dev.dA, dev.dA, 15), (dev.dA, none, 15)):
        p = dict(min_shared=NONE) if a is dev.dA and b is dev.dA else {}  # a threshold nothing passes
        h = a.neighbors_counted(b, 3, reuse=h, **p)
        assert h.info() == dict(n_queries=rows, n_hits=0) and h.has_totals() and h.has_weights()
        assert h.offsets.tolist() == [0] * (rows + 1) and all(x is not None and len(x) == 0 for x in arrays(h)[1:])
        assert h.plan()["plan"].startswith("bsk_sets_neighbors_counted:")


def test_two_calls_are_byte_identical(engine):
    dev = Device(engine, "window_edges")
    first = blob(arrays(dev.dA.neighbors_counted(dev.dB, 2 * W + 1, min_jaccard=(1, 8))))
    assert blob(arrays(dev.dA.neighbors_counted(dev.dB, 2 * W + 1, min_jaccard=(1, 8)))) == first and len(first) > 8 * 9
