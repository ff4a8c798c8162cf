"""GPU: the sparse all-pairs comparison (bsk_sets_neighbors; compare.hip's k_cmp_tile_nb) -- every result compared for exact equality
with the model of tests/neighbor_cases.py AND with bsk_sets_compare of the same operands filtered on the host; the tiles run and skipped
as the plan reports them; the second run, determinism, the result slot, and a collection of more than 2^31 cells."""
import contextlib
import ctypes as C
import math
import os
import time

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import compare_cases as CC
from tests import neighbor_cases as NC
from tests.compare_cases import collection

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
CAPS = CC.read_caps()
R, COLS, W = CAPS["CMP_ROWS"], CAPS["CMP_COLS"], CAPS["CMP_WINDOW"]
NONE = 0xFFFFFFFF  # a min_shared above every cell


def load(engine, sets):
    return engine.sets_from_arrays(*collection(sets))


def arrays(h):
    return h.offsets, h.target, h.shared, h.total


def rule(p):
    """test parameters -> keyword arguments of the model"""
    mj = p.get("min_jaccard") or (0, 0)
    num, den = mj if isinstance(mj, tuple) else (int(math.ceil(mj * (1 << 30))), 1 << 30)  # a float: the mirror's fraction over 2^30
    return dict(min_shared=p.get("min_shared", 1), num=num, den=den, upper=p.get("upper", False))


class Case:
    """a pair of collections on the device and, per limit, the dense reference (computed once) and the dense compare of the library"""

    def __init__(self, engine, A, B=None):
        self.engine, self.A, self.B = engine, A, A if B is None else B
        self.dA = load(engine, A)
        self.dB = self.dA if B is None else load(engine, B)
        self._ref, self._dense = {}, {}

    def ref(self, limit):
        if limit not in self._ref:
            self._ref[limit] = CC.ref_compare(self.A, self.B, limit)
        return self._ref[limit]

    def dense(self, limit):
        if limit not in self._dense:
            cmp = self.dA.compare(self.dB, limit)
            self._dense[limit] = (cmp.shared.copy(), cmp.total.copy())
            cmp.close()
        return self._dense[limit]

    def check(self, limit, what="", reuse=None, **p):
        h = self.dA.neighbors(self.dB, limit, reuse=reuse, **p)
        got = arrays(h)
        assert got[0].dtype == U64 and got[1].dtype == U32 and got[2].dtype == U32 and got[3].dtype == U32, what
        assert h.info() == dict(n_queries=len(self.A), n_hits=len(got[1])) and len(got[0]) == len(self.A) + 1, what
        model = NC.filter_matrices(*self.ref(limit), **rule(p))
        assert NC.same(got, model), (what, limit, p, "model")
        assert NC.same(got, NC.filter_matrices(*self.dense(limit), **rule(p))), (what, limit, p, "bsk_sets_compare, filtered")
        plan = h.plan()
        fig = NC.plan_figures(plan["plan"])
        assert "k_cmp_tile_nb" in plan["plan"] and plan["n_large_queries"] == 0, plan
        assert (fig["tiles"], fig["skipped"]) == NC.expected_tiles(len(self.A), len(self.B), p.get("upper", False), CAPS), (what, plan)
        assert fig["rounds"] >= fig["tiles"] and fig["runs"] in (1, 2), plan
        return h

    def sweep(self, limits, what):
        """every parameter set of the contract at every limit, into one re-used object"""
        h = None
        for limit in limits:
            sh, tt = self.ref(limit)
            h = self.check(limit, what, reuse=h)
            h = self.check(limit, what, reuse=h, min_shared=0)
            h = self.check(limit, what, reuse=h, min_shared=NONE)
            assert h.info()["n_hits"] == 0 and not h.offsets.any()
            h = self.check(limit, what, reuse=h, min_jaccard=(1, 1))  # shared == total: on whole sets, identical sets only
            assert limit or all(np.array_equal(self.A[i], self.B[int(j)]) for i, j in zip(h.query().astype(int), h.target))
            h = self.check(limit, what, reuse=h, upper=True)
            # a Jaccard fraction equal to one pair's shared / total exactly: kept; a step above: dropped
            sharing = np.argwhere((sh > 0) & (sh < tt))
            if len(sharing):
                i, j = (int(v) for v in sharing[len(sharing) // 2])
                s, t = int(sh[i, j]), int(tt[i, j])
                h = self.check(limit, what, reuse=h, min_jaccard=(s, t))
                assert j in h.target[int(h.offsets[i]):int(h.offsets[i + 1])]
                h = self.check(limit, what, reuse=h, min_jaccard=(s + 1, t))
                assert j not in h.target[int(h.offsets[i]):int(h.offsets[i + 1])]
        return h


def test_hand_case(engine):
    A, B, want = CC.hand_case()
    case = Case(engine, A, B)
    for limit, (sh, tt) in want.items():
        case._ref[limit] = (np.array(sh, U32), np.array(tt, U32))
    h = case.sweep(list(want), "hand")
    h = case.check(0, "hand", reuse=h)
    assert [x.tolist() for x in arrays(h)] == [[0, 2, 2, 3], [0, 1, 0], [2, 1, 1], [5, 4, 4]]
    assert h.jaccard().tolist() == [2 / 5, 1 / 4, 1 / 4] and h.has_totals()
    assert np.array_equal(h.mash_distance(21), case.dA.compare(case.dB).mash_distance(21)[[0, 0, 2], [0, 1, 0]])
    assert NC.same(arrays(case.check(0, "hand, float", min_jaccard=0.25)), arrays(case.check(0, "hand", min_jaccard=(1 << 28, 1 << 30))))
    assert case.check(0, "hand, float", min_jaccard=0.25).info()["n_hits"] == 3 and case.check(0, "hand, float", min_jaccard=0.2500001).info()["n_hits"] == 1


def test_window_edges(engine):
    A, B, claim = CC.window_edges(W)
    Case(engine, A, B).sweep([0, W + 1, 8 * W + 1], "window edges")  # all, a limit inside the second window, one beyond every union


def test_tile_edges(engine):
    A, B, claim = CC.tile_edges(R, COLS)
    full = {limit: CC.ref_compare(A, B, limit) for limit in (0, 7)}
    for na, nb in claim["shapes"]:
        case = Case(engine, A[:na], B[:nb])
        for limit in (0, 7):
            case._ref[limit] = (full[limit][0][:na, :nb], full[limit][1][:na, :nb])
        h = case.check(0, f"tile edges {na} x {nb}")
        h = case.check(7, f"tile edges {na} x {nb}", reuse=h, min_shared=3)
        h = case.check(0, f"tile edges {na} x {nb}", reuse=h, upper=True, min_jaccard=(1, 5))
        case.check(7, f"tile edges {na} x {nb}", reuse=h, upper=True)
    Case(engine, A, B).sweep([0, 7], "tile edges, whole")


def test_extreme_values(engine):
    sets, _, claim = CC.extreme_values(W)
    Case(engine, sets).sweep([0, 1, 2, W + 1], "extreme values")


@pytest.mark.parametrize("name", ["low", "gap", "dense", "dense_t"])
def test_skew(engine, name):
    A, B = CC.skew_cases(W)[name]
    Case(engine, A, B).sweep([0, 2 * W + 3], "skew " + name)


def test_limit_landings(engine):
    for a, b, limit, shared, total in CC.limit_landings():
        case = Case(engine, [a], [b])
        h = case.check(limit, "limit landings")
        assert [x.tolist() for x in arrays(h)] == ([[0, 1], [0], [shared], [total]] if shared else [[0, 0], [], [], []])
        if shared:
            h = case.check(limit, "limit landings", reuse=h, min_jaccard=(shared, total), min_shared=shared)
            assert h.info()["n_hits"] == 1
            assert case.check(limit, "limit landings", reuse=h, min_shared=shared + 1).info()["n_hits"] == 0


def test_mash_shape(engine):
    sets, claim = CC.mash_shape()
    case = Case(engine, sets)
    h = case.sweep([claim["limit"]], "mash shape")
    h = case.check(claim["limit"], "mash shape", reuse=h)
    assert len(h.total) and (h.total == claim["limit"]).all()  # full-size bottom-n sketches: total == limit


def test_small_pool_against_bit_masks(engine):
    sets, masks = CC.small_pool_sets(33)
    case = Case(engine, sets)
    case._ref[0] = CC.mask_compare(masks, masks)
    case.sweep([0], "small pool")


def test_empty_operands(engine):
    A, _, _ = CC.tile_edges(R, COLS)
    dA, none = load(engine, A[:5]), load(engine, [])
    h = None
    for a, b, rows in ((none, dA, 0), (dA, none, 5), (none, none, 0), (dA, dA, 5), (dA, none, 5)):
        h = a.neighbors(b, 3, reuse=h)
        assert h.info()["n_queries"] == rows and h.has_totals()
        if a is none or b is none:
            assert h.info()["n_hits"] == 0 and h.offsets.tolist() == [0] * (rows + 1) and len(h.total) == 0
        else:
            assert NC.same(arrays(h), NC.ref_neighbors(A[:5], A[:5], 3))


# ---- the triangle ----
@pytest.mark.parametrize("n", [16, 17, 33])
def test_upper_of_a_collection_against_itself(engine, n):
    sets, masks = CC.small_pool_sets(n, seed=21)
    case = Case(engine, sets)
    case._ref[0] = CC.mask_compare(masks, masks)
    full, up = case.check(0, "self"), case.check(0, "self, upper", upper=True)
    T = -(-n // R)
    assert NC.plan_figures(up.plan()["plan"])["skipped"] == T * (T - 1) // 2 and NC.plan_figures(up.plan()["plan"])["tiles"] == T * (T + 1) // 2
    cells = lambda h: {(int(i), int(j)): (int(s), int(t)) for i, j, s, t in zip(h.query(), h.target, h.shared, h.total)}
    f, u = cells(full), cells(up)
    assert all(j > i for i, j in u)  # no j <= i: the diagonal is absent
    assert {**u, **{(j, i): v for (i, j), v in u.items()}} == {k: v for k, v in f.items() if k[0] != k[1]}


def test_upper_of_two_collections_of_different_sizes(engine):
    A, B, _ = CC.tile_edges(R, COLS)
    for na, nb in ((33, 17), (17, 33)):
        case = Case(engine, A[:na], B[:nb])
        h = case.check(0, f"upper {na} x {nb}", upper=True)
        assert len(h.target) and (h.target.astype(np.int64) > h.query().astype(np.int64)).all()
        case.check(5, f"upper {na} x {nb}", reuse=h, upper=True, min_shared=2)


# ---- the room ----
@contextlib.contextmanager
def switch(engine, name, value):
    os.environ[name] = value
    try:
        engine.reload_options()
        yield
    finally:
        del os.environ[name]
        engine.reload_options()


def test_the_second_run(engine):
    A, B, _ = CC.tile_edges(R, COLS)
    case = Case(engine, A, B[:17])  # 33 x 17: six tiles
    plain = case.check(0, "room")
    assert plain.info()["n_hits"] > 8 and NC.plan_figures(plain.plan()["plan"])["runs"] == 1
    with switch(engine, "BSK_NB_ROOM", "8"):
        small = case.check(0, "room of 8")
        assert NC.plan_figures(small.plan()["plan"])["runs"] == 2
        assert NC.same(arrays(small), arrays(plain))
        again = case.check(0, "room of 8, re-used", reuse=small)  # the object holds the room now
        assert NC.plan_figures(again.plan()["plan"])["runs"] == 1 and NC.same(arrays(again), arrays(plain))
        up = case.check(0, "room of 8, upper", upper=True)
        assert NC.plan_figures(up.plan()["plan"])["runs"] == (2 if up.info()["n_hits"] > 8 else 1)
    assert NC.plan_figures(case.check(0, "room").plan()["plan"])["runs"] == 1


def test_ten_calls_are_byte_identical(engine):
    sets, claim = CC.mash_shape()
    dA = load(engine, sets)
    first = None
    for _ in range(10):
        h = dA.neighbors(None, claim["limit"], min_jaccard=(1, 4))
        got = b"".join(np.ascontiguousarray(x).tobytes() for x in arrays(h))
        h.close()
        first = first or got
        assert got == first
    assert len(first) > 8 * 41


# ---- the slot ----
def test_the_slot(engine):
    A, B, _ = CC.tile_edges(R, COLS)
    case = Case(engine, A[:17], B[:17])
    lib, ctx = engine.lib, engine.ctx
    ix = case.dB.index()
    hits = ix.search(case.dA)
    searched = tuple(x.copy() for x in (hits.offsets, hits.target, hits.shared))
    assert not hits.has_totals() and hits.total is None
    h = case.check(0, "into the hits of a search", reuse=hits)  # hits of a search, then neighbours: totals present
    assert h is hits and h.has_totals() and len(h.total) == h.info()["n_hits"]
    top = h.top(3)  # the n best of a neighbours result: the model's order, no totals
    assert NC.same((top.offsets, top.target, top.shared), NC.top_rows(h.offsets, h.target, h.shared, 3)) and not top.has_totals() and top.total is None
    again = ix.search(case.dA, reuse=h)  # ... then a search into it again: no totals
    assert NC.same((again.offsets, again.target, again.shared), searched)
    pt = C.c_void_p(1)
    assert lib.bsk_hits_totals_device(again.h, C.byref(pt)) == L.OK and pt.value is None
    buf = np.zeros(1024, U32)
    assert lib.bsk_hits_fetch_totals(ctx, again.h, 0, 17, buf.ctypes.data, buf.size) == L.ERR_ARG and not buf.any()
    # top() into hits with totals leaves them without
    h2 = case.check(0, "fresh")
    assert h2.top(2, reuse=case.check(0, "to be re-used")).has_totals() is False
    # fetch_totals: range and cap rules of bsk_hits_fetch
    n = h2.info()["n_hits"]
    assert np.array_equal(h2.fetch_totals(3, 5), h2.total[int(h2.offsets[3]):int(h2.offsets[8])])
    assert lib.bsk_hits_fetch_totals(ctx, h2.h, 0, 18, buf.ctypes.data, buf.size) == L.ERR_ARG
    assert lib.bsk_hits_fetch_totals(ctx, h2.h, 17, 1, buf.ctypes.data, buf.size) == L.ERR_ARG
    assert lib.bsk_hits_fetch_totals(ctx, h2.h, 0, 17, buf.ctypes.data, n - 1) == L.ERR_ARG and not buf.any()
    assert lib.bsk_hits_fetch_totals(ctx, h2.h, 17, 0, buf.ctypes.data, 0) == L.OK
    # hits of another context: BSK_ERR_ARG, and they stay in the slot
    other = S.Engine(0)
    try:
        foreign = load(other, A[:3]).neighbors()
        slot = C.c_void_p(foreign.h.value)
        assert lib.bsk_sets_neighbors(ctx, case.dA.h, case.dB.h, 0, None, C.byref(slot)) == L.ERR_ARG and slot.value == foreign.h.value
        assert b"another context" in lib.bsk_last_error(ctx)
        assert lib.bsk_hits_fetch_totals(ctx, foreign.h, 0, 0, buf.ctypes.data, 0) == L.ERR_ARG
        assert foreign.info()["n_queries"] == 3  # intact
        bad = L.NeighborParams(1, 2, 0, 0)
        keep = C.c_void_p(h2.h.value)
        assert lib.bsk_sets_neighbors(ctx, case.dA.h, case.dB.h, 0, C.byref(bad), C.byref(keep)) == L.ERR_ARG and keep.value == h2.h.value
        bad = L.NeighborParams(1, 0, 3, 2)
        assert lib.bsk_sets_neighbors(ctx, case.dA.h, case.dB.h, 0, C.byref(bad), C.byref(keep)) == L.ERR_ARG and keep.value == h2.h.value
        foreign.close()
    finally:
        other.close()
    assert NC.same(arrays(case.check(0, "after the refusals", reuse=h2)), NC.filter_matrices(*case.ref(0)))


# ---- beyond 2^31 cells ----
def test_more_cells_than_the_dense_compare_takes(engine):
    """46 400 sets, set i = {i // 2}, against themselves: 2 152 960 000 cells (measured on an MI355X: 0.31 s, and 0.15 s for the upper triangle)."""
    n = 46400
    s = engine.sets_from_arrays(*NC.pairs_case(n))
    cmp = C.c_void_p()
    assert engine.lib.bsk_sets_compare(engine.ctx, s.h, s.h, 0, C.byref(cmp)) == L.ERR_UNSUPPORTED and cmp.value is None  # the gap
    t0 = time.perf_counter()
    h = s.neighbors()
    t1 = time.perf_counter()
    print(f"bsk_sets_neighbors, {n} x {n} sets of one value: {t1 - t0:.3f} s")
    i = np.arange(n, dtype=np.int64)
    assert h.info() == dict(n_queries=n, n_hits=2 * n) and np.array_equal(h.offsets, 2 * np.arange(n + 1, dtype=U64))
    assert np.array_equal(h.target.reshape(n, 2), np.stack([i - i % 2, i - i % 2 + 1], 1))
    assert (h.shared == 1).all() and (h.total == 1).all()
    fig = NC.plan_figures(h.plan()["plan"])
    assert fig["tiles"] + fig["skipped"] == 2900 * 2900 and fig["skipped"] == 0 and fig["runs"] == 1
    t0 = time.perf_counter()
    up = s.neighbors(upper=True, reuse=h)
    t1 = time.perf_counter()
    print(f"bsk_sets_neighbors, upper, {n} x {n} sets of one value: {t1 - t0:.3f} s")
    assert up.info() == dict(n_queries=n, n_hits=n // 2)
    assert np.array_equal(np.diff(up.offsets.astype(np.int64)), (i % 2 == 0).astype(np.int64))  # (2m, 2m + 1) for every m
    assert np.array_equal(up.target, np.arange(1, n, 2, dtype=U32)) and (up.shared == 1).all() and (up.total == 1).all()
    fig = NC.plan_figures(up.plan()["plan"])
    assert fig["tiles"] + fig["skipped"] == 2900 * 2900 and fig["skipped"] == 2900 * 2899 // 2
