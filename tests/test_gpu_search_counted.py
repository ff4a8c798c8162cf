"""GPU: the weighted containment search (bsk_index_build_counted, bsk_index_search_counted; search.hip's k_ix_gather, k_sw_row, k_sw_chunk,
k_sw_finish) -- all five arrays of every result compared for exact equality with the model of tests/search_counted_cases.py, the first
three also with bsk_index_search on the same operands, the weights with bsk_sets_neighbors_counted; the plan's path figures against
paths(); the crafted posting sums, list lengths, the two new caps straddled, saturation on both paths, the four combinations of counted
and uncounted operands, the empties, a counted index under the unweighted entries, attached handles and norms, re-use, the grid cap and
determinism."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import search_cases as SC
from tests import search_counted_cases as W

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
SEARCH_PLAN = "k_sr_lookup + k_sr_small (LDS sort, <= %d target ids per query); large path: " % SC.SR_CAP


def load(engine, coll, counts=None):
    return engine.sets_from_arrays(*coll) if counts is None else engine.sets_from_arrays_counted(coll[0], coll[1], counts)


def arrays(h):
    return h.offsets, h.target, h.shared, h.dot, h.min_sum


def blob(xs):
    return b"".join(np.ascontiguousarray(x).tobytes() for x in xs)


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))


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


class Device:
    """a case on the device: targets indexed with and without counts, queries loaded with and without counts"""

    def __init__(self, engine, tg, t_cnt, qs, q_cnt, claims):
        self.engine, self.tg, self.t_cnt, self.qs, self.q_cnt, self.claims = engine, tg, t_cnt, qs, q_cnt, claims
        self.dT, self.dTu = load(engine, tg, t_cnt), load(engine, tg)
        self.dQ, self.dQu = load(engine, qs, q_cnt), load(engine, qs)
        self.ix, self.plain = self.dT.index_counted(), self.dTu.index()
        assert self.ix.counted and not self.plain.counted

    def check(self, thr=(1, 0.0, 0.0), tc=True, qc=True, reuse=None, want=None):
        """one call: types, sizes, all five arrays against the model, the first three against bsk_index_search, the plan"""
        ix, dQ = (self.ix if tc else self.plain), (self.dQ if qc else self.dQu)
        if want is None:
            want = W.ref_search_counted(self.tg, self.t_cnt if tc else None, self.qs, self.q_cnt if qc else None, *thr)
        h = ix.search_counted(dQ, *thr, reuse=reuse)
        got = arrays(h)
        nq = len(self.qs[0]) - 1
        assert h.has_weights() and not h.has_totals() and not h.has_members(), thr
        assert [x.dtype for x in got] == [U64, U32, U32, U64, U64]
        assert h.info() == dict(n_queries=nq, n_hits=len(got[1])) and len(got[0]) == nq + 1 and all(len(x) == len(got[1]) for x in got[2:])
        differ = [k for k, (g, w) in enumerate(zip(got, want)) if not np.array_equal(g, w)]
        assert same(got, want), (thr, tc, qc, "arrays that differ", differ)
        un = ix.search(dQ, *thr)
        assert blob(got[:3]) == blob((un.offsets, un.target, un.shared)) and not un.has_weights()  # bit for bit the unweighted search's rows
        plan, uplan = h.plan(), un.plan()
        assert plan["plan"] == uplan["plan"] + W.plan_tail(self.claims["sums"], self.qs[0], got[0]), plan
        assert plan["plan"].startswith(SEARCH_PLAN) and plan["n_large_queries"] == uplan["n_large_queries"] == self.claims["n_large"], plan
        un.close()
        return h


@functools.lru_cache(maxsize=None)
def crafted(name):
    """a crafted case with seeded counts -> (tg, t_cnt, qs, q_cnt, claims); built once"""
    kind = "mixed"
    if name == "posting edges":
        tg, qs, cl = SC.posting_edge_case()
    elif name == "list lengths":
        tg, qs, cl = SC.list_length_case()
    elif name == "boundary":
        tg, qs, cl = SC.boundary_case(6, 6)
    elif name.startswith("row edges"):
        tg, qs, cl, _ = W.row_edge_case()
        kind = "max" if name.endswith("max") else "mixed"
    elif name.startswith("chunk edges"):
        tg, qs, cl, _ = W.chunk_edge_case()
        kind = "max" if name.endswith("max") else "mixed"
    else:
        raise KeyError(name)
    t_cnt, q_cnt = W.with_counts(tg, qs, 1000 + len(name), kind)
    return tg, t_cnt, qs, q_cnt, cl


# ---- the crafted cases of the search, with counts ----
def test_posting_sum_edges(engine):
    """posting sums 1, 63, 64, 65, 2047, 2048, 2049 and 5 000, made several ways: both sides of SR_CAP, both kernels of the payload pass"""
    tg, t_cnt, qs, q_cnt, cl = crafted("posting edges")
    assert set(SC.SUM_EDGES) <= set(cl["sums"].tolist()) and 0 < cl["n_large"] < len(cl["sums"])
    d = Device(engine, tg, t_cnt, qs, q_cnt, cl)
    h = d.check()
    in_row, chunks = W.paths(cl["sums"], qs[0], h.offsets)
    assert in_row.sum() >= 20 and chunks.sum() >= 100  # both paths ran: small-path queries of more than SW_ROW hits take the chunks too
    assert (h.dot == U64(W.MAX)).any() and (h.min_sum > U64(1 << 32)).any()  # counts of 2^32 - 1 on both sides: saturated dots, a min_sum above 2^32
    d.check((2, 0.0, 0.0), reuse=h)


def test_list_lengths(engine):
    """posting lists of 63, 64, 65, 128 and 129 targets at value index 0, 63, 64, 100 and 129 of large queries: the whole-wavefront walk"""
    tg, t_cnt, qs, q_cnt, cl = crafted("list lengths")
    d = Device(engine, tg, t_cnt, qs, q_cnt, cl)
    h = d.check()
    assert W.paths(cl["sums"], qs[0], h.offsets)[1].sum() >= 25
    d.check((2, 0.0, 0.0), reuse=h)  # most pairs share one value: their postings are met and must not be added anywhere


def test_boundary_of_the_small_path(engine):
    tg, t_cnt, qs, q_cnt, cl = crafted("boundary")
    assert cl["n_large"] == 6 and (cl["sums"] <= SC.SR_CAP).sum() == 6 and cl["sums"].min() >= 2036
    d = Device(engine, tg, t_cnt, qs, q_cnt, cl)
    h = d.check()
    in_row, chunks = W.paths(cl["sums"], qs[0], h.offsets)
    assert chunks.sum() == 12 and in_row.sum() == 0  # small-path queries of some 2 040 hits: beyond the LDS row, one chunk each
    h2 = d.check((2, 0.0, 0.0), reuse=h)  # rows of a few hits: the small-path queries move to k_sw_row
    assert W.paths(cl["sums"], qs[0], h2.offsets)[0].sum() > 0


# ---- the payload pass's own caps ----
@pytest.mark.parametrize("kind", ["mixed", "max"])
def test_lds_row_straddled(engine, kind):
    """rows of SW_ROW - 1, SW_ROW and SW_ROW + 1 hits on the small path: the last one takes the atomics"""
    tg, t_cnt, qs, q_cnt, cl = crafted("row edges " + kind)
    d = Device(engine, tg, t_cnt, qs, q_cnt, cl)
    h = d.check()
    assert np.diff(h.offsets).tolist() == [W.SW_ROW - 1, W.SW_ROW, W.SW_ROW + 1, 200]
    assert h.plan()["plan"].endswith("k_sw_row 3 queries (<= %d hits), k_sw_chunk %d chunks of %d values" % (W.SW_ROW, -(-(W.SW_ROW + 3) // W.SW_CHUNK), W.SW_CHUNK))
    if kind == "max":  # every count 2^32 - 1: two shared values wrap, one does not
        assert np.array_equal(h.dot == U64(W.MAX), h.shared >= 2) and np.array_equal(h.min_sum, h.shared.astype(U64) * U64(W.M32))
    h2 = d.check((2, 0.0, 0.0), reuse=h)  # fewer hits per row: all three in LDS now, the fourth query without a hit
    assert h2.plan()["plan"].endswith("k_sw_row 3 queries (<= %d hits), k_sw_chunk 0 chunks of %d values" % (W.SW_ROW, W.SW_CHUNK))


@pytest.mark.parametrize("kind", ["mixed", "max"])
def test_chunk_straddled(engine, kind):
    """large queries of SW_CHUNK - 1, SW_CHUNK, SW_CHUNK + 1, 2 SW_CHUNK and 2 SW_CHUNK + 1 values: 1, 1, 2, 2 and 3 chunks"""
    tg, t_cnt, qs, q_cnt, cl = crafted("chunk edges " + kind)
    d = Device(engine, tg, t_cnt, qs, q_cnt, cl)
    h = d.check()
    assert "k_sw_chunk 9 chunks" in h.plan()["plan"]
    d.check((2, 0.0, 0.0), reuse=h)     # drops most pairs of the large queries
    d.check((1, 0.02, 0.0), reuse=h)
    d.check((1, 0.0, 0.5), reuse=h)


@pytest.mark.parametrize("large", [False, True])
def test_saturation_is_exact(engine, large):
    """dot exactly 2^64 - 1 without a wrap, one below, beyond by one, beyond by a whole wrap; a min_sum above 2^32 -- in LDS and with atomics"""
    tg, t_cnt, qs, q_cnt, cl, want = W.saturation_case(large)
    d = Device(engine, tg, t_cnt, qs, q_cnt, cl)
    h = d.check()
    assert [int(x) for x in h.dot[:5]] == want["dot"] and [int(x) for x in h.min_sum[:5]] == want["min_sum"]
    assert ("k_sw_chunk 1 chunks" if large else "k_sw_row 1 queries") in h.plan()["plan"]
    h = d.check((3, 0.0, 0.0), reuse=h)
    assert h.target.tolist() == [2, 4] and [int(x) for x in h.dot] == [W.MAX, W.MAX]


# ---- counted and uncounted operands ----
@pytest.mark.parametrize("name", ["chunk edges mixed", "row edges mixed"])
def test_four_combinations(engine, name):
    tg, t_cnt, qs, q_cnt, cl = crafted(name)
    d = Device(engine, tg, t_cnt, qs, q_cnt, cl)
    h = None
    for tc in (True, False):
        for qc in (True, False):
            h = d.check((1, 0.0, 0.0), tc, qc, reuse=h)
            if not tc and not qc:
                assert np.array_equal(h.dot, h.shared.astype(U64)) and np.array_equal(h.min_sum, h.shared.astype(U64))
            if not tc and qc:  # against an index without counts: the share of the query's mass found
                wc = h.weighted_containment()
                tot = d.dQ.totals()[h.query().astype(np.int64)].astype(np.float64)
                ok = h.dot != U64(W.MAX)
                assert np.array_equal(wc[ok], h.dot[ok].astype(np.float64) / tot[ok]) and (wc[ok] <= 1.0).all() and np.isnan(wc[~ok]).all()
            if tc:
                with pytest.raises(ValueError):
                    h.weighted_containment()
    # an index built by the new entry from uncounted sets is an index without counts
    u = d.dTu.index_counted()
    assert not u.counted and u.info() == d.plain.info()
    assert same(arrays(u.search_counted(d.dQ)), arrays(d.plain.search_counted(d.dQ)))


def test_empties(engine):
    """empty queries among the others, queries without a hit, no queries at all, an index of empty targets and an index of no targets"""
    tg = SC.collection([[1, 2, 3], [], [3, 4]])
    qs = SC.collection([[], [3], [9, 10], [], [1, 2, 3, 4], []])
    t_cnt, q_cnt = np.array([5, 6, 7, 8, 9], U32), np.array([2, 3, 4, 1, W.M32, 1, 2], U32)
    d = Device(engine, tg, t_cnt, qs, q_cnt, SC.claims(SC.posting_sums(*tg, *qs)))
    h = d.check()
    assert h.offsets.tolist() == [0, 0, 2, 2, 2, 4, 4] and h.dot.tolist() == [14, 16, 1 * 5 + W.M32 * 6 + 7, 8 + 2 * 9] and h.min_sum.tolist() == [2, 2, 1 + 6 + 1, 1 + 2]
    none = d.check((4, 0.0, 0.0), reuse=h)  # no hits: has_weights all the same
    assert none.info()["n_hits"] == 0 and none.has_weights() and len(none.dot) == 0
    assert "k_sw_row 0 queries" in none.plan()["plan"] and "k_sw_chunk 0 chunks" in none.plan()["plan"]
    no_q = SC.collection([])
    d0 = Device(engine, tg, t_cnt, no_q, np.zeros(0, U32), SC.claims(np.zeros(0, np.int64)))
    assert d0.check().info() == dict(n_queries=0, n_hits=0)
    for empty_tg in (SC.collection([[], [], []]), SC.collection([])):
        de = Device(engine, empty_tg, np.zeros(0, U32), qs, q_cnt, SC.claims(np.zeros(6, np.int64)))
        he = de.check()
        assert he.info() == dict(n_queries=6, n_hits=0) and he.has_weights()
        sq, tt = de.ix.norms()
        assert sq.tolist() == tt.tolist() == [0] * (len(empty_tg[0]) - 1)


# ---- a counted index under the entries that existed ----
def test_counted_index_equals_plain_index(engine):
    tg, t_cnt, qs, q_cnt, cl = crafted("list lengths")
    d = Device(engine, tg, t_cnt, qs, q_cnt, cl)
    a, b = d.ix.info(), d.plain.info()
    T, P = len(tg[0]) - 1, len(tg[1])
    assert a["device_bytes"] == b["device_bytes"] + P * 4 + 2 * T * 8 and {k: v for k, v in a.items() if k != "device_bytes"} == {k: v for k, v in b.items() if k != "device_bytes"}
    by_old_entry = d.dT.index()  # bsk_index_build of counted sets: an index without counts
    assert not by_old_entry.counted and by_old_entry.info() == b
    for thr in ((1, 0.0, 0.0), (3, 0.0, 0.0), (1, 0.05, 0.0)):
        x, y = d.ix.search(d.dQ, *thr), d.plain.search(d.dQ, *thr)
        assert blob((x.offsets, x.target, x.shared)) == blob((y.offsets, y.target, y.shared)) and x.plan() == y.plan() and not x.has_weights()
        t = x.top(3)
        assert not t.has_weights() and same((t.offsets, t.target, t.shared), SC.ref_top(y.offsets, y.target, y.shared, 3))


def test_norms_and_attached_handle(engine):
    tg, t_cnt, qs, q_cnt, cl = crafted("row edges mixed")
    d = Device(engine, tg, t_cnt, qs, q_cnt, cl)
    sq, tt = d.ix.norms()
    assert sq.dtype == tt.dtype == U64 and np.array_equal(sq, d.dT.sumsq()) and np.array_equal(tt, d.dT.totals()) and (sq == U64(W.MAX)).any()
    psq, ptt = d.plain.norms()
    assert np.array_equal(psq, np.diff(tg[0])) and np.array_equal(ptt, np.diff(tg[0]))  # an index without counts: |t| for both
    part = np.zeros(7, U64)
    assert engine.lib.bsk_index_fetch_norms(engine.ctx, d.ix.h, 3, 7, None, part.ctypes.data) == L.OK and np.array_equal(part, tt[3:10])
    assert engine.lib.bsk_index_fetch_norms(engine.ctx, d.ix.h, 3, 7, part.ctypes.data, None) == L.OK and np.array_equal(part, sq[3:10])
    assert engine.lib.bsk_index_fetch_norms(engine.ctx, d.ix.h, len(tt) - 2, 3, part.ctypes.data, None) == L.ERR_ARG  # a range outside the targets
    other = S.Engine(0)
    assert engine.lib.bsk_index_fetch_norms(other.ctx, d.ix.h, 0, 1, part.ctypes.data, None) == L.ERR_ARG  # a foreign context
    handle = d.ix.attach(other)
    assert handle.counted and handle.info() == d.ix.info() and handle.norms() is d.ix.norms()
    fresh = S.Index(other, handle.h, handle.target_sizes)  # the same handle without the inherited norms: fetched through it
    assert np.array_equal(fresh.norms()[0], sq) and np.array_equal(fresh.norms()[1], tt)
    fresh.h = None
    q2 = load(other, qs, q_cnt)
    want = arrays(d.ix.search_counted(d.dQ, 2))
    assert same(arrays(handle.search_counted(q2, 2)), want)
    d.ix.close()  # the first handle goes: the arrays stay with the attached one
    assert same(arrays(handle.search_counted(q2, 2)), want)
    for x in (q2, handle, other):
        x.close()


# ---- two independent kernels, one answer ----
@pytest.mark.parametrize("m", [1, 2, 5])
def test_against_neighbors_counted(engine, m):
    """bsk_sets_neighbors_counted(queries, targets, limit 0, min_shared m) walks every cell with compare.hip's tile kernel; the search
    with the covers at 0 must list the same rows with the same weights"""
    rng = np.random.default_rng(5 + m)
    pool = rng.integers(0, 2**64, 900, dtype=U64)
    tg = SC.collection([pool[rng.choice(900, int(rng.integers(0, 120)), replace=False)] for _ in range(150)])
    qs = SC.collection([pool[rng.choice(900, int(rng.integers(0, 300)), replace=False)] for _ in range(70)] + [pool])  # the last query: every value, the large path
    t_cnt, q_cnt = W.with_counts(tg, qs, 77, "mixed")
    cl = SC.claims(SC.posting_sums(*tg, *qs))
    assert cl["n_large"] >= 1
    d = Device(engine, tg, t_cnt, qs, q_cnt, cl)
    h = d.ix.search_counted(d.dQ, m)
    nb = d.dQ.neighbors_counted(d.dT, 0, min_shared=m)
    assert same(arrays(h), arrays(nb)) and len(h.target) > 0
    for name in ("cosine", "angular_similarity", "weighted_jaccard", "bray_curtis"):  # bound norms against the operands' own
        assert np.array_equal(getattr(h, name)(), getattr(nb, name)(), equal_nan=True), name
    d.check((m, 0.0, 0.0), reuse=h)


# ---- re-use ----
def test_reuse_and_refusals(engine):
    tg, t_cnt, qs, q_cnt, cl = crafted("chunk edges mixed")
    d = Device(engine, tg, t_cnt, qs, q_cnt, cl)
    lib = engine.lib
    h = d.dQ.neighbors(d.dQ, 0, min_shared=3)  # an object that holds totals
    assert h.has_totals() and not h.has_weights()
    h = d.check(reuse=h)
    assert not h.has_totals() and h.has_weights()
    first = blob(arrays(h))
    plain = d.ix.search(d.dQ)
    folded = plain.fold(np.arange(0, len(tg[0]), 2, dtype=U64))  # (an even number of targets: groups of two)
    assert folded.has_members()
    folded = d.check(reuse=folded)  # ... and one that held members
    assert not folded.has_members() and blob(arrays(folded)) == first
    # an unweighted search into the weighted object leaves it without weights; the arrays stay
    pd, pm = C.c_void_p(), C.c_void_p()
    assert lib.bsk_hits_weights_device(h.h, C.byref(pd), C.byref(pm)) == L.OK and pd.value and pm.value
    h = d.ix.search(d.dQ, 2, reuse=h)
    assert not h.has_weights() and h.dot is None
    buf = np.zeros(4, U64)
    assert lib.bsk_hits_fetch_weights(engine.ctx, h.h, 0, 1, buf.ctypes.data, buf.ctypes.data, 4) == L.ERR_ARG
    h = d.check(reuse=h)
    pd2, pm2 = C.c_void_p(), C.c_void_p()
    assert lib.bsk_hits_weights_device(h.h, C.byref(pd2), C.byref(pm2)) == L.OK and (pd2.value, pm2.value) == (pd.value, pm.value) and blob(arrays(h)) == first
    for t in (h.top(2), h.fold(np.array([0, len(tg[0]) - 1], U64))):  # what top() and fold() make of weighted hits carries no weights
        assert not t.has_weights()
    # the refusals: the slot is kept, the object intact
    slot = C.c_void_p(h.h.value)
    other = S.Engine(0)
    foreign_q, foreign_h = load(other, qs), d.plain.attach(other)
    bad = [(engine.ctx, d.ix.h, d.dQ.h, L.SearchParams(1, 1, 0.0, 0.0)), (engine.ctx, d.ix.h, d.dQ.h, L.SearchParams(1, 0, 1.5, 0.0)),
           (engine.ctx, d.ix.h, d.dQ.h, L.SearchParams(1, 0, 0.0, float("nan"))), (engine.ctx, d.ix.h, foreign_q.h, L.SearchParams(1, 0, 0.0, 0.0)),
           (engine.ctx, foreign_h.h, d.dQ.h, L.SearchParams(1, 0, 0.0, 0.0)), (engine.ctx, None, d.dQ.h, L.SearchParams(1, 0, 0.0, 0.0))]
    for ctx, ix, q, sp in bad:
        assert lib.bsk_index_search_counted(ctx, ix, q, C.byref(sp), C.byref(slot)) == L.ERR_ARG and slot.value == h.h.value, (sp.reserved, sp.min_query_cov)
    assert b"bsk_index_search_counted: null argument" in lib.bsk_last_error(engine.ctx)
    foreign_hits = foreign_h.search(foreign_q)
    fslot = C.c_void_p(foreign_hits.h.value)
    sp = L.SearchParams(1, 0, 0.0, 0.0)
    keep = fslot.value
    assert lib.bsk_index_search_counted(engine.ctx, d.ix.h, d.dQ.h, C.byref(sp), C.byref(fslot)) == L.ERR_ARG and fslot.value == keep  # hits of another context
    assert h.has_weights() and blob(h.fetch() + h.fetch_weights()) == first  # kept means intact
    out = C.c_void_p(99)
    assert lib.bsk_index_build_counted(engine.ctx, foreign_q.h, C.byref(out)) == L.ERR_ARG and out.value is None  # the build only writes its slot
    assert b"bsk_index_build_counted: the sets belong to another context" in lib.bsk_last_error(engine.ctx)


# ---- the grid cap, determinism ----
@pytest.mark.parametrize("cap", ["1", "3"])
def test_grid_cap(engine, cap):
    """BSK_GRID_CAP = 1 and 3: one and three workgroups walk every query and every chunk in their stride loops (and build the index)"""
    for name in ("row edges mixed", "chunk edges max", "boundary"):
        tg, t_cnt, qs, q_cnt, cl = crafted(name)
        free = Device(engine, tg, t_cnt, qs, q_cnt, cl)
        want = [arrays(free.ix.search_counted(free.dQ, m)) for m in (1, 2)]
        with switch(engine, "BSK_GRID_CAP", cap):
            d = Device(engine, tg, t_cnt, qs, q_cnt, cl)
            assert d.ix.info() == free.ix.info() and np.array_equal(d.ix.norms()[0], free.ix.norms()[0]) and np.array_equal(d.ix.norms()[1], free.ix.norms()[1])
            for m, w in zip((1, 2), want):
                assert same(arrays(d.ix.search_counted(d.dQ, m)), w), (name, m)     # the capped index, the capped pass
                assert same(arrays(free.ix.search_counted(d.dQ, m)), w), (name, m)  # the free index, the capped pass
        assert same(arrays(d.ix.search_counted(free.dQ, 1)), want[0]), name        # the capped index, the free pass


def test_two_calls_bit_for_bit(engine):
    for name in ("chunk edges max", "posting edges"):
        tg, t_cnt, qs, q_cnt, cl = crafted(name)
        d = Device(engine, tg, t_cnt, qs, q_cnt, cl)
        a = d.ix.search_counted(d.dQ)
        first = blob(arrays(a))
        b = d.ix.search_counted(d.dQ)
        assert blob(arrays(b)) == first
        a = d.ix.search_counted(d.dQ, reuse=a)  # ... and into the object that held them
        assert blob(arrays(a)) == first
        d2 = Device(engine, tg, t_cnt, qs, q_cnt, cl)  # a second build of the same sets: the same index, the same answer
        assert blob(arrays(d2.ix.search_counted(d2.dQ))) == first
