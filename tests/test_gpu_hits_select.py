"""GPU: bsk_hits_filter and bsk_hits_top_by against the integer model of tests/select_cases.py -- every measure, every row length at
which a path changes, every payload combination an entry can produce, the wide arithmetic, the result slot, the chains and the grid caps."""
import ctypes as C
import re
from fractions import Fraction

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import select_cases as SC
from tests.test_gpu_grid_caps import GRID_CAPS, grid_stats, switches

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
TOP64 = SC.TOP64
TB_PLAN = re.compile(r"bsk_hits_top_by n = (\d+) (\w+): k_tb_group (\d+) queries \(<= 16 hits\); k_tb_lds (\d+) queries \(<= 1024 hits\); k_tb_global (\d+) queries, (\d+) indices")
FL_PLAN = re.compile(r"bsk_hits_filter (\w+): k_sel_check \+ k_sel_place \+ k_sel_offsets, hits=(\d+) kept=(\d+)")


def rec_of(h):
    """everything the hits hold on the device, through the fetches"""
    o, t, s = h.fetch()
    dot, ms = h.fetch_weights() if h.has_weights() else (None, None)
    return SC.record(o, t, s, h.fetch_totals() if h.has_totals() else None, dot, ms, h.fetch_members() if h.has_members() else None)


def upload(engine, rec):
    return engine.hits_from_arrays(rec["o"], rec["t"], rec["s"], rec["total"])


def counted(engine, sets):
    return engine.sets_from_arrays_counted(*sets)


class Zoo:
    """one object per payload combination an entry can produce, each with every row length of SC.ROW_LENGTHS, its record and its norms:
    norms[kind] = (per query, per target) for kind in sizes / sumsq / totals, given to the calls explicitly where explicit is True"""

    def __init__(self, engine):
        self.engine, self.items = engine, {}
        plain, tot = SC.shape_record(with_total=False), SC.shape_record()
        sizes = SC.shape_sizes(plain)
        self.add("none", upload(engine, plain), dict(sizes=sizes), True)
        self.add("totals", upload(engine, tot), dict(sizes=sizes), True)
        q, t = SC.weighted_sets()
        self.a, self.b = counted(engine, q), counted(engine, t)
        self.ix = self.b.index_counted()
        plain_ix = self.b.index()
        norms = dict(sizes=(np.diff(q[0]), np.diff(t[0])), sumsq=(self.a.sumsq(), self.b.sumsq()), totals=(self.a.totals(), self.b.totals()))
        self.add("totals+weights", self.a.neighbors_counted(self.b), norms, False)
        self.add("weights", self.ix.search_counted(self.a), norms, False)
        self.add("weights, plain index", plain_ix.search_counted(self.a), dict(norms, sumsq=(norms["sumsq"][0], norms["sizes"][1]), totals=(norms["totals"][0], norms["sizes"][1])),
                 False)
        go = np.arange(0, 4201, 2, dtype=U64)  # pairs of targets: members 1 or 2
        self.add("members", self.items["none"][0].fold(go), dict(sizes=(sizes[0] + U64(40), np.full(len(go) - 1, 40, U64))), True)

    def add(self, name, h, norms, explicit):
        self.items[name] = (h, rec_of(h), norms, explicit)

    def norms_for(self, name, measure):
        """(qnorm, tnorm) of the model, and the keywords of the call"""
        h, rec, norms, explicit = self.items[name]
        kind = dict(query_cov="sizes", target_cov="sizes", jaccard="sizes", cosine="sumsq").get(measure, "totals")
        qn, tn = norms.get(kind, (None, None))
        return qn, tn, (dict(qnorm=qn, tnorm=tn) if explicit and SC.needs(measure, rec)[1] else {})

    def measures(self, name):
        h, rec, norms, _ = self.items[name]
        out = [m for m in SC.MEASURES if SC.applies(m, rec) and (m != "weighted_containment" or name == "weights, plain index")]
        return out


@pytest.fixture(scope="module")
def zoo(engine):
    return Zoo(engine)


NAMES = ("none", "totals", "totals+weights", "weights", "weights, plain index", "members")


def test_the_zoo_covers_the_payload_combinations_and_the_row_lengths(zoo):
    combos = set()
    for name in NAMES:
        h, rec, _, _ = zoo.items[name]
        combos.add(tuple(p for p in SC.PAYLOADS if rec[p] is not None))
        if name != "members":
            assert set(SC.ROW_LENGTHS) <= set(np.diff(rec["o"]).astype(int).tolist()), name
    assert combos == {(), ("total",), ("total", "dot", "msum"), ("dot", "msum"), ("members",)}
    assert set(sum((zoo.measures(n) for n in NAMES), [])) == set(SC.MEASURES)


@pytest.mark.parametrize("name", NAMES)
def test_top_by_every_measure_every_n(zoo, name):
    h, rec, _, _ = zoo.items[name]
    lens = np.diff(rec["o"]).astype(np.int64)
    paths = (int(((lens >= 1) & (lens <= 16)).sum()), int(((lens > 16) & (lens <= 1024)).sum()), int((lens > 1024).sum()))
    assert all(paths)  # every path is taken
    res = None
    for measure in zoo.measures(name):
        qn, tn, kw = zoo.norms_for(name, measure)
        rows = SC.ranked_rows(rec, measure, qn, tn)
        for n in SC.TOP_NS:
            res = h.top_by(n, measure, reuse=res, **kw)
            got, want = rec_of(res), SC.top_by_model(rec, measure, n, rows=rows)
            assert not SC.same(got, want), (name, measure, n, SC.same(got, want))
            p = res.plan()
            m = TB_PLAN.fullmatch(p["plan"])
            assert m and int(m.group(1)) == n and tuple(int(m.group(k)) for k in (3, 4, 5)) == paths and p["n_large_queries"] == paths[2], p
            assert res.info() == dict(n_queries=len(lens), n_hits=len(want["t"]))
            if measure == "shared":  # the cross-check between the two implementations
                top = h.top(n)
                assert all(np.array_equal(x, y) for x, y in zip(top.fetch(), (got["o"], got["t"], got["s"]))), (name, n)
                assert not top.has_totals() and not top.has_weights() and not top.has_members()  # bsk_hits_top still drops
                top.close()
    res.close()


def thresholds(measure, fr):
    """(num, den, what): everything, nothing, a hit's own measure (kept) and the smallest step above it (dropped)"""
    if measure == "cosine":  # the bound is on the cosine, N / D is its square: own measures are not expressible, rationals around them are
        return [(0, 1, "all"), (TOP64, 1, "none"), (9, 10, "9/10"), (1, 2, "1/2"), (1, 1, "1"), (TOP64, TOP64 - 1, "just above 1"), (TOP64 - 1, TOP64, "just below 1")]
    best = max(fr, key=lambda f: Fraction(f[0], f[1]))
    mid = sorted(fr, key=lambda f: Fraction(f[0], f[1]))[len(fr) // 2]
    out = [(0, 1, "all"), SC.step_above(*best) + ("none",), (mid[0], mid[1], "own"), SC.step_above(*mid) + ("own + step",)]
    M = TOP64 // max(mid)
    return out + [(mid[0] * M, mid[1] * M, "own, parts near 2^64")]


@pytest.mark.parametrize("name", NAMES)
def test_filter_every_measure_every_threshold(zoo, name):
    h, rec, _, _ = zoo.items[name]
    res = res2 = top = None
    for measure in zoo.measures(name):
        qn, tn, kw = zoo.norms_for(name, measure)
        fr = SC.all_nd(measure, rec, qn, tn)
        top = h.top_by(17, measure, reuse=top, **kw)  # rows that are not ascending: legal input
        trec = rec_of(top)
        for num, den, what in thresholds(measure, fr):
            res = h.filter(measure, (num, den), reuse=res, **kw)
            got, want = rec_of(res), SC.filter_model(rec, measure, num, den, fractions_=fr)
            assert not SC.same(got, want), (name, measure, what, SC.same(got, want))
            if what == "all":
                assert not SC.same(got, rec)
            if what == "none":
                assert len(got["t"]) == 0 and not got["o"].any()
            if what == "own":
                assert len(got["t"]) > 0
            if what == "own + step":
                assert len(got["t"]) < kept_own
            kept_own = len(got["t"]) if what == "own" else None
            m = FL_PLAN.fullmatch(res.plan()["plan"])
            assert m and int(m.group(2)) == len(rec["t"]) and int(m.group(3)) == len(want["t"]) and res.plan()["n_large_queries"] == 0
            res2 = top.filter(measure, (num, den), reuse=res2, **kw)
            assert not SC.same(rec_of(res2), SC.filter_model(trec, measure, num, den, qn, tn)), (name, measure, what, "after top_by")
    for x in (res, res2, top):
        x.close()


def test_empty_hits_and_no_queries(engine):
    for o in (np.zeros(1, U64), np.zeros(5, U64)):
        h = engine.hits_from_arrays(o, np.zeros(0, U32), np.zeros(0, U32))
        for res in (h.filter("shared", 1), h.top_by(3, "shared"), h.filter("query_cov", 0.5, qnorm=np.ones(len(o) - 1, U64)),
                    h.top_by(3, "jaccard", qnorm=np.ones(len(o) - 1, U64), tnorm=np.ones(1, U64))):
            assert res.info() == dict(n_queries=len(o) - 1, n_hits=0) and np.array_equal(res.fetch()[0], o)
            res.close()
        h.close()


# ---- wide arithmetic ----
def test_norms_up_to_the_top_of_u64(engine):
    """Q + T wraps a u64, the cross products pass 128 bits"""
    rec = SC.record([0, 4, 7], [0, 1, 2, 3, 1, 2, 3], [TOP64 >> 32, 3, 3, 2, 7, 7, 1])
    h = engine.hits_from_arrays(rec["o"], rec["t"], rec["s"])
    qn, tn = np.array([TOP64, TOP64 - 5], U64), np.array([TOP64, TOP64 - 1, TOP64 - 2, 1 << 63], U64)
    for measure in ("query_cov", "target_cov", "jaccard"):
        fr = SC.all_nd(measure, rec, qn, tn)
        for n in (1, 2, 4):
            got = rec_of(h.top_by(n, measure, qnorm=qn, tnorm=tn))
            assert not SC.same(got, SC.top_by_model(rec, measure, n, qn, tn)), (measure, n)
        for N, D in fr:
            for num, den in ((N, D), SC.step_above(N, D)) if D <= TOP64 else ((1, TOP64), (TOP64, 1), (3, TOP64 - 1)):
                got = rec_of(h.filter(measure, (num, den), qnorm=qn, tnorm=tn))
                assert not SC.same(got, SC.filter_model(rec, measure, num, den, fractions_=fr)), (measure, num, den)
    # 3 / (2^64-2) against 3 / (2^64-3): equal as doubles, told apart here
    assert SC.nd("target_cov", rec, 0, 1, qn, tn) != SC.nd("target_cov", rec, 0, 2, qn, tn)
    assert list(rec_of(h.top_by(4, "target_cov", tnorm=tn))["t"][:4]) == [0, 3, 2, 1]
    h.close()


def test_counts_at_the_edge_of_the_formats(engine):
    q, t = SC.wide_sets()
    a, b = counted(engine, q), counted(engine, t)
    h = a.neighbors_counted(b)
    rec = rec_of(h)
    m = (1 << 32) - 1
    assert list(rec["t"]) == [0, 1, 2, 3] and [int(x) for x in rec["dot"]] == [m * m, TOP64, 3 << 32, 5 << 32]  # exact, saturated, multiples of 2^32
    qs, ts = a.sumsq(), b.sumsq()
    assert int(qs[0]) == int(ts[0]) == m * m
    # the cosine of exactly 1: kept at 1, dropped one step above it, with the operands' own norms
    one = rec_of(h.filter("cosine", (1, 1)))
    assert 0 in list(one["t"]) and not SC.same(one, SC.filter_model(rec, "cosine", 1, 1, qs, ts))
    for num, den in ((TOP64, TOP64), (TOP64, TOP64 - 1), (TOP64 - 1, TOP64), (1 << 63, (1 << 63) + 1)):
        got = rec_of(h.filter("cosine", (num, den)))
        assert not SC.same(got, SC.filter_model(rec, "cosine", num, den, qs, ts)), (num, den)
    assert 0 not in list(rec_of(h.filter("cosine", (TOP64, TOP64 - 1)))["t"])
    # the saturated dot is the number 2^64-1
    assert list(rec_of(h.filter("dot", (TOP64, 1)))["t"]) == [1] and list(rec_of(h.top_by(1, "dot"))["t"]) == [0, 1]
    # fractions whose cross products agree in their low 128 bits: N = dot^2 and D = Q T are multiples of 2^64 for targets 2 and 3
    qn, tn = np.array([1, 1 << 63], U64), np.array([1, 1, 38, 14], U64)
    fr = SC.all_nd("cosine", rec, qn, tn)
    assert (fr[2][0] * fr[3][1]) % (1 << 128) == (fr[3][0] * fr[2][1]) % (1 << 128) == 0 and fr[2][0] * fr[3][1] != fr[3][0] * fr[2][1]
    for n in (1, 2, 3):
        got = rec_of(h.top_by(n, "cosine", qnorm=qn, tnorm=tn))
        assert not SC.same(got, SC.top_by_model(rec, "cosine", n, qn, tn)), n
    assert list(rec_of(h.top_by(3, "cosine", qnorm=qn, tnorm=tn))["t"][1:]) == [1, 3, 2]  # 9/19 < 25/7: by the high bits alone
    # ... and fractions that differ only below the 128th bit of products near 2^256
    qn, tn = np.array([TOP64, TOP64], U64), np.array([TOP64, TOP64, TOP64, TOP64 - 1], U64)
    for n in (1, 3):
        assert not SC.same(rec_of(h.top_by(n, "cosine", qnorm=qn, tnorm=tn)), SC.top_by_model(rec, "cosine", n, qn, tn)), n
    for num, den in ((TOP64, TOP64), (1, TOP64), (TOP64 - 1, TOP64)):
        assert not SC.same(rec_of(h.filter("cosine", (num, den), qnorm=qn, tnorm=tn)), SC.filter_model(rec, "cosine", num, den, qn, tn)), (num, den)
    for x in (h, a, b):
        x.close()


# ---- the result slot ----
def test_reuse_into_objects_of_every_history(zoo):
    engine = zoo.engine
    h, rec, _, _ = zoo.items["totals+weights"]
    small = engine.hits_from_arrays(np.array([0, 1], U64), np.array([3], U32), np.array([9], U32))  # smaller, no payloads
    large = zoo.items["none"][0].fold(np.arange(0, 4201, 2, dtype=U64))  # with members, which the result must not show
    for slot in (small, large):
        res = h.filter("cosine", Fraction(1, 2), reuse=slot)
        assert res is slot and not SC.same(rec_of(res), SC.filter_model(rec, "cosine", 1, 2, zoo.a.sumsq(), zoo.b.sumsq()))
        assert not res.has_members()
        res = h.top_by(3, "min_sum", reuse=slot)
        assert res is slot and not SC.same(rec_of(res), SC.top_by_model(rec, "min_sum", 3))
        # a result with weights, re-used for hits without: the flags follow the input
        plain = zoo.items["none"][0].top_by(2, "shared", reuse=slot)
        assert plain is slot and not plain.has_weights() and not plain.has_totals() and not SC.same(rec_of(plain), SC.top_by_model(zoo.items["none"][1], "shared", 2))
        slot.close()


def test_every_argument_error_keeps_the_slot(zoo):
    engine, lib = zoo.engine, zoo.engine.lib
    h, rec, norms, _ = zoo.items["totals+weights"]
    plain = zoo.items["none"][0]
    res = h.top_by(2, "dot")
    before, slot = rec_of(res), C.c_void_p(res.h.value)
    qs, ts = norms["sumsq"]
    nq, nt = len(qs), len(ts)
    other = S.Engine(0)
    foreign = other.hits_from_arrays(np.array([0, 1], U64), np.array([0], U32), np.array([1], U32))
    fslot = C.c_void_p(foreign.h.value)

    def measure(kind, q=qs, t=ts, flags=0, n_q=None, n_t=None):
        return L.Measure(kind, flags, None if q is None else q.ctypes.data, (0 if q is None else len(q)) if n_q is None else n_q, None if t is None else t.ctypes.data,
                         (0 if t is None else len(t)) if n_t is None else n_t)

    zeros_q, zeros_t, ones_q = np.zeros(nq, U64), np.zeros(nt, U64), np.ones(nq, U64)
    fp, fp0 = L.FilterParams(1, 2), L.FilterParams(1, 0)
    bad = [("unknown kind", engine.ctx, h.h, measure(11), slot), ("flag", engine.ctx, h.h, measure(L.MEASURE_COSINE, flags=1), slot),
           ("no members", engine.ctx, h.h, measure(L.MEASURE_MEMBERS), slot), ("no weights", engine.ctx, plain.h, measure(L.MEASURE_COSINE), slot),
           ("no qnorm", engine.ctx, h.h, measure(L.MEASURE_COSINE, q=None), slot), ("no tnorm", engine.ctx, h.h, measure(L.MEASURE_COSINE, t=None), slot),
           ("n_qnorm", engine.ctx, h.h, measure(L.MEASURE_COSINE, n_q=nq - 1), slot), ("target >= n_tnorm", engine.ctx, h.h, measure(L.MEASURE_COSINE, n_t=100), slot),
           ("D == 0 by Q", engine.ctx, h.h, measure(L.MEASURE_COSINE, q=zeros_q), slot), ("D == 0 by T", engine.ctx, h.h, measure(L.MEASURE_TARGET_COV, t=zeros_t), slot),
           ("D < 0", engine.ctx, h.h, measure(L.MEASURE_WEIGHTED_JACCARD, q=zeros_q, t=zeros_t), slot),
           ("D == 0 in BC", engine.ctx, h.h, measure(L.MEASURE_BC_SIMILARITY, q=zeros_q, t=zeros_t), slot),
           ("D < 0 in Jaccard", engine.ctx, plain.h, measure(L.MEASURE_JACCARD, q=np.zeros(plain.info()["n_queries"], U64), t=np.zeros(4200, U64)), slot),
           ("*out == h", engine.ctx, res.h, measure(L.MEASURE_SHARED), slot), ("foreign hits", engine.ctx, foreign.h, measure(L.MEASURE_SHARED), slot),
           ("foreign context", other.ctx, h.h, measure(L.MEASURE_SHARED), slot), ("foreign slot", engine.ctx, h.h, measure(L.MEASURE_SHARED), fslot),
           ("null hits", engine.ctx, None, measure(L.MEASURE_SHARED), slot), ("null ctx", None, h.h, measure(L.MEASURE_SHARED), slot)]
    for what, ctx, hh, m, sl in bad:
        held = sl.value
        assert lib.bsk_hits_filter(ctx, hh, C.byref(m), C.byref(fp), C.byref(sl)) == L.ERR_ARG and sl.value == held, ("filter", what)
        assert lib.bsk_hits_top_by(ctx, hh, C.byref(m), 3, C.byref(sl)) == L.ERR_ARG and sl.value == held, ("top_by", what)
        assert not SC.same(rec_of(res), before), what  # readable and unchanged
    ok = measure(L.MEASURE_QUERY_MASS, q=ones_q, t=None)
    assert lib.bsk_hits_filter(engine.ctx, h.h, C.byref(ok), C.byref(fp0), C.byref(slot)) == L.ERR_ARG and slot.value == res.h.value  # min_den == 0
    assert lib.bsk_hits_filter(engine.ctx, h.h, C.byref(ok), None, C.byref(slot)) == L.ERR_ARG and slot.value == res.h.value
    assert lib.bsk_hits_filter(engine.ctx, h.h, None, C.byref(fp), C.byref(slot)) == L.ERR_ARG and slot.value == res.h.value
    assert lib.bsk_hits_top_by(engine.ctx, h.h, C.byref(ok), 0, C.byref(slot)) == L.ERR_ARG and slot.value == res.h.value  # n == 0
    assert lib.bsk_hits_filter(engine.ctx, h.h, C.byref(ok), C.byref(fp), None) == L.ERR_ARG and lib.bsk_hits_top_by(engine.ctx, h.h, C.byref(ok), 3, None) == L.ERR_ARG
    assert b"bsk_hits_top_by" in lib.bsk_last_error(engine.ctx)
    assert not SC.same(rec_of(res), before)
    # ... and the same calls with nothing wrong go through, into that slot
    assert lib.bsk_hits_filter(engine.ctx, h.h, C.byref(ok), C.byref(fp), C.byref(slot)) == L.OK and slot.value == res.h.value
    assert not SC.same(rec_of(res), SC.filter_model(rec, "weighted_containment", 1, 2, ones_q, None))
    with pytest.raises(S.DeviceError, match="bad argument: bsk_hits_filter: the result slot holds h itself"):
        res.filter("shared", 1, reuse=res)
    with pytest.raises(ValueError, match="64 bits"):
        h.filter("shared", Fraction(1 << 64, 3))
    with pytest.raises(ValueError, match="64 bits"):
        h.filter("jaccard", 1e-30)
    with pytest.raises(ValueError, match="measure"):
        h.top_by(1, "manhattan")
    for x in (res, foreign, other):
        x.close()


# ---- the chains ----
def test_clusters_by_a_weighted_measure(engine):
    rng = np.random.default_rng(21)
    n, offs, vals, cnts = 90, [0], [], []
    for i in range(n):  # families of sets around a few centres: the cosines spread over 0 .. 1
        base = 100 * (i % 9)
        v = np.unique(np.concatenate([base + np.arange(12), base + rng.integers(0, 40, 6)])).astype(U64)
        c = np.where(v < base + 12, 5 + (v % 7) * 2, rng.integers(1, 13, len(v))).astype(U32)  # the family's pattern, and noise beside it
        vals.append(v), cnts.append(c), offs.append(offs[-1] + len(v))
    a = engine.sets_from_arrays_counted(np.array(offs, U64), np.concatenate(vals), np.concatenate(cnts))
    h = a.neighbors_counted(a)
    rec, sq = rec_of(h), a.sumsq()
    f = h.filter("cosine", Fraction(9, 10))
    want = SC.filter_model(rec, "cosine", 9, 10, sq, sq)
    assert not SC.same(rec_of(f), want) and n < len(want["t"]) < len(rec["t"])  # more than the diagonal, fewer than all
    got = f.cluster()
    ref = engine.hits_from_arrays(want["o"], want["t"], want["s"]).cluster()
    assert np.array_equal(got.label, ref.label) and np.array_equal(got.rep, ref.rep) and 1 < got.info()["n_clusters"] < n
    # the float form of the same bound, taken exactly
    assert not SC.same(rec_of(h.filter("cosine", 0.9)), SC.filter_model(rec, "cosine", *(0.9).as_integer_ratio(), sq, sq))
    # the Python norm rule: the result keeps the norms, an operand overwritten before the first use refuses
    cos = f.cosine()
    h2 = a.neighbors_counted(a)
    a.close()
    assert np.array_equal(f.cosine(), cos) and np.all(cos >= 0.9 - 1e-12)  # (the operands are closed: the norms came along)
    g = f.filter("cosine", Fraction(19, 20))
    assert not SC.same(rec_of(g), SC.filter_model(rec_of(f), "cosine", 19, 20, sq, sq)) and 0 < len(g.target) < len(f.target)
    assert np.all(g.cosine() >= 0.95 - 1e-12) and np.all(g.weighted_jaccard() > 0)
    with pytest.raises(ValueError, match="written or closed"):
        h2.filter("cosine", Fraction(9, 10))
    with pytest.raises(ValueError, match="written or closed"):
        h2.top_by(3, "weighted_jaccard")
    assert h2.top_by(3, "dot").info()["n_hits"] == 3 * n  # a measure without norms still runs


def test_the_best_genome_keeps_its_members(zoo):
    engine = zoo.engine
    q, t = SC.weighted_sets()
    hits = zoo.b.index().search(zoo.a)
    go = np.arange(0, len(t[0]), 3, dtype=U64)  # genomes of three chunks
    go[-1] = len(t[0]) - 1
    folded = hits.fold(go)
    frec = rec_of(folded)
    best = folded.top_by(1, "members")
    got = rec_of(best)
    assert not SC.same(got, SC.top_by_model(frec, "members", 1)) and got["members"] is not None and best.has_members() and int(got["members"].max()) == 3
    assert np.array_equal(best.members, got["members"])
    # weighted containment against the index without counts, the restriction of the formula
    plain, prec, pn, _ = zoo.items["weights, plain index"]
    assert not SC.same(rec_of(plain.filter("weighted_containment", Fraction(1, 3))), SC.filter_model(prec, "weighted_containment", 1, 3, pn["totals"][0], None))
    with pytest.raises(ValueError, match="index without counts"):
        zoo.items["weights"][0].filter("weighted_containment", Fraction(1, 3))
    with pytest.raises(ValueError, match="Index.search_counted"):
        zoo.items["totals+weights"][0].top_by(1, "weighted_containment")


# ---- the grid caps ----
def caps_record(engine):
    """600 rows of up to 16 hits, eight rows for a wavefront and two for a workgroup; with totals"""
    rng = np.random.default_rng(5)
    lens = [int(x) for x in rng.integers(0, 17, 600)]
    for r, c in ((7, 100), (99, 1024), (200, 17), (201, 64), (333, 500), (400, 65), (401, 300), (599, 31), (50, 1025), (450, 1500)):
        lens[r] = c
    o = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    t = np.concatenate([np.sort(rng.choice(3000, size=c, replace=False)) for c in lens]).astype(U32)
    s = rng.integers(1, 6, len(t)).astype(U32)
    return SC.record(o, t, s, s * rng.integers(1, 4, len(t)).astype(U32))


@pytest.mark.parametrize("entry", ["filter", "top_by"])
def test_under_a_grid_cap_the_record_is_the_same(engine, entry):
    rec = caps_record(engine)
    h = upload(engine, rec)
    call = (lambda: h.filter("jaccard", Fraction(1, 2))) if entry == "filter" else (lambda: h.top_by(20, "jaccard"))
    want = SC.filter_model(rec, "jaccard", 1, 2) if entry == "filter" else SC.top_by_model(rec, "jaccard", 20)
    records = {}
    for cap in (None,) + GRID_CAPS:
        with switches(engine, dict(BSK_GRID_CAP=None if cap is None else str(cap))):
            s0, c0 = grid_stats(engine)
            records[cap] = rec_of(call())
            s1, c1 = grid_stats(engine)
        sized, cut = s1 - s0, c1 - c0
        assert sized >= 3, (entry, cap, sized)
        if cap is None:
            assert cut == 0, (entry, sized, cut)
        elif cap == 1:
            assert cut == sized, (entry, "every grid of the call is cut at cap 1", sized, cut)
        else:
            assert cut > 0, (entry, cap)
        assert not SC.same(records[cap], want), (entry, cap)
    h.close()
