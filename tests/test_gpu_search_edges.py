"""GPU: the containment search at the places where search.hip changes behaviour.

Every test builds inputs for one edge (tests/search_cases.py), asserts that the device reached it -- the exact number of large
queries, the exact directory statistics, sizes beyond one pass of the capped grids for this device's CU count -- and then compares
offsets, target ids and shared counts exactly with the NumPy reference."""
import ctypes as C
import functools

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import search_cases as SC
from tests.search_cases import collection, ref_search

pytestmark = pytest.mark.gpu
U64 = np.uint64


@functools.lru_cache(None)
def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipDeviceGetAttribute.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
    return hip


def one_pass(engine):
    """how many items one pass of each capped grid of bsk_index_search covers on device 0 (grid_for in sets_internal.hpp)"""
    v = C.c_int()
    assert _hip().hipDeviceGetAttribute(C.byref(v), 63, 0) == 0  # hipDeviceAttributeMultiprocessorCount
    cus = v.value
    assert cus > 0
    return dict(cus=cus, lookup=cus * 512, move=cus * 512, small=cus * 160, list_large=cus * 2048, emit=cus * 64)


def check(hits, want):
    o, t, s = hits.fetch()
    assert np.array_equal(o, want[0]), "offsets"
    assert np.array_equal(t, want[1]), "targets"
    assert np.array_equal(s, want[2]), "shared"


def search(engine, ix, tg, qs, want=None, **kw):
    """search, assert the large-path count against the host's posting sums, compare exactly with the reference"""
    hits = ix.search(engine.sets_from_arrays(*qs), **kw)
    n_large = int((SC.posting_sums(*tg, *qs) > SC.SR_CAP).sum())
    assert hits.plan()["n_large_queries"] == n_large, (hits.plan(), n_large)
    if want is None:
        want = ref_search(*tg, *qs, kw.get("min_shared", 1), kw.get("min_query_cov", 0.0), kw.get("min_target_cov", 0.0))
    check(hits, want)
    return hits, want


def index_and_search(engine, tg, qs, **kw):
    ix = engine.sets_from_arrays(*tg).index()
    hits, want = search(engine, ix, tg, qs, **kw)
    return ix, hits, want


# ---- the directory ----
@pytest.mark.parametrize("n_targets", [0, 5])
def test_index_without_values(engine, n_targets):
    """no targets, or only empty ones: U = 0, one empty bucket; every lookup misses"""
    tg = (np.zeros(n_targets + 1, U64), np.zeros(0, U64))
    ix = engine.sets_from_arrays(*tg).index()
    inf = ix.info()
    assert (inf["n_targets"], inf["n_postings"], inf["n_distinct"], inf["max_bucket"]) == (n_targets, 0, 0, 0), inf
    qs = collection([[0], [1, 2, 3], [], [2**64 - 1], SC.unmix64([0, 1, 2**63, 2**64 - 1])])
    hits, _ = search(engine, ix, tg, qs)
    assert hits.info() == dict(n_queries=5, n_hits=0)


@pytest.mark.parametrize("name", SC.LAYOUTS)
def test_directory_layouts(engine, name):
    """n_distinct and max_bucket exactly as the host's mixer and directory predict; lookups of the first, middle and last key of
    the fullest bucket, of keys just outside it and between its keys, and of empty buckets next to full ones"""
    vals, _ = SC.layout(name)
    d = SC.directory(vals)
    rng = np.random.default_rng(len(vals))
    n_t = 40
    holder = rng.integers(0, n_t, len(vals))
    second = rng.random(len(vals)) < 0.3
    tt = np.concatenate([holder, (holder[second] + 1 + rng.integers(0, n_t - 1, second.sum())) % n_t])
    tv = np.concatenate([vals, vals[second]])
    tsets = [[]] * 3 + [tv[tt == t] for t in range(n_t)] + [[]] * 4  # leading and trailing runs of empty targets
    tg = collection(tsets)
    probes = SC.unmix64(SC.probe_keys(d))
    qsets = [[p] for p in probes] + [probes, []]
    miss = rng.integers(0, 2**64, 3000, dtype=U64)
    qsets += [np.concatenate([vals[rng.integers(0, len(vals), rng.integers(0, 20))], miss[rng.integers(0, 3000, rng.integers(0, 10))]])
              for _ in range(2000)]
    qs = collection(qsets)
    ix, hits, (o, _, _) = index_and_search(engine, tg, qs)
    inf = ix.info()
    assert inf["n_distinct"] == d["n_distinct"] and inf["max_bucket"] == d["max_bucket"], (inf, d["max_bucket"])
    assert inf["n_targets"] == n_t + 7 and inf["n_postings"] == len(tv)
    hit = np.diff(o)[:len(probes)] > 0
    assert np.array_equal(hit, np.isin(probes, vals)) and hit.any()


# ---- posting-count edges ----
def test_posting_sum_edges(engine):
    """sums 1, 63, 64, 65, 2047, 2048, 2049, 5 000 made several ways, and runs of 8 .. 40 queries of exactly 2 048 (the whole LDS
    slice of a wavefront, four wavefronts side by side) between runs of tiny queries"""
    tg, qs, cl = SC.posting_edge_case()
    ix, hits, _ = index_and_search(engine, tg, qs)
    assert hits.plan()["n_large_queries"] == cl["n_large"] == (cl["sums"] > SC.SR_CAP).sum()
    search(engine, ix, tg, qs, min_shared=2)
    search(engine, ix, tg, qs, min_query_cov=0.02, min_target_cov=0.5)


@pytest.mark.parametrize("n_targets", [1, 2, 3])
def test_staging_clamp(engine, n_targets):
    """posting sums far above T on both paths: a query's staging span is min(sum, T)"""
    tg, qs, cl = SC.clamp_case(n_targets)
    ix, hits, _ = index_and_search(engine, tg, qs)
    assert hits.plan()["n_large_queries"] == cl["n_large"] >= 2
    search(engine, ix, tg, qs, min_query_cov=0.5)


def test_long_posting_lists_in_large_queries(engine):
    """k_lg_emit: lists of 63 and 64 ids (one lane), 65, 128 and 129 (the whole wavefront) at value index 0, 63 and beyond 64"""
    tg, qs, cl = SC.list_length_case()
    ix, hits, _ = index_and_search(engine, tg, qs)
    assert hits.plan()["n_large_queries"] == cl["n_large"] == len(cl["sums"]) - 1 + int(cl["large"][-1])


@pytest.mark.parametrize("n_large,last_only", [(n, False) for n in (1, 2, 3, 4, 5, 255, 256, 257)] + [(1, True)])
def test_number_of_large_queries(engine, n_large, last_only):
    """NL large queries -- the slot sort runs over 32 + ceil(log2 NL) bits -- first, last and interleaved; with min_shared = 2 the
    large query that shares one value with each target lists nothing, its large neighbours keep hits"""
    tg, qs, cl = SC.nl_case(n_large, last_only)
    ix, hits, _ = index_and_search(engine, tg, qs)
    assert hits.plan()["n_large_queries"] == n_large == cl["n_large"]
    hits2, (o, _, _) = search(engine, ix, tg, qs, min_shared=2)
    nh = np.diff(o)
    if n_large > 2:
        assert nh[1] == 0 and (nh[cl["large"]] > 0).sum() == n_large - 1


_EDGE_KW = [dict(min_query_cov=qc) for qc in (0.1, 1 / 3, 0.5, 1.0)] + \
    [dict(min_target_cov=tc, min_shared=ms) for tc, ms in ((0.1, 1), (0.3, 1), (1.0, 1), (0.0, 7), (0.25, 30), (0.0, 0))]


@pytest.mark.parametrize("kw", _EDGE_KW, ids=["-".join(f"{k}={v:.3g}" for k, v in kw.items()) for kw in _EDGE_KW])
def test_threshold_edges_on_the_large_path(engine, kw):
    """test_gpu_search's threshold edges with every query on the large path (k_lg_keep evaluates the rule); containment and
    Jaccard against float64 from the reference"""
    tg, qs, cl = SC.edge_large_case()
    ix, hits, (o, t, s) = index_and_search(engine, tg, qs, **kw)
    assert hits.plan()["n_large_queries"] == len(qs[0]) - 1 == cl["n_large"]
    q = np.repeat(np.arange(len(o) - 1), np.diff(o).astype(np.int64))
    qn, tn = np.diff(qs[0])[q].astype(np.float64), np.diff(tg[0])[t.astype(np.int64)].astype(np.float64)
    sf = s.astype(np.float64)
    assert np.array_equal(hits.containment(), sf / qn) and np.array_equal(hits.jaccard(), sf / (qn + tn - sf))


# ---- beyond one pass of the capped grids ----
_COMP = np.frombuffer(b"TGCA", np.uint8)
_CODE = np.zeros(256, np.uint8)
_CODE[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4)


def _splice(qs, at, v):
    """the collection qs with the set v inserted before query `at`"""
    o, x = qs
    a = int(o[at])
    sizes = np.insert(np.diff(o), at, len(v))
    offs = np.zeros(len(sizes) + 1, U64)
    offs[1:] = np.cumsum(sizes)
    return offs, np.concatenate([x[:a], v, x[a:]])


def test_reads_against_genomes_beyond_one_grid(engine):
    """more reads than one pass of k_sr_lookup, k_sr_small, k_sr_move and k_sr_list_large covers, and three genome-size queries
    on the large path, two of them beyond k_sr_list_large's first pass"""
    lim = one_pass(engine)
    rng = np.random.default_rng(21)
    G, glen, rlen = 50, 200_000, 150
    nreads = max(800_000, int(lim["list_large"] * 1.5) + 1)
    genomes = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, G * glen)]
    goffs = np.arange(G + 1, dtype=U64) * U64(glen)
    p = engine.params(L.MINIMIZER, k=21, w=11)
    gsets = engine.run(engine.batch_from_arrays(genomes, goffs), p).device_sets()
    ix = gsets.index()
    tg = gsets.fetch()
    gsets.close()
    src = rng.integers(0, G, nreads)
    reads = sliding_window_view(genomes, rlen)[src * glen + rng.integers(0, glen - rlen + 1, nreads)]
    rc = rng.random(nreads) < 0.5
    reads[rc] = _COMP[_CODE[reads[rc][:, ::-1]]]
    roffs = np.arange(nreads + 1, dtype=U64) * U64(rlen)
    rsets = engine.run(engine.batch_from_arrays(reads.reshape(-1), roffs), p).device_sets()
    qs = rsets.fetch()
    rsets.close()
    del reads
    gv = [tg[1][int(tg[0][g]):int(tg[0][g + 1])] for g in (3, 7, 11)]
    qs = _splice(qs, nreads, gv[2])
    qs = _splice(qs, nreads, gv[1])
    at = lim["list_large"] + 1000
    qs = _splice(qs, at, gv[0])
    nq = len(qs[0]) - 1
    assert nq > max(lim["lookup"], lim["small"], lim["move"], lim["list_large"]) and at > lim["list_large"], (nq, lim)
    sums = SC.posting_sums(*tg, *qs)
    assert np.array_equal(np.flatnonzero(sums > SC.SR_CAP), [at, nq - 2, nq - 1])
    counts = SC.ref_counts(*tg, *qs)
    for kw in (dict(), dict(min_query_cov=0.5)):
        want = SC.ref_select(counts, tg[0], qs[0], 1, kw.get("min_query_cov", 0.0))
        hits, _ = search(engine, ix, tg, qs, want=want, **kw)
        assert hits.plan()["n_large_queries"] == 3 and hits.info()["n_hits"] > lim["move"]


def test_boundary_dense_beyond_one_grid(engine):
    """posting sums straddling SR_CAP: about half of the queries on each path, more large queries than one pass of k_lg_emit, more
    queries than one pass of k_sr_small, with sums near 2 048 among those beyond it"""
    lim = one_pass(engine)
    n_large = lim["emit"] * 5 // 4 + 500
    tg, qs, cl = SC.boundary_case(n_large, n_large)
    nq = len(qs[0]) - 1
    assert n_large > lim["emit"] * 1.25 and nq > lim["small"], (n_large, nq, lim)
    late = cl["sums"][lim["small"]:]
    assert ((late > 1024) & (late <= SC.SR_CAP)).any() and (late > SC.SR_CAP).any()
    ix, hits, _ = index_and_search(engine, tg, qs)
    assert hits.plan()["n_large_queries"] == n_large == cl["n_large"]


def test_s2_all_vs_all(engine):
    """scripts/perf_search.py's S2 at its measured size: 2 000 sets of 10^4 values from a pool of 10^6, all against all, every
    query on the large path; the reference is the exact 2 000 x 2 000 matrix of shared counts"""
    offs, vals = SC.s2_case()
    n = len(offs) - 1
    sets = engine.sets_from_arrays(offs, vals)
    ix = sets.index()
    m = SC.s2_matrix(offs, vals)
    size = np.diff(offs).astype(np.int64)
    assert np.array_equal(np.diag(m), size)
    for kw in (dict(), dict(min_shared=100, min_query_cov=0.0101, min_target_cov=0.0099)):
        hits = ix.search(sets, **kw)
        assert hits.plan()["n_large_queries"] == n
        o, t, s = hits.fetch()
        q = np.repeat(np.arange(n), np.diff(o).astype(np.int64))
        ti = t.astype(np.int64)
        assert ((np.diff(ti) > 0) | (np.diff(q) > 0)).all()  # targets strictly ascending inside a query
        got = np.zeros((n, n), np.int64)
        got[q, ti] = s
        ms, qc, tc = kw.get("min_shared", 1), kw.get("min_query_cov", 0.0), kw.get("min_target_cov", 0.0)
        mf = m.astype(np.float64)
        keep = (m >= ms) & (mf >= qc * size[:, None].astype(np.float64)) & (mf >= tc * size[None, :].astype(np.float64))
        assert len(t) == int(keep.sum()) and np.array_equal(got, np.where(keep, m, 0))
        if not kw:
            assert np.array_equal(np.diag(got), size) and len(t) == int((m > 0).sum())
        else:
            assert 0.2 * n * n < len(t) < 0.8 * n * n


# ---- API edges ----
def test_zero_queries_and_only_empty_queries(engine):
    tg = collection([[1, 2, 3], [3, 4], []])
    ix = engine.sets_from_arrays(*tg).index()
    for qs in ((np.zeros(1, U64), np.zeros(0, U64)), collection([[]] * 5)):
        nq = len(qs[0]) - 1
        hits, _ = search(engine, ix, tg, qs)
        assert hits.info() == dict(n_queries=nq, n_hits=0) and hits.plan()["n_large_queries"] == 0
        o, t, s = hits.fetch()
        assert np.array_equal(o, np.zeros(nq + 1, U64)) and len(t) == len(s) == 0
        assert len(hits.fetch(nq, 0)[0]) == 1


def test_fetch_subranges_and_bad_ranges(engine):
    """bsk_hits_fetch(first, count): offsets rebased, the hits of exactly those queries; ranges outside the hits and a hit_cap
    below their hits are BSK_ERR_ARG"""
    tg, qs, cl = SC.nl_case(5)
    ix, hits, (o, t, s) = index_and_search(engine, tg, qs)
    nq = len(o) - 1
    big = np.flatnonzero(cl["large"])
    g = int(big[2])
    ranges = [(0, 0), (nq, 0), (nq - 1, 1), (0, nq), (0, 1), (g, 1), (g, 3), (g - 2, 3), (g + 1, nq - g - 1), (3, 7), (1, nq - 1)]
    for first, count in ranges:
        fo, ft, fs = hits.fetch(first, count)
        a, b = int(o[first]), int(o[first + count])
        assert np.array_equal(fo, o[first:first + count + 1] - o[first]), (first, count)
        assert np.array_equal(ft, t[a:b]) and np.array_equal(fs, s[a:b]), (first, count)
    lib, ctx = engine.lib, engine.ctx
    buf = np.zeros(nq + 2, U64)
    tb, sb = np.zeros(len(t) + 1, np.uint32), np.zeros(len(t) + 1, np.uint32)
    for first, count in ((nq + 1, 0), (nq, 1), (1, nq), (0, nq + 1), (5, 2**64 - 1)):
        assert lib.bsk_hits_fetch(ctx, hits.h, first, count, buf.ctypes.data, None, None, 0) == L.ERR_ARG, (first, count)
    nh = int(o[-1]) - int(o[1])
    assert nh > 0
    assert lib.bsk_hits_fetch(ctx, hits.h, 1, nq - 1, buf.ctypes.data, tb.ctypes.data, sb.ctypes.data, nh - 1) == L.ERR_ARG
    assert lib.bsk_hits_fetch(ctx, hits.h, 1, nq - 1, buf.ctypes.data, tb.ctypes.data, None, nh - 1) == L.ERR_ARG
    assert lib.bsk_hits_fetch(ctx, hits.h, 1, nq - 1, buf.ctypes.data, tb.ctypes.data, sb.ctypes.data, nh) == L.OK
    assert np.array_equal(tb[:nh], t[int(o[1]):]) and np.array_equal(sb[:nh], s[int(o[1]):])
    assert lib.bsk_hits_fetch(ctx, hits.h, 1, nq - 1, buf.ctypes.data, None, None, 0) == L.OK
    assert np.array_equal(buf[:nq], o[1:] - o[1])


def test_device_pointers_equal_fetch(engine):
    tg, qs, _ = SC.nl_case(4)
    ix, hits, (o, t, s) = index_and_search(engine, tg, qs)
    po, pt, ps = hits.device()
    hip = _hip()

    def d2h(ptr, m, dt):
        a = np.empty(m, dt)
        if m:
            assert hip.hipMemcpy(a.ctypes.data, ptr, a.nbytes, 2) == 0
        return a

    assert np.array_equal(d2h(po, len(o), np.uint64), o)
    assert np.array_equal(d2h(pt, len(t), np.uint32), t) and np.array_equal(d2h(ps, len(s), np.uint32), s)


def test_owners_closed_early(engine):
    """the target sets closed right after the build, the queries and the index before the hits are fetched"""
    tg, qs, cl = SC.nl_case(4)
    want = ref_search(*tg, *qs)
    ts = engine.sets_from_arrays(*tg)
    ix = ts.index()
    ts.close()
    q = engine.sets_from_arrays(*qs)
    hits = ix.search(q)
    q.close()
    ix.close()
    assert hits.plan()["n_large_queries"] == cl["n_large"]
    check(hits, want)


def test_reuse_after_argument_error_and_across_indexes(engine):
    """an argument error leaves a reused hits object holding the earlier result; one hits object serves two indexes"""
    tga, qsa, _ = SC.nl_case(4)
    tgb, qsb, _ = SC.posting_edge_case()
    ixa = engine.sets_from_arrays(*tga).index()
    ixb = engine.sets_from_arrays(*tgb).index()
    qa, qb = engine.sets_from_arrays(*qsa), engine.sets_from_arrays(*qsb)
    hits = ixa.search(qa)
    first = hits.fetch()
    plan = hits.plan()
    for kw in (dict(min_query_cov=2.0), dict(min_target_cov=float("nan"))):
        with pytest.raises(S.DeviceError):
            ixa.search(qa, reuse=hits, **kw)
        assert hits.h and hits.plan() == plan
        assert all(np.array_equal(x, y) for x, y in zip(hits.fetch(), first))
    for ix, tg, q, qs in ((ixb, tgb, qb, qsb), (ixa, tga, qa, qsa), (ixb, tgb, qb, qsb)):
        hits = ix.search(q, reuse=hits)
        assert hits.plan()["n_large_queries"] == int((SC.posting_sums(*tg, *qs) > SC.SR_CAP).sum())
        check(hits, ref_search(*tg, *qs))


def test_other_context_rejected(engine):
    """an index, queries or hits of one Engine are not accepted by another"""
    tg, qs, _ = SC.nl_case(2)
    ix = engine.sets_from_arrays(*tg).index()
    mine = engine.sets_from_arrays(*qs)
    hits = ix.search(mine)
    other = S.Engine(0)
    try:
        theirs = other.sets_from_arrays(*qs)
        with pytest.raises(S.DeviceError):
            ix.search(theirs)
        out = C.c_void_p()
        assert other.lib.bsk_index_build(engine.ctx, theirs.h, C.byref(out)) == L.ERR_ARG and not out.value
        their_hits = other.sets_from_arrays(*tg).index().search(theirs)
        with pytest.raises(S.DeviceError):
            ix.search(mine, reuse=their_hits)
        assert their_hits.h and their_hits.info()["n_queries"] == len(qs[0]) - 1
        buf = np.zeros(len(qs[0]), U64)
        assert engine.lib.bsk_hits_fetch(other.ctx, hits.h, 0, 1, buf.ctypes.data, None, None, 0) == L.ERR_ARG
        check(hits, ref_search(*tg, *qs))
        their_hits.close()
        theirs.close()
    finally:
        other.close()
