"""GPU: containment search of sets against a device-resident index (bsk_sets_from_host, bsk_index_*, bsk_hits_*).

Expected hits come from a plain NumPy reference (tests/search_cases.py): value -> targets, pairs counted, the contract's float64
threshold expression."""
import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests.search_cases import collection, ref_search

pytestmark = pytest.mark.gpu
U64 = np.uint64


def check(hits, want):
    o, t, s = hits.fetch()
    assert np.array_equal(o, want[0]), "offsets"
    assert np.array_equal(t, want[1]), "targets"
    assert np.array_equal(s, want[2]), "shared"


def search_and_check(engine, tg, qs, **kw):
    ix = engine.sets_from_arrays(*tg).index()
    q = engine.sets_from_arrays(*qs)
    hits = ix.search(q, **kw)
    check(hits, ref_search(*tg, *qs, kw.get("min_shared", 1), kw.get("min_query_cov", 0.0), kw.get("min_target_cov", 0.0)))
    return ix, hits


# ---- upload ----
def test_upload_round_trip_and_rejections(engine):
    rng = np.random.default_rng(1)
    offs, vals = collection([rng.integers(0, 2**63, rng.integers(0, 50), dtype=U64) for _ in range(300)] + [[0, 2**64 - 1], []])
    s = engine.sets_from_arrays(offs, vals)
    assert s.info() == dict(n_sets=301 + 1, n_values=len(vals))
    o2, v2 = s.fetch()
    assert np.array_equal(o2, offs) and np.array_equal(v2, vals)
    bad = [(np.array([0, 2], U64), np.array([5, 3], U64)),       # not ascending
           (np.array([0, 2], U64), np.array([5, 5], U64)),       # a duplicate
           (np.array([1, 2], U64), np.array([5, 6], U64)),       # offsets[0] != 0
           (np.array([0, 3, 2], U64), np.array([5, 6], U64))]    # offsets decrease
    for o, v in bad:
        with pytest.raises(S.DeviceError):
            engine.sets_from_arrays(o, v)
    with pytest.raises(ValueError):  # offsets[n] != len(values)
        engine.sets_from_arrays(np.array([0, 3], U64), np.array([1, 2], U64))


# ---- exact parity ----
@pytest.mark.parametrize("n_targets,pool,tmax,seed", [(1, 300, 200, 2), (40, 2000, 300, 3), (700, 20000, 120, 4), (70000, 400000, 12, 5)])
def test_parity_random_collections(engine, n_targets, pool, tmax, seed):
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 2**64, pool, dtype=U64)
    p[:2] = [0, 2**64 - 1]
    tsets = [p[rng.integers(0, pool, rng.integers(0, tmax + 1))] for _ in range(n_targets)]
    tsets[0] = np.array([0, 2**64 - 1, p[5]], U64)
    if n_targets > 2:
        tsets[1] = []  # an empty target
    tg = collection(tsets)
    qsets = [p[rng.integers(0, pool, rng.integers(0, 60))] for _ in range(3000)]
    qsets += [[], tsets[0], [0], [2**64 - 1]]  # an empty query, a query equal to a target, the extreme values
    qs = collection(qsets)
    ix, hits = search_and_check(engine, tg, qs)
    inf = ix.info()
    assert inf["n_targets"] == n_targets and inf["n_postings"] == len(tg[1]) and inf["n_distinct"] == len(np.unique(tg[1]))
    assert 1 <= inf["max_bucket"] <= 32 and inf["device_bytes"] > 0
    assert hits.info()["n_queries"] == len(qsets)


# ---- threshold edges ----
def edge_collection():
    """target j = 100 values of its own; query (j, size, s) = s values of target j + size - s values held by no target: the pair
    (query, j) shares exactly s, for every s in 0..size"""
    tg = collection([np.arange(100, dtype=U64) + U64(1000 * j) for j in range(8)])
    qsets = []
    j = 0
    for size in (10, 30, 60, 90, 100):
        for s in range(0, size + 1):
            qsets.append(np.concatenate([np.arange(s, dtype=U64) + U64(1000 * j), np.arange(size - s, dtype=U64) + U64(10**9 + 1000 * j)]))
            j = (j + 1) % 8
    return tg, collection(qsets)


@pytest.mark.parametrize("qc", [0.1, 1 / 3, 0.5, 1.0])
def test_threshold_query_cover(engine, qc):
    tg, qs = edge_collection()
    search_and_check(engine, tg, qs, min_query_cov=qc)


@pytest.mark.parametrize("tc,ms", [(0.1, 1), (0.3, 1), (1.0, 1), (0.0, 7), (0.25, 30), (0.0, 0)])
def test_threshold_target_cover_and_min_shared(engine, tc, ms):
    tg, qs = edge_collection()
    search_and_check(engine, tg, qs, min_target_cov=tc, min_shared=ms)


def test_bad_search_arguments(engine):
    tg, qs = edge_collection()
    ix = engine.sets_from_arrays(*tg).index()
    q = engine.sets_from_arrays(*qs)
    for kw in (dict(min_query_cov=float("nan")), dict(min_query_cov=1.5), dict(min_target_cov=-0.1), dict(min_target_cov=float("inf"))):
        with pytest.raises(S.DeviceError):
            ix.search(q, **kw)


# ---- the large-query path ----
def test_large_path_value_in_every_target(engine):
    """one value X held by each of 5 000 targets, queried by 10 000 queries: every query's postings overflow pass C"""
    X = 2**63 + 12345
    tg = collection([[X, 10**6 + 2 * t, 10**6 + 2 * t + 1] for t in range(5000)])
    qs = collection([[X, 10**12 + q] for q in range(10000)])
    ix = engine.sets_from_arrays(*tg).index()
    hits = ix.search(engine.sets_from_arrays(*qs))
    assert hits.plan()["n_large_queries"] == 10000, hits.plan()
    o, t, s = hits.fetch()
    assert np.array_equal(o, np.arange(10001, dtype=U64) * U64(5000))
    assert np.array_equal(t, np.tile(np.arange(5000, dtype=np.uint32), 10000))
    assert (s == 1).all()
    jac = hits.jaccard()
    assert np.allclose(jac, 1.0 / (2 + 3 - 1)) and np.allclose(hits.containment(), 0.5)


def test_large_path_genome_size_query(engine):
    """a 10^6-value query against 200 overlapping targets (and small queries beside it)"""
    rng = np.random.default_rng(7)
    qv = np.unique(rng.integers(0, 2**64, 1_000_000, dtype=U64))
    tsets = [qv[rng.integers(0, len(qv), rng.integers(1000, 60000))] for _ in range(200)]
    tsets += [rng.integers(0, 2**64, 500, dtype=U64) for _ in range(5)]
    tg = collection(tsets)
    qsets = [qv] + [qv[rng.integers(0, len(qv), 20)] for _ in range(500)]
    qs = collection(qsets)
    for kw in (dict(), dict(min_target_cov=0.5), dict(min_query_cov=0.01)):
        ix, hits = search_and_check(engine, tg, qs, **kw)
        assert hits.plan()["n_large_queries"] >= 1, hits.plan()


# ---- values that are far from uniform ----
def test_kmer_codes_k11_and_shifted_values(engine):
    rng = np.random.default_rng(11)
    seqs = ["".join(rng.choice(list("ACGT"), rng.integers(200, 3000))) for _ in range(300)]
    res = engine.run(engine.batch(seqs), engine.params(L.KMER, 11))
    tsets = res.device_sets()
    assert int(tsets.fetch()[1].max()) < 2**22
    ix = tsets.index()
    assert ix.info()["max_bucket"] <= 32, ix.info()
    tg = tsets.fetch()
    qseqs = [s[a:a + 150] for s in seqs[:100] for a in (0, 40)]
    qres = engine.run(engine.batch(qseqs), engine.params(L.KMER, 11))
    qsets = qres.device_sets()
    hits = ix.search(qsets)
    check(hits, ref_search(*tg, *qsets.fetch()))
    # values i << 32: every raw top-bits bucket distinct, every low word zero
    tg2 = collection([(np.arange(t, t + rng.integers(1, 400), dtype=U64) << U64(32)) for t in range(0, 200000, 500)])
    qs2 = collection([(rng.integers(0, 200400, 30, dtype=U64) << U64(32)) for _ in range(2000)])
    ix2, _ = search_and_check(engine, tg2, qs2)
    assert ix2.info()["max_bucket"] <= 32, ix2.info()


# ---- end to end: genomes -> per-sequence sets -> index; reads -> per-read sets -> search ----
_COMP = np.frombuffer(b"TGCA", np.uint8)
_CODE = np.zeros(256, np.uint8)
_CODE[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4)


@pytest.mark.parametrize("kind,pk,scale", [(L.MINIMIZER, dict(k=21, w=11), 1), (L.SYNCMER, dict(k=31, s=11), 10)])
def test_end_to_end_reads_against_genomes(engine, kind, pk, scale):
    rng = np.random.default_rng(21)
    G, glen, nreads, rlen = 50, 200_000, 20_000, 150
    genomes = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, G * glen)]
    goffs = np.arange(G + 1, dtype=U64) * U64(glen)
    p = engine.params(kind, **pk)
    gsets = engine.run(engine.batch_from_arrays(genomes, goffs), p).device_sets(scale=scale)
    ix = gsets.index()
    tg = gsets.fetch()
    src = rng.integers(0, G, nreads)
    start = rng.integers(0, glen - rlen + 1, nreads)
    idx = (src * glen + start)[:, None] + np.arange(rlen)[None, :]
    reads = genomes[idx]
    rc = rng.random(nreads) < 0.5
    reads[rc] = _COMP[_CODE[reads[rc][:, ::-1]]]
    roffs = np.arange(nreads + 1, dtype=U64) * U64(rlen)
    qsets = engine.run(engine.batch_from_arrays(reads.reshape(-1), roffs), p).device_sets(scale=scale)
    hits = ix.search(qsets)
    qs = qsets.fetch()
    want = ref_search(*tg, *qs)
    check(hits, want)
    o, t, s = want
    best = np.full(nreads, -1)
    nz = np.diff(o) > 0
    for r in np.nonzero(nz)[0]:
        a, b = int(o[r]), int(o[r + 1])
        best[r] = t[a + int(np.argmax(s[a:b]))]
    if scale == 1:
        assert (best == src).mean() >= 0.999
    else:  # about 0.7 syncmers per read survive scale 10: the reads that keep one
        assert nz.sum() > nreads // 4 and (best[nz] == src[nz]).mean() >= 0.999


# ---- re-use of a hits object ----
def test_reuse_equals_fresh(engine):
    rng = np.random.default_rng(31)
    p = rng.integers(0, 2**64, 5000, dtype=U64)
    tg = collection([p[rng.integers(0, 5000, rng.integers(0, 300))] for _ in range(500)])
    ix = engine.sets_from_arrays(*tg).index()
    big = collection([p[rng.integers(0, 5000, rng.integers(0, 80))] for _ in range(6000)] + [p])
    small = collection([p[rng.integers(0, 5000, rng.integers(0, 20))] for _ in range(300)])
    hits = None
    for qs in (big, small, big):
        q = engine.sets_from_arrays(*qs)
        hits = ix.search(q, reuse=hits)
        fresh = ix.search(q)
        a, b = hits.fetch(), fresh.fetch()
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        check(hits, ref_search(*tg, *qs))
