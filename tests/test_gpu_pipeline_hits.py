"""GPU: the pipeline's hits sink (BSK_SINK_HITS) -- reads in, the best targets of every read out.

The chunks, in record order, must equal ONE big batch through device_sets(scale) -> Index.search -> Hits.top; a small case pins the
whole chain independently of the library: sets from the CPU oracle's minimizers, hits from NumPy (tests/search_cases.ref_search)."""
import ctypes as C
import gzip
import threading

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests.search_cases import collection, ref_search
from tests.test_gpu_hits_top import ref_top

pytestmark = pytest.mark.gpu
U64 = np.uint64
K, W = 21, 11
ACGT = np.frombuffer(b"ACGT", np.uint8)


def all_devices():
    n = C.c_int()
    L.load().bsk_device_count(C.byref(n))
    return list(range(max(1, n.value)))


def make_case(n_reads, seed, n_genomes=20, glen=20_000, with_n=True):
    """genomes (every odd one repeats half of its neighbour, so reads from there have two targets) and reads of 150 bases cut from
    them with a few bases changed; every 40th read shorter than k, every 50th with an N, every 30th random"""
    rng = np.random.default_rng(seed)
    g = ACGT[rng.integers(0, 4, (n_genomes, glen))]
    g[1::2, : glen // 2] = g[0::2, : glen // 2]
    goffs = np.arange(n_genomes + 1, dtype=U64) * U64(glen)
    src, at = rng.integers(0, n_genomes, n_reads), rng.integers(0, glen - 150, n_reads)
    reads = g[src[:, None], at[:, None] + np.arange(150)[None, :]].copy()
    mut = rng.integers(0, 150, (n_reads, 2))
    reads[np.arange(n_reads)[:, None], mut] = ACGT[rng.integers(0, 4, (n_reads, 2))]
    reads[29::30] = ACGT[rng.integers(0, 4, reads[29::30].shape)]
    if with_n:
        reads[49::50, 70] = ord("N")
    lens = np.full(n_reads, 150, np.int64)
    lens[39::40] = rng.integers(1, K, len(lens[39::40]))
    keep = np.arange(150)[None, :] < lens[:, None]
    roffs = np.zeros(n_reads + 1, U64)
    roffs[1:] = np.cumsum(lens)
    return (g.reshape(-1).copy(), goffs), (reads[keep].copy(), roffs)


def build_index(engine, genomes, p, scale):
    sets = engine.run(engine.batch_from_arrays(*genomes), p).device_sets(scale=scale)
    ix = sets.index()
    sets.close()
    return ix


def one_batch(engine, ix, reads, p, scale, top_n, **kw):
    """the same reads as ONE batch: sets at the scale, searched, reduced -> (offsets, target, shared, status)"""
    whole = engine.run(engine.batch_from_arrays(*reads), p)
    status = whole.fetch()[1]
    sets = whole.device_sets(scale=scale)
    hits = ix.search(sets, **kw)
    out = hits.top(top_n) if top_n else hits
    o, t, s = out.fetch()
    return o, t.copy(), s.copy(), status.copy()


def collect(pl):
    out = []
    for c in pl.chunks():
        assert c.sink == L.SINK_HITS and c.hash is None and c.pos is None
        assert len(c.offsets) == c.n_records + 1 and int(c.offsets[-1]) == c.n_values == len(c.target) == len(c.shared)
        out.append(dict(seq=c.sequence, first=c.first_record, n=c.n_records, src=c.source_index, offsets=c.offsets.astype(U64).copy(), status=c.status.copy(),
                        target=c.target.copy(), shared=c.shared.copy(), link=c.link_bytes, n_values=c.n_values, checksum=c.checksum, narrow=c.offsets.dtype == np.uint32,
                        device=c.device))
    return out


def assert_equals_batch(chunks, want, n_records, first_of_source=True):
    """chunks in record order whose concatenation is the one batch's result"""
    o, t, s, st = want
    assert [c["seq"] for c in chunks] == list(range(len(chunks)))
    at = 0
    for c in chunks:
        m = c["n"]
        if first_of_source:
            assert c["first"] == at
        a, b = int(o[at]), int(o[at + m])
        assert np.array_equal(c["offsets"], o[at:at + m + 1] - o[at]), c["seq"]
        assert np.array_equal(c["target"], t[a:b]), c["seq"]
        assert np.array_equal(c["shared"], s[a:b]), c["seq"]
        assert np.array_equal(c["status"], st[at:at + m]), c["seq"]
        assert c["narrow"] and c["link"] == 5 * m + 8 * (b - a) and c["n_values"] == b - a  # per record a u32 offset and a status byte, per hit two u32
        at += m
    assert at == n_records


@pytest.mark.parametrize("devices", ["one", "twice", "all"])
@pytest.mark.parametrize("scale", [1, 100])
def test_hits_sink_from_memory_equals_one_batch(engine, devices, scale):
    devs = {"one": [0], "twice": [0, 0], "all": all_devices()}[devices]
    n = 24_000
    genomes, reads = make_case(n, 31 + scale)
    p = engine.params(L.MINIMIZER, K, w=W)
    ix = build_index(engine, genomes, p, scale)
    for top_n, kw in ((0, {}), (1, {}), (3, {}), (1, dict(min_shared=2, min_query_cov=0.2, min_target_cov=0.0001)), (0, dict(min_shared=3))):
        want = one_batch(engine, ix, reads, p, scale, top_n, **kw)
        with S.Engine.pipeline_open(p, data=reads[0], offsets=reads[1], devices=devs, n_streams=2, chunk_records=2501, sink=L.SINK_HITS, sets_scale=scale,
                                    alphabet=L.ALPHA_DNA, host_checksum=True, search=ix, top_n=top_n, **kw) as pl:
            chunks = collect(pl)
        st = pl.stats
        assert len(chunks) == -(-n // 2501) and {c["device"] for c in chunks} <= set(devs)
        assert_equals_batch(chunks, want, n)
        for c in chunks:
            assert c["checksum"] == int(c["target"].astype(U64).sum() + c["shared"].astype(U64).sum())
        assert st["records"] == n and st["chunks"] == len(chunks) and st["n_streams"] == 2 * len(devs)
        assert st["checksum"] == sum(c["checksum"] for c in chunks) % (1 << 64)
        o, t, s, status = want
        cnt = np.diff(o).astype(np.int64)
        short = (status & L.ST_CODE_MASK) == L.ST_SHORT
        assert short.sum() == n // 40 and (cnt[short] == 0).all()  # reads shorter than k: flagged, no hits
        if top_n:
            assert cnt.max() <= top_n
        if not kw and scale == 1:
            assert (cnt > 0).mean() > 0.9 and (status & L.ST_HAS_NON_ACGT).astype(bool).sum() >= n // 100
            if top_n == 0:
                assert (cnt >= 2).mean() > 0.3  # reads of the shared halves have two targets
    ix.close()


def write_fastq(path, data, offs, gz):
    opener = gzip.open if gz else open
    with opener(path, "wb") as f:
        for i in range(len(offs) - 1):
            s = data[int(offs[i]):int(offs[i + 1])].tobytes()
            f.write(b"@r%d x\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))


def test_hits_sink_from_files(engine, tmp_path):
    """a plain file (the block-parallel reader, host-packed chunks), a gzip file (the serial reader), and the two in order"""
    n = 12_000
    genomes, reads = make_case(n, 37)
    p = engine.params(L.MINIMIZER, K, w=W)
    ix = build_index(engine, genomes, p, 1)
    want = one_batch(engine, ix, reads, p, 1, 2)
    paths = []
    for gz in (False, True):
        path = str(tmp_path / ("r.fq.gz" if gz else "r.fq"))
        write_fastq(path, reads[0], reads[1], gz)
        paths.append(path)
    for path in paths:
        with S.Engine.pipeline_open(p, paths=[path], devices=[0], n_streams=3, chunk_records=1700, sink=L.SINK_HITS, search=ix, top_n=2) as pl:
            chunks = collect(pl)
        assert_equals_batch(chunks, want, n)
    with S.Engine.pipeline_open(p, paths=paths, devices=[0, 0], n_streams=2, chunk_records=5000, sink=L.SINK_HITS, search=ix, top_n=2, n_readers=1) as pl:
        chunks = collect(pl)
    assert [c["src"] for c in chunks] == sorted(c["src"] for c in chunks) and {c["src"] for c in chunks} == {0, 1}
    for src in (0, 1):  # file 0's chunks, then file 1's, every file counted from its own record 0
        mine = [dict(c, seq=i) for i, c in enumerate(c for c in chunks if c["src"] == src)]
        assert_equals_batch(mine, want, n)
    ix.close()


@pytest.mark.parametrize("top_n", [0, 1, 3])
def test_small_case_against_oracle_sets_and_numpy(engine, oracle, top_n):
    """1 500 reads against 20 targets, nothing of the library on the expected side: sets = the distinct hashes of the oracle's
    minimizers, hits = ref_search, order = lexsort((target, -shared)) cut at top_n"""
    n = 1500
    genomes, reads = make_case(n, 41, glen=4000, with_n=False)
    p = engine.params(L.MINIMIZER, K, w=W)

    def oracle_sets(data, offs):
        out = []
        for i in range(len(offs) - 1):
            s = data[int(offs[i]):int(offs[i + 1])].tobytes()
            out.append(oracle.minimizer(s, K, W, closed=True)[0] if len(s) >= K else [])
        return collection(out)

    tg, qs = oracle_sets(*genomes), oracle_sets(*reads)
    assert len(tg[0]) - 1 == 20 and len(qs[0]) - 1 == n
    want = ref_search(*tg, *qs, 2, 0.0, 0.0)
    if top_n:
        want = ref_top(*want, top_n)
    ix = engine.sets_from_arrays(*tg).index()  # (the index too is made of the oracle's sets)
    with S.Engine.pipeline_open(p, data=reads[0], offsets=reads[1], devices=[0, 0], n_streams=1, chunk_records=256, sink=L.SINK_HITS, alphabet=L.ALPHA_DNA,
                                search=ix, top_n=top_n, min_shared=2) as pl:
        chunks = collect(pl)
    o = np.concatenate([[0]] + [c["offsets"][1:].astype(np.int64) + sum(int(d["n_values"]) for d in chunks[:i]) for i, c in enumerate(chunks)]).astype(U64)
    assert np.array_equal(o, want[0])
    assert np.array_equal(np.concatenate([c["target"] for c in chunks]), want[1])
    assert np.array_equal(np.concatenate([c["shared"] for c in chunks]), want[2])
    cnt = np.diff(want[0])
    assert (cnt > 0).mean() > 0.85 and (cnt[39::40] == 0).all()
    for c in chunks:
        assert (((c["status"] & L.ST_CODE_MASK) == L.ST_SHORT) == (np.arange(c["first"], c["first"] + c["n"]) % 40 == 39)).all()
    ix.close()


def _free0():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    f, t = C.c_size_t(), C.c_size_t()
    assert hip.hipSetDevice(0) == 0 and hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
    return f.value


def test_early_close_and_cancel_leave_nothing_attached(engine):
    """a run closed after its first chunk and a run cancelled from another thread: the index is the caller's alone afterwards (its
    release frees the device arrays), and a second run over a fresh index works"""
    n = 20_000
    genomes, reads = make_case(n, 43, glen=400_000)
    p = engine.params(L.MINIMIZER, K, w=W)
    for how in ("close", "cancel"):
        ix = build_index(engine, genomes, p, 1)
        dev_bytes = ix.info()["device_bytes"]
        assert dev_bytes > 16 << 20
        pl = S.Engine.pipeline_open(p, data=reads[0], offsets=reads[1], devices=[0, 0], n_streams=2, chunk_records=500, sink=L.SINK_HITS, alphabet=L.ALPHA_DNA,
                                    repeat=500, search=ix, top_n=1)
        if how == "close":
            first = pl.next()
            assert first.sequence == 0 and first.n_records == 500 and first.target is not None
        else:
            got, out = [], {}

            def consumer():
                try:
                    for c in pl.chunks():
                        got.append(c.sequence)
                except S.PipelineStopped:
                    out["stopped"] = True

            t = threading.Thread(target=consumer)
            t.start()
            while len(got) < 3:
                pass
            pl.cancel()
            t.join(60)
            assert not t.is_alive() and out.get("stopped") and got == list(range(len(got)))
        st = pl.close()
        assert st["seconds"] > 0
        engine.sync()
        held = _free0()
        ix.close()
        assert _free0() - held > dev_bytes * 0.8, (how, "the pipeline's handles are gone: the caller's release frees the arrays")
    ix = build_index(engine, genomes, p, 1)
    want = one_batch(engine, ix, reads, p, 1, 1)
    with S.Engine.pipeline_open(p, data=reads[0], offsets=reads[1], devices=[0], n_streams=2, chunk_records=3000, sink=L.SINK_HITS, alphabet=L.ALPHA_DNA,
                                search=ix, top_n=1) as pl:
        chunks = collect(pl)
    assert_equals_batch(chunks, want, n)
    ix.close()


def test_plain_open_refuses_the_hits_sink_and_other_sinks_have_no_hits(engine):
    genomes, reads = make_case(2000, 47)
    p = engine.params(L.MINIMIZER, K, w=W)
    lib = L.load()
    dev = (C.c_int * 1)(0)
    cfg = L.PipelineConfig(dev, 1, 1, 500, L.SINK_HITS, 1, L.ALPHA_DNA, 0, 0, 0)
    h = C.c_void_p(1)
    assert lib.bsk_pipeline_open_memory(C.byref(cfg), reads[0].ctypes.data, reads[1].ctypes.data, 2000, 1, C.byref(p), C.byref(h)) == L.ERR_ARG and h.value is None
    with pytest.raises(S.DeviceError):
        S.Engine.pipeline_open(p, data=reads[0], offsets=reads[1], devices=[0], sink=L.SINK_HITS, alphabet=L.ALPHA_DNA)
    ix = build_index(engine, genomes, p, 1)
    with pytest.raises(S.DeviceError):  # the search entries take the hits sink only
        S.Engine.pipeline_open(p, data=reads[0], offsets=reads[1], devices=[0], sink=L.SINK_SETS, alphabet=L.ALPHA_DNA, search=ix)
    with S.Engine.pipeline_open(p, data=reads[0], offsets=reads[1], devices=[0], chunk_records=500, sink=L.SINK_SETS, alphabet=L.ALPHA_DNA) as pl:
        c = pl.next()
        assert c.target is None and c.shared is None
        t, s = C.c_void_p(), C.c_void_p()
        assert lib.bsk_chunk_hits(pl._held, C.byref(t), C.byref(s)) == L.ERR_ARG and t.value is None
    ix.close()
