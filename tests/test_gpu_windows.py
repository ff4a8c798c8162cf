"""GPU: bsk_result_sets_windows against the NumPy model of tests/window_cases.py -- fed with the HOST tuples of BatchResult.fetch, so it
shares no code with the device path.  Every comparison is exact.

Batches (the smallest that reach every layout a result's tuples can lie in):
  mixed    reads of 0, 20 (< k), 150, 250, 400 and 1 000 bases in one batch, cut into a class plan (tails behind the bulk's slabs)
  rows     reads of 200 .. 290 bases: k_minimizer_ring writes a unit's tuples as rows, stride 64 (BSK_REF_ROWS)
  uniform  600 synthetic reads of 150 bases
  wide     a 5 000-base and a 300 000-base sequence: a tiled call, wide first / count arrays instead of reference words
The test asserts that the layouts were really met (bsk_result_plan, bsk_result_class_plan, the reference words, bsk_result_device_wide)."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import window_cases as WC

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
WMAX = 2**31 - 1
# window in {1, 7, 64, 1 000, 2^31 - 1}; step in {0, 1 (with window 7), window / 2, window - 1}; count in {1, 3, 10, 100 000}
PARAMS = [dict(window=1), dict(window=7), dict(window=7, step=1), dict(window=7, step=3), dict(window=7, step=6), dict(window=64), dict(window=64, step=32),
          dict(window=64, step=63), dict(window=1000), dict(window=1000, step=500), dict(window=1000, step=999), dict(window=WMAX), dict(window=WMAX, step=WMAX - 1),
          dict(count=1), dict(count=3), dict(count=10), dict(count=100000)]
KINDS = {"minimizer": lambda e: e.params(L.MINIMIZER, 21, w=11), "syncmer": lambda e: e.params(L.SYNCMER, 31, s=11), "nthash": lambda e: e.params(L.NTHASH, 21),
         "prot_minimizer": lambda e: e.params(L.PROT_MINIMIZER, 9, w=5)}
BATCHES = ("mixed", "rows", "uniform", "wide")
CLASSED = {"BSK_CLASS_FORCE": "1", "BSK_CLASS_MIN": "64"}


@contextlib.contextmanager
def switches(engine, env):
    before = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        engine.reload_options()
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        engine.reload_options()


def d2h(ptr, n, dt):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    a = np.empty(n, dt)
    if n:
        assert hip.hipMemcpy(a.ctypes.data, ptr, a.nbytes, 2) == 0
    return a


def rand_reads(rng, lengths):
    return [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]) for n in lengths]


def make_batch(engine, name):
    rng = np.random.default_rng([20261020, BATCHES.index(name)])
    if name == "mixed":
        return engine.batch(rand_reads(rng, [(0, 20, 150, 250, 400, 1000)[i % 6] for i in range(6 * 70)]))
    if name == "rows":
        return engine.batch(rand_reads(rng, rng.choice((200, 250, 290), 64 * 37 + 29)))
    if name == "uniform":
        return engine.synth(L.ALPHA_DNA, 600, 150, 0x5EED0077)
    return engine.batch(rand_reads(rng, (5000, 300000)))


_RESULTS = {}


def result_of(engine, batch, kind):
    """the result of one batch and kind with its host tuples, made once for the module and left unchanged"""
    key = (batch, kind)
    if key not in _RESULTS:
        with switches(engine, CLASSED if batch == "mixed" else {}):
            b = make_batch(engine, batch)
            res = engine.run(b, KINDS[kind](engine))
        offs, _, h, pos = res.fetch()
        _RESULTS[key] = (b, res, (offs, h, pos))
    return _RESULTS[key][1:]


def fetched(sets):
    o, v = sets.fetch()
    return o, v, (sets.fetch_counts() if sets.counted else None)


def check(engine, res, host, kw, scale, counted, into=None):
    """one call: seq_offsets, offsets, values and counts are the model's; the union of every sequence's windows is the sequence's own set"""
    want = WC.windows_model(*host, scale=scale, **kw)
    ws = res.window_sets(scale=scale, counted=counted, into=into, **kw)
    o, v, c = fetched(ws)
    what = (kw, scale, counted)
    assert np.array_equal(ws.group_offsets, want[0]), what
    assert np.array_equal(o, want[1]) and np.array_equal(v, want[2]), what
    assert ws.counted == counted and (c is None or np.array_equal(c, want[3])), what
    assert ws.info() == dict(n_sets=int(want[0][-1]), n_values=len(want[2])), what
    back = ws.reduce(ws.group_offsets, 1)
    own = res.device_sets(scale=scale)
    assert WC.same(back.fetch(), own.fetch()), what
    assert back.group_offsets is None and own.group_offsets is None
    back.close()
    own.close()
    return ws


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("batch", BATCHES)
def test_every_layout_every_kind(engine, batch, kind):
    res, host = result_of(engine, batch, kind)
    dev = res.device()
    # the layouts this file is about were really met (other pairs of batch and kind land where the planner puts them: a 1 000-base read
    # is tiled for the every-position kinds and for syncmers, so their `mixed` results are wide too)
    if batch == "wide":
        assert dev["wide"] and not dev["refs"] and dev["first"] and dev["count"], res.plan()  # a tiled call: first / count instead of reference words
    if kind == "minimizer" and batch != "wide":
        assert not dev["wide"] and dev["refs"]  # packed reference words
    if batch == "rows" and kind == "minimizer":
        refs = d2h(dev["refs"], res.info()["n_reads"], U64)
        assert "k_minimizer_ring" in res.plan()["kernel"] and ((refs >> U64(63)) != 0).any(), res.plan()  # unit rows, stride 64
    if batch == "mixed" and kind == "minimizer":
        assert res.class_plan()[0] > 0, res.plan()  # a class plan: tails behind the bulk
    assert (host[2] is None) == (kind == "nthash")
    ws = None
    for i, kw in enumerate(PARAMS):  # every parameter set; scale and counted alternate, so each meets every other value of the grid
        ws = check(engine, res, host, kw, 100 if i % 2 else 1, bool((i // 2) % 2), into=ws)
    ws.close()


def test_full_grid_on_the_mixed_minimizer_batch(engine):
    """every parameter set x scale {1, 100} x counted / uncounted; among them windows of more than 64 tuples (the sort) and of at most 64 (k_sets_rows)"""
    res, host = result_of(engine, "mixed", "minimizer")
    for kw in PARAMS:
        for scale in (1, 100):
            for counted in (False, True):
                check(engine, res, host, kw, scale, counted).close()
    # the two paths of sets_build, by construction: the most tuples one window gathers
    p = WC.positions(host[0], host[2])
    seq = np.repeat(np.arange(len(host[0]) - 1), np.diff(host[0].astype(np.int64)))
    assert np.bincount(seq * 16 + p // 64).max() <= 64 and np.bincount(seq).max() > 64  # window=64: small sets; window=2^31-1: a whole 1 000-base read


def test_small_and_large_windows_of_every_position_tuples(engine):
    res, host = result_of(engine, "uniform", "nthash")  # 130 tuples a read: window 64 -> at most 64 a window, window 1 000 -> 130
    for kw in (dict(window=64), dict(window=1000), dict(window=65)):
        check(engine, res, host, kw, 1, False).close()


def test_reuse(engine):
    res, host = result_of(engine, "uniform", "minimizer")
    ws = check(engine, res, host, dict(window=64, step=32), 1, True)  # counted ...
    h0 = ws.h.value
    ws = check(engine, res, host, dict(window=64, step=32), 1, False, into=ws)  # ... re-used uncounted: the counts are gone, the object stays
    assert ws.h.value == h0 and not ws.counted
    per = res.counted_sets()  # a per-sequence object re-used for windows and back
    want = fetched(per)
    check(engine, res, host, dict(count=3), 100, False, into=per)
    assert per.group_offsets is not None
    res.counted_sets(into=per)
    assert per.group_offsets is None and all(np.array_equal(a, b) for a, b in zip(fetched(per), want))
    per.close()
    ws.close()


def test_results_with_no_tuples(engine):
    k = 21
    b = engine.batch([b"ACGT" * 4, b"", b"ACGTACGTAC"])  # all shorter than k
    res = engine.run(b, engine.params(L.NTHASH, k))
    for kw in (dict(window=7), dict(count=3)):
        ws = res.window_sets(**kw)
        assert ws.info() == dict(n_sets=0, n_values=0) and list(ws.group_offsets) == [0, 0, 0, 0]
        ws.close()
    rng = np.random.default_rng(5)
    b2 = engine.batch(rand_reads(rng, (k, 0, k, 150)))  # a sequence whose only tuple sits at position 0
    res2 = engine.run(b2, engine.params(L.NTHASH, k))
    offs, _, h, pos = res2.fetch()
    for kw in (dict(window=1), dict(window=7, step=1), dict(count=10), dict(window=WMAX)):
        ws = check(engine, res2, (offs, h, pos), kw, 1, True)
        assert list(np.diff(ws.group_offsets)[:3]) == [1, 0, 1]
        ws.close()


def test_errors_keep_or_release_the_slot(engine):
    res, host = result_of(engine, "uniform", "minimizer")
    lib, ws = engine.lib, res.window_sets(window=64)
    before, slot = fetched(ws), C.c_void_p(ws.h.value)
    call = lambda ctx, r, wp, scale, s: lib.bsk_result_sets_windows(ctx, r, C.byref(wp) if wp is not None else None, scale, s, None)
    WP = L.WindowParams
    other = S.Engine(0)
    bad = [(engine.ctx, res.h, WP(0, 0, 0, 0), 1), (engine.ctx, res.h, WP(7, 0, 3, 0), 1), (engine.ctx, res.h, WP(7, 8, 0, 0), 1), (engine.ctx, res.h, WP(0, 2, 3, 0), 1),
           (engine.ctx, res.h, WP(2**31, 0, 0, 0), 1), (engine.ctx, res.h, WP(7, 0, 0, 2), 1), (engine.ctx, res.h, WP(7, 0, 0, 0x80000001), 1), (engine.ctx, res.h, WP(7, 0, 0, 0), -1),
           (other.ctx, res.h, WP(7, 0, 0, 0), 1), (engine.ctx, None, WP(7, 0, 0, 0), 1), (engine.ctx, res.h, None, 1), (None, res.h, WP(7, 0, 0, 0), 1)]
    for ctx, r, wp, scale in bad:
        assert call(ctx, r, wp, scale, C.byref(slot)) == L.ERR_ARG and slot.value == ws.h.value, (wp and (wp.window, wp.step, wp.count, wp.flags), scale)
    assert call(engine.ctx, res.h, WP(7, 0, 0, 0), 1, None) == L.ERR_ARG
    foreign = other.sets_from_arrays(np.array([0, 1], U64), np.array([5], U64))  # *sets of another context: refused, and still the caller's
    fslot = C.c_void_p(foreign.h.value)
    assert call(engine.ctx, res.h, WP(7, 0, 0, 0), 1, C.byref(fslot)) == L.ERR_ARG and fslot.value == foreign.h.value
    assert all(np.array_equal(a, b) for a, b in zip(fetched(ws)[:2], before[:2]))  # kept means intact
    foreign.close()
    other.close()
    # 2^32 gathered tuples with the overlap counted: ~200 000 windows of 100 000 tuples each.  Known after a read-back: the slot is released
    wres, _ = result_of(engine, "wide", "nthash")
    with pytest.raises(S.DeviceError, match="unsupported: bsk_result_sets_windows: more than 2\\^32 values"):
        wres.window_sets(window=100000, step=1, into=ws)
    assert ws.h is None
    ws2 = res.window_sets(window=64)  # the context goes on working
    assert np.array_equal(ws2.fetch()[1], before[1])
    ws2.close()


def grid_stats(engine):
    out = (C.c_uint64 * 2)()
    assert engine.lib.bsk_ctx_grid_stats(engine.ctx, out) == L.OK
    return int(out[0]), int(out[1])


def test_capped_grids_take_their_later_trips(engine):
    """600 sequences of 1 000 bases under BSK_GRID_CAP: k_win_count (600 sequences: three workgroups' worth) and k_win_spans (thousands of
    windows) run their stride loops' later trips, the counters show the cut, and the sets are those of the uncapped call"""
    b = engine.synth(L.ALPHA_DNA, 600, 1000, 0x5EED0078)
    res = engine.run(b, engine.params(L.MINIMIZER, 21, w=11))
    offs, _, h, pos = res.fetch()
    for kw, counted in ((dict(window=64, step=32), False), (dict(count=10), True), (dict(window=7), False)):
        plain = fetched(check(engine, res, (offs, h, pos), kw, 1, counted))
        for cap, least in ((1, 2), (3, 1)):  # cap 1: both new grids are cut; cap 3: three workgroups still cover 600 sequences, the windows' grid is cut
            with switches(engine, {"BSK_GRID_CAP": str(cap)}):
                s0, c0 = grid_stats(engine)
                ws = res.window_sets(counted=counted, **kw)
                s1, c1 = grid_stats(engine)
                assert s1 - s0 >= 2 and c1 - c0 >= least, (cap, s1 - s0, c1 - c0)
                got = fetched(ws)
                assert all(np.array_equal(a, b) for a, b in zip(got[:2], plain[:2])) and (not counted or np.array_equal(got[2], plain[2])), (kw, cap)
                ws.close()


def test_end_to_end_chunked_genomes(engine):
    """three 20 000-base genomes -> window_sets(count=10) -> index; 200 reads of 150 bases cut from them -> sets -> search -> fold by genome ->
    top(1): every array is the model's at every step"""
    rng = np.random.default_rng(99)
    genomes = rand_reads(rng, (20000, 20000, 20000))
    p = engine.params(L.MINIMIZER, 21, w=11)
    gres = engine.run(engine.batch(genomes), p)
    go, _, gh, gp = gres.fetch()
    wm = WC.windows_model(go, gh, gp, count=10)
    chunks = gres.window_sets(count=10)
    assert np.array_equal(chunks.group_offsets, wm[0]) and WC.same(chunks.fetch(), wm[1:3]) and list(np.diff(wm[0])) == [10, 10, 10]
    ix = chunks.index()
    reads = []
    for i in range(200):
        g, at = genomes[i % 3], int(rng.integers(0, 20000 - 150))
        reads.append(g[at:at + 150])
    rres = engine.run(engine.batch(reads), p)
    ro, _, rh, _ = rres.fetch()
    qo, qv = WC.sets_per_sequence(ro, rh)
    queries = rres.device_sets()
    assert WC.same(queries.fetch(), (qo, qv))
    hits = ix.search(queries)
    # the search's model: shared values of every query with every chunk
    ho, ht, hs = [0], [], []
    csets = [set(wm[2][int(a):int(b)].tolist()) for a, b in zip(wm[1][:-1], wm[1][1:])]
    for q in range(200):
        qs = set(qv[int(qo[q]):int(qo[q + 1])].tolist())
        for t, cs in enumerate(csets):
            n = len(qs & cs)
            if n:
                ht.append(t)
                hs.append(n)
        ho.append(len(ht))
    assert WC.same(hits.fetch(), (ho, ht, hs))
    folded = hits.fold(chunks.group_offsets)
    fm = WC.fold_model(ho, ht, hs, wm[0])
    assert WC.same(folded.fetch(), fm[:3]) and np.array_equal(folded.members, fm[3])
    best = folded.top(1)
    assert WC.same(best.fetch(), WC.top1_model(*fm[:3])) and best.members is None
    own = np.array([i % 3 for i in range(200)])
    bo, bt, _ = best.fetch()
    assert (np.diff(bo.astype(np.int64)) == 1).all() and np.array_equal(bt, own)  # every read finds its genome
