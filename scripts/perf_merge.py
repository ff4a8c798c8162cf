"""dev helper: time the merged hits (bsk_hits_merge) on one GPU beside the host route they replace and beside a plain device-to-device
copy of the same arrays; median and best of `reps` wall times of the call (a host clock around work that ends in a synchronise), after
a first call that sizes the arrays.
The data: 10^6 query rows against 10^4 targets split by target into 8 shards, 10 hits a row in the whole, 10^7 hits in the 8 parts;
once plain (bsk_index_search) and once with weights (bsk_index_search_counted: dot and min_sum per hit).
  concat   the shards behind one another (the running bases): the result is the search against the whole index
  sort     the same parts with equal bases under BSK_MERGE_ADD: rows interleave, pairs that meet add up
  host     fetch every part, join in NumPy (concatenate, lexsort by row and target), hits_from_arrays -- which carries no weights
  copy     hipMemcpyAsync device-to-device of every part's target, shared (, dot, min_sum) into the result's arrays: the yardstick of
           concat, which moves the same bytes
  transpose  bsk_hits_transpose of the merged hits: the sort-based entry of the same size
usage: perf_merge.py [scale=1.0] [reps=7]   (scale < 1 shrinks the row count)"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bio_amd import sketches as S

SCALE = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
U64, U32 = np.uint64, np.uint32
P, NT = 8, 10_000
eng = S.Engine(0)
rng = np.random.default_rng(11)
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
D2D = 3  # hipMemcpyDeviceToDevice


def timed(fn):
    eng.lib.bsk_ctx_sync(eng.ctx)
    t = time.perf_counter()
    out = fn()
    eng.lib.bsk_ctx_sync(eng.ctx)
    return out, time.perf_counter() - t


def run(fn):
    """-> (the last result, median seconds, best seconds)"""
    out, times = None, []
    for k in range(REPS + 1):  # (the first call sizes the result's arrays and the context's temporaries)
        out, dt = timed(lambda: fn(out))
        if k:
            times.append(dt)
    return out, statistics.median(times), min(times)


def weights_device(h):
    d, m = C.c_void_p(), C.c_void_p()
    eng._chk(eng.lib.bsk_hits_weights_device(h.h, C.byref(d), C.byref(m)))
    return d.value, m.value


def copy_parts(parts, res, weighted):
    """every part's per-hit arrays into the result's, one after another, on the null stream; the caller synchronises"""
    _, rt, rs = res.device()
    rd, rm = weights_device(res) if weighted else (None, None)
    at = 0
    for p in parts:
        n = p.info()["n_hits"]
        _, pt, ps = p.device()
        pairs = [(rt, pt, 4), (rs, ps, 4)]
        if weighted:
            pd, pm = weights_device(p)
            pairs += [(rd, pd, 8), (rm, pm, 8)]
        for dst, src, w in pairs:
            assert hip.hipMemcpyAsync(dst + at * w, src, n * w, D2D, None) == 0
        at += n
    assert hip.hipDeviceSynchronize() == 0
    return res


def host_route(parts, bases):
    o, t, s = zip(*[p.fetch() for p in parts])
    rows = np.concatenate([np.repeat(np.arange(len(x) - 1, dtype=np.int64), np.diff(x).astype(np.int64)) for x in o])
    tt = np.concatenate([x.astype(np.int64) + int(b) for x, b in zip(t, bases)])
    order = np.lexsort((tt, rows))
    oo = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=len(o[0]) - 1))]).astype(U64)
    return eng.hits_from_arrays(oo, tt[order].astype(U32), np.concatenate(s)[order])


def entry(parts, bases, add):
    """the C entry itself into one slot (Engine.merge_hits compares the parts' query_sizes and adds up norms on the host: glue, not the
    merge) -> (the call, the Hits that will own the slot)"""
    arr = (C.c_void_p * len(parts))(*[p.h for p in parts])
    b = np.ascontiguousarray(bases, U64)
    slot = C.c_void_p()

    def call(_):
        eng._chk(eng.lib.bsk_hits_merge(eng.ctx, arr, b.ctypes.data, len(parts), 1 if add else 0, C.byref(slot)))
        return slot

    return call, lambda: bound(slot, parts[0])


def bound(slot, like):
    h = S.Hits(eng)
    h._bind(slot, like.query_sizes, np.zeros(0, U64))
    return h


def report(name, parts, whole, weighted):
    bases = np.concatenate([[0], np.cumsum([len(p.target_sizes) for p in parts[:-1]])]).astype(U64)
    H = sum(p.info()["n_hits"] for p in parts)
    moved = H * (8 + (16 if weighted else 0))  # bytes read = bytes written, per-hit arrays only
    call, own = entry(parts, bases, False)
    _, m_cat, b_cat = run(call)
    cat = own()
    assert all(np.array_equal(x, y) for x, y in zip(cat.fetch(), whole.fetch())), "the merged shards are not the whole search"
    call, own = entry(parts, np.zeros(P, U64), True)
    _, m_srt, b_srt = run(call)
    srt = own()
    tr, m_tr, b_tr = run(lambda o: cat.transpose(NT, reuse=o))
    host, m_host, b_host = run(lambda o: host_route(parts, bases))
    assert all(np.array_equal(x, y) for x, y in zip(host.fetch(), cat.fetch())), "the host route differs"
    plans = cat.plan()["plan"], srt.plan()["plan"]
    _, m_cp, b_cp = run(lambda o: copy_parts(parts, cat, weighted))  # (last: it overwrites cat's arrays with the unmerged order)
    print(f"{name}: {P} parts, {whole.info()['n_queries']} rows, {H} hits, {moved / 1e6:.0f} MB each way", flush=True)
    print(f"  concat {m_cat*1e3:.2f} ms (best {b_cat*1e3:.2f}) | {plans[0]}", flush=True)
    print(f"  sort+ADD {m_srt*1e3:.2f} ms (best {b_srt*1e3:.2f}) | {plans[1]}", flush=True)
    print(f"  d2d copy {m_cp*1e3:.2f} ms (best {b_cp*1e3:.2f}); concat / copy = {m_cat / m_cp:.2f}", flush=True)
    print(f"  transpose of the merged hits {m_tr*1e3:.2f} ms (best {b_tr*1e3:.2f}); concat / transpose = {m_cat / m_tr:.2f}", flush=True)
    print(f"  host route (shared only) {m_host*1e3:.1f} ms (best {b_host*1e3:.1f}); x{m_host / m_cat:.0f} of concat", flush=True)
    for x in (cat, srt, tr, host):
        x.close()


# target t holds the values 1 000 t .. 1 000 t + 999; a query holds one value of each of 10 targets spread over the shards
n = int(1_000_000 * SCALE)
tv = np.arange(NT * 1000, dtype=U64)
tc = rng.integers(1, 5, len(tv)).astype(U32)
first = rng.integers(0, NT // 10, n)
qt = first[:, None] + (NT // 10) * np.arange(10)[None, :]  # ten targets, ascending, a tenth of the targets apart
qv = (qt * 1000 + rng.integers(0, 1000, (n, 10))).astype(U64)
queries = eng.sets_from_arrays_counted(np.arange(n + 1, dtype=U64) * U64(10), qv.reshape(-1), rng.integers(1, 5, n * 10).astype(U32))
cuts = [NT * p // P for p in range(P + 1)]
whole_sets = eng.sets_from_arrays_counted(np.arange(NT + 1, dtype=U64) * U64(1000), tv, tc)
shard_sets = [eng.sets_from_arrays_counted(np.arange(b - a + 1, dtype=U64) * U64(1000), tv[a * 1000:b * 1000], tc[a * 1000:b * 1000]) for a, b in zip(cuts[:-1], cuts[1:])]
whole_ix, ixs = whole_sets.index_counted(), [s.index_counted() for s in shard_sets]
for weighted in (False, True):
    search = (lambda ix: ix.search_counted(queries)) if weighted else (lambda ix: ix.search(queries))
    whole, parts = search(whole_ix), [search(ix) for ix in ixs]
    assert whole.info()["n_hits"] == 10 * n == sum(p.info()["n_hits"] for p in parts) and whole.has_weights() == weighted
    report("with weights" if weighted else "plain", parts, whole, weighted)
    for x in [whole] + parts:
        x.close()
