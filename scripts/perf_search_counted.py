"""dev helper: time the weighted containment search (bsk_index_build_counted / bsk_index_search_counted) against the unweighted search on
the same operands and against the routes it replaces.  Every figure is the median of REPS calls between two synchronisations of the
context's stream, with the smallest and the largest beside it.
  reads:  G synthetic genomes of 1 Mbp as counted per-sequence minimizer sets (k = 21, w = 11) -> index; the counted per-read sets of R
          reads of 150 bp cut from them -> search.  The small path: k_sw_row.
  sample: T sets of V values drawn from a pool with seeded counts -> index; ONE counted set of Q values of the same pool -> search.
          The large path: k_sw_chunk and its atomics.
  routes: (only in mode "all") a panel of N counted sets of M values against itself by bsk_sets_neighbors_counted, and one sample
          against the sets one by one by bsk_sets_op_counted KEEP + bsk_sets_totals, each beside the search that gives the same numbers.
Mode "search" times bsk_index_search alone on both shapes and needs no entry of the weighted search: run it with BSK_LIB pointing at
another build of the library (and BSK_LIB_PARTIAL=1 when that build lacks newer entries) to compare two builds on the same operands.
usage: perf_search_counted.py [all|search] [G=1000] [R=1e6] [T=1e4] [V=2000] [Q=1e6] [N=4000] [M=1000] [reps=7]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bio_amd import _lib as L
from bio_amd import sketches as S

A = sys.argv[1:]
MODE = A[0] if A else "all"
G, R, T, V, Q, N, M = (int(float(A[i])) if len(A) > i else d for i, d in ((1, 1000), (2, 1_000_000), (3, 10_000), (4, 2000), (5, 1_000_000), (6, 4000), (7, 1000)))
REPS = int(A[8]) if len(A) > 8 else 7
HBM = 8.0e12  # bytes/s: the MI355X's peak memory bandwidth, for the traffic floor
eng = S.Engine(0)
OUT = {}


def timed(fn, reps=REPS):
    """-> (last result, (median, min, max) seconds); one untimed call first"""
    out = fn()
    ts = []
    for _ in range(reps):
        eng.lib.bsk_ctx_sync(eng.ctx)
        t = time.perf_counter()
        out = fn()
        eng.lib.bsk_ctx_sync(eng.ctx)
        ts.append(time.perf_counter() - t)
    return out, (float(np.median(ts)), min(ts), max(ts))


def rebuilt(build):
    """build() with the previous call's index closed first"""
    hold = [None]

    def f():
        if hold[0] is not None:
            hold[0].close()
        hold[0] = build()
        return hold[0]

    return f


def entry(name, ix, queries):
    """the C entry itself into one re-used slot: the Python mirror's own fetches (the queries' offsets, the norms) stay out of the time"""
    slot, sp, fn = C.c_void_p(), L.SearchParams(1, 0, 0.0, 0.0), getattr(eng.lib, name)

    def f():
        rc = fn(eng.ctx, ix.h, queries.h, C.byref(sp), C.byref(slot))
        assert rc == L.OK, rc

    return f


def ms(t):
    return "%9.3f ms (%.3f .. %.3f)" % (t[0] * 1e3, t[1] * 1e3, t[2] * 1e3)


def rows(rng, n, size, pool):
    """n sets of `size` distinct draws from pool -> (offsets, values), every set ascending"""
    v = np.sort(pool[rng.integers(0, len(pool), (n, size))], axis=1)
    keep = np.ones(v.shape, bool)
    keep[:, 1:] = v[:, 1:] != v[:, :-1]
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum(keep.sum(1))
    return offs, v[keep]


def counts(rng, n):
    """abundances: mostly small, a heavy tail"""
    return np.minimum(rng.zipf(1.6, n), 1 << 20).astype(np.uint32)


def shape(name, targets, queries):
    """the unweighted and the weighted search of `queries` against an index of `targets`, both counted"""
    res = {}
    if MODE == "all":
        ix, tb = timed(rebuilt(targets.index), 3)
        ix.close()
        ix, tbc = timed(rebuilt(targets.index_counted), 3)
        res.update(build=tb, build_counted=tbc, build_ratio=tbc[0] / tb[0])
        print(f"{name}: index build          {ms(tb)}\n{name}: index build counted  {ms(tbc)}   ratio {tbc[0] / tb[0]:.2f}")
    else:
        ix = targets.index()
    inf, qv = ix.info(), queries.info()["n_values"]
    plain, weighted = entry("bsk_index_search", ix, queries), entry("bsk_index_search_counted", ix, queries) if MODE == "all" else None
    _, ts = timed(plain)
    h = ix.search(queries)
    res.update(search=ts, n_hits=h.info()["n_hits"], n_postings=inf["n_postings"], query_values=qv)
    print(f"{name}: search               {ms(ts)}   {h.info()['n_queries']} queries, {qv} values, {h.info()['n_hits']} hits; {inf['n_targets']} targets, {inf['n_postings']} postings")
    if MODE == "all":
        visited = int(h.shared.astype(np.uint64).sum())  # every posting of every query value lands in exactly one pair's shared count
        _, tw = timed(weighted)
        hw = ix.search_counted(queries)
        assert np.array_equal(hw.offsets, h.offsets) and np.array_equal(hw.target, h.target) and np.array_equal(hw.shared, h.shared)
        own = tw[0] - ts[0]
        floor_bytes = visited * 8 + qv * 12 + res["n_hits"] * 20  # target + count per posting; range + count per query value; the row's targets read, dot and min_sum written
        res.update(search_counted=tw, ratio=tw[0] / ts[0], pass_own=own, postings_visited=visited, floor_bytes=floor_bytes, floor_s=floor_bytes / HBM,
                   over_floor=own / (floor_bytes / HBM), plan=hw.plan()["plan"])
        print(f"{name}: search counted       {ms(tw)}   ratio {tw[0] / ts[0]:.3f}; the pass alone {own * 1e3:.3f} ms; {visited} postings visited, traffic floor "
              f"{floor_bytes / 1e6:.1f} MB = {floor_bytes / HBM * 1e6:.1f} us at {HBM / 1e12:.0f} TB/s: the pass takes {own / (floor_bytes / HBM):.1f} x that\n{name}: {hw.plan()['plan']}", flush=True)
    OUT[name] = res
    return ix


# ---- reads ----
glen, rlen = 1_000_000, 150
gb = eng.synth(L.ALPHA_DNA, G, glen, 0x5EED0007)
p = eng.params(L.MINIMIZER, 21, w=11)
gsets = eng.run(gb, p).counted_sets()
gdata, _ = gb.fetch_ascii(0, G)
rng = np.random.default_rng(1)
start = rng.integers(0, G, R) * glen + rng.integers(0, glen - rlen + 1, R)
reads = np.lib.stride_tricks.sliding_window_view(gdata, rlen)[start]
del gdata
rb = eng.batch_from_arrays(reads.reshape(-1), np.arange(R + 1, dtype=np.uint64) * rlen)
rsets = eng.run(rb, p).counted_sets()
del reads
shape("reads", gsets, rsets).close()
for x in (rsets, gsets, rb, gb):
    x.close()

# ---- sample ----
rng = np.random.default_rng(2)
pool = rng.integers(0, 2**64, 4 * Q, dtype=np.uint64)
to, tv = rows(rng, T, V, pool)
targets = eng.sets_from_arrays_counted(to, tv, counts(rng, len(tv)))
so, sv = rows(rng, 1, Q, pool)
sample = eng.sets_from_arrays_counted(so, sv, counts(rng, len(sv)))
shape("sample", targets, sample).close()

if MODE == "all":
    # ---- routes: KEEP + totals, one merge per target, against the search on an index without counts (dot = the sample's mass in the target) ----
    T2 = min(T, 1000)
    small = eng.sets_from_arrays_counted(to[:T2 + 1], tv[:int(to[T2])], counts(rng, int(to[T2])))
    plain_ix = eng.sets_from_arrays(to[:T2 + 1], tv[:int(to[T2])]).index()
    hold = [None, None]

    def keep_totals():
        hold[0] = sample.keep(small, into=hold[0])
        return hold[0].totals()

    mass, tk = timed(keep_totals)
    _, tsr = timed(entry("bsk_index_search_counted", plain_ix, sample))
    h = plain_ix.search_counted(sample)
    got = np.zeros(T2, np.uint64)
    got[h.target] = h.dot
    assert np.array_equal(got, mass)
    print(f"routes: one sample of {len(sv)} values against {T2} targets: KEEP + totals {ms(tk)}; search_counted {ms(tsr)}; ratio {tsr[0] / tk[0]:.3f}")
    OUT["keep_totals"] = dict(keep_totals=tk, search_counted=tsr, ratio=tsr[0] / tk[0], targets=T2)
    # ---- routes: a panel against itself ----
    po, pv = rows(rng, N, M, pool[:1000 * M])
    panel = eng.sets_from_arrays_counted(po, pv, counts(rng, len(pv)))
    pix = panel.index_counted()
    hold = [None, None]

    def by_neighbors():
        hold[0] = panel.neighbors_counted(panel, 0, reuse=hold[0])
        return hold[0]

    nb, tn = timed(by_neighbors, 3)
    _, tp = timed(entry("bsk_index_search_counted", pix, panel))
    h = pix.search_counted(panel)
    assert np.array_equal(nb.offsets, h.offsets) and np.array_equal(nb.target, h.target) and np.array_equal(nb.dot, h.dot) and np.array_equal(nb.min_sum, h.min_sum)
    print(f"routes: a panel of {N} sets of {M} values against itself, {h.info()['n_hits']} pairs of {N * N}: neighbors_counted {ms(tn)}; search_counted {ms(tp)}; "
          f"ratio {tp[0] / tn[0]:.3f}")
    OUT["panel"] = dict(neighbors_counted=tn, search_counted=tp, ratio=tp[0] / tn[0], sets=N, values=M, pairs=h.info()["n_hits"])
print(json.dumps(dict(mode=MODE, lib=L.SO_PATH, reps=REPS, results=OUT)))
