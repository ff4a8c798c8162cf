"""dev helper: time the containment search (bsk_index_build / bsk_index_search) and the reduction to the n best hits (bsk_hits_top:
n = 1 on S1's hits, n = 10 on S2's) on two scenarios.
S1, reads against genomes: G synthetic genomes of 1 Mbp as per-sequence minimizer sets (k = 21, w = 11) -> index; the per-read sets of
    R reads of 150 bp cut from them (half reverse-complemented) -> search.
S2, all-vs-all: N sets of 10^4 values drawn from a shared pool of 10^6 -> index, the same sets as queries.
usage: perf_search.py [G=1000] [R=1e7] [N=2000] [reps=3]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bio_amd import _lib as L
from bio_amd import sketches as S

G = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1000
R = int(float(sys.argv[2])) if len(sys.argv) > 2 else 10_000_000
N = int(float(sys.argv[3])) if len(sys.argv) > 3 else 2000
REPS = int(sys.argv[4]) if len(sys.argv) > 4 else 3
eng = S.Engine(0)


def timed(fn):
    eng.lib.bsk_ctx_sync(eng.ctx)
    t = time.perf_counter()
    out = fn()
    eng.lib.bsk_ctx_sync(eng.ctx)
    return out, time.perf_counter() - t


def scenario(name, targets, queries, top_n):
    best_b, ix = 1e9, None
    for _ in range(REPS):
        if ix is not None:
            ix.close()
        ix, dt = timed(targets.index)
        best_b = min(best_b, dt)
    inf = ix.info()
    qv = queries.info()["n_values"]
    best_s, hits = 1e9, None
    for _ in range(REPS):
        hits, dt = timed(lambda: ix.search(queries, reuse=hits))
        best_s = min(best_s, dt)
    hi = hits.info()
    print(f"{name}: index build {best_b*1e3:9.2f} ms ({inf['n_postings']/best_b/1e9:.2f} G postings/s; {inf['n_targets']} targets, "
          f"{inf['n_postings']} postings, {inf['n_distinct']} keys, max bucket {inf['max_bucket']}, device_bytes {inf['device_bytes']})")
    print(f"{name}: search      {best_s*1e3:9.2f} ms ({qv/best_s/1e9:.2f} G query values/s, {hi['n_hits']/best_s/1e9:.3f} G hits/s; "
          f"{hi['n_queries']} queries, {qv} values, {hi['n_hits']} hits; {hits.plan()['plan']})", flush=True)
    if hasattr(eng.lib, "bsk_hits_top"):  # (a library without it: the search figures alone)
        best_t, top = 1e9, None
        for _ in range(REPS + 1):  # (the first call sizes the result's arrays)
            top, dt = timed(lambda: hits.top(top_n, reuse=top))
            best_t = min(best_t, dt)
        print(f"{name}: top {top_n:<2}      {best_t*1e3:9.2f} ms ({100*best_t/best_s:.1f} % of the search; {top.info()['n_hits']} hits kept; {top.plan()['plan']})",
              flush=True)
        top.close()
    hits.close()
    ix.close()


# S1
glen, rlen = 1_000_000, 150
gb = eng.synth(L.ALPHA_DNA, G, glen, 0x5EED0007)
p = eng.params(L.MINIMIZER, 21, w=11)
gsets = eng.run(gb, p).device_sets()
gdata, _ = gb.fetch_ascii(0, G)
rng = np.random.default_rng(1)
src = rng.integers(0, G, R)
start = src * glen + rng.integers(0, glen - rlen + 1, R)
win = np.lib.stride_tricks.sliding_window_view(gdata, rlen)
reads = np.empty((R, rlen), np.uint8)
comp = np.zeros(256, np.uint8)
comp[np.frombuffer(b"ACGT", np.uint8)] = np.frombuffer(b"TGCA", np.uint8)
for a in range(0, R, 1 << 20):
    b = min(R, a + (1 << 20))
    reads[a:b] = win[start[a:b]]
    rc = np.nonzero(rng.random(b - a) < 0.5)[0] + a
    reads[rc] = comp[reads[rc][:, ::-1]]
del win, gdata
roffs = np.arange(R + 1, dtype=np.uint64) * np.uint64(rlen)
rsets = eng.run(eng.batch_from_arrays(reads.reshape(-1), roffs), p).device_sets()
del reads
scenario("S1 reads vs genomes", gsets, rsets, 1)
gsets.close()
rsets.close()

# S2
pool = rng.integers(0, 2**64, 1_000_000, dtype=np.uint64)
sets = [np.unique(pool[rng.integers(0, len(pool), 10_000)]) for _ in range(N)]
offs = np.zeros(N + 1, np.uint64)
offs[1:] = np.cumsum([len(s) for s in sets])
s2 = eng.sets_from_arrays(offs, np.concatenate(sets))
scenario("S2 all-vs-all", s2, s2, 10)
