"""dev helper: time the all-pairs comparison (bsk_sets_compare) and bsk_sets_bottom on one GPU; best of three wall times of the call, after
a first call that sizes the arrays.
M1  N sketches of 1 000 values (drawn from a pool of 20 000), all against all, limit 1 000: cells/s, merged values/s (the sum of the
    total matrix over the time) and the rounds figures -- against the route a host has without it: Sets.fetch and a NumPy walk per pair,
    timed on `host_pairs` pairs and scaled to all of them (the pairs are independent and alike).
M2  DESIGN 3.6's S2 sets (2 000 sets of 10^4 values from a pool of 10^6), limit 0 -- against the other device route to the same numbers,
    bsk_index_build + bsk_index_search with min_shared 1 (sparse output), in the same process.
M1w, M2w  the same sets with counts 1..10 through bsk_sets_compare_counted (k_cmp_tile_w), beside bsk_sets_compare on the same values in
    the same process: both times, their ratio, the figures (equal by construction); some cells' dot and min_sum against a NumPy walk.
B1  10^7 read-size sets (20 values) cut to n = 8;  B2  1 000 sets of 2 * 10^5 values cut to n = 1 000: input values/s.
Q1, Q2  bsk_sets_sumsq on B1's and B2's sets with counts 1..10, beside bsk_sets_totals.
usage: perf_compare.py [N=10000] [host_pairs=2000] [reps=3] [scale=1.0 (of B1 / B2 / M2)]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bio_amd import sketches as S

N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000
HOST_PAIRS = int(float(sys.argv[2])) if len(sys.argv) > 2 else 2000
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
SCALE = float(sys.argv[4]) if len(sys.argv) > 4 else 1.0
U64 = np.uint64
eng = S.Engine(0)
rng = np.random.default_rng(2)


def timed(fn):
    eng.lib.bsk_ctx_sync(eng.ctx)
    t = time.perf_counter()
    out = fn()
    eng.lib.bsk_ctx_sync(eng.ctx)
    return out, time.perf_counter() - t


def best(fn):
    b, out = 1e9, None
    for _ in range(REPS + 1):  # (the first call sizes the result's arrays and the context's temporaries)
        out, dt = timed(lambda: fn(out))
        b = min(b, dt)
    return out, b


def walk(a, b, limit):
    u = np.union1d(a, b)
    if limit:
        u = u[:limit]
    return int(np.count_nonzero(np.intersect1d(a, b, assume_unique=True) <= u[-1])) if len(u) else 0, len(u)


def weights(a, ca, b, cb, limit):
    """(dot, min_sum) of one pair: the shared values at or below the last walked value of the union"""
    u = np.union1d(a, b)
    if limit:
        u = u[:limit]
    if len(u) == 0:
        return 0, 0
    _, ia, ib = np.intersect1d(a, b, assume_unique=True, return_indices=True)
    keep = a[ia] <= u[-1]
    x, y = ca[ia][keep].astype(np.int64), cb[ib][keep].astype(np.int64)
    return int((x * y).sum()), int(np.minimum(x, y).sum())


def weighted_row(tag, host, counts, limit, plain_dt, plain_plan, checks):
    """time compare_counted on `sets` with `counts` attached, beside the plain compare's time on the same values"""
    offs = np.concatenate([np.zeros(1, U64), np.cumsum([len(h) for h in host], dtype=U64)])
    wsets = eng.sets_from_arrays_counted(offs, np.concatenate(host), np.concatenate(counts))
    wc, wdt = best(lambda o: wsets.compare_counted(wsets, limit, reuse=o))
    wp = wc.plan()
    assert (wp["tiles"], wp["rounds"], wp["max_rounds"]) == (plain_plan["tiles"], plain_plan["rounds"], plain_plan["max_rounds"])
    rows = min(len(host), 64)
    dot, ms = wc.fetch_weights(0, rows)
    for i, j in zip(rng.integers(0, rows, checks), rng.integers(0, len(host), checks)):
        assert weights(host[i], counts[i], host[j], counts[j], limit) == (int(dot[i, j]), int(ms[i, j])), (tag, i, j)
    print(f"{tag} counts 1..10: compare_counted {wdt*1e3:.1f} ms | compare {plain_dt*1e3:.1f} ms on the same values | ratio {wdt/plain_dt:.3f} | tiles {wp['tiles']} rounds {wp['rounds']}"
          f" most {wp['max_rounds']} (equal) | {checks} cells' dot and min_sum equal to a NumPy walk | {wp['plan']}", flush=True)
    wc.close()
    wsets.close()


# ---- M1 ----
pool = np.unique(rng.integers(0, 1 << 64, 20_200, dtype=U64))[:20_000]
keys = rng.random((N, len(pool)), dtype=np.float32)
vals = np.sort(pool[np.argpartition(keys, 1000, axis=1)[:, :1000]], axis=1)  # 1 000 of the pool per sketch
del keys
sk = eng.sets_from_arrays(np.arange(N + 1, dtype=U64) * U64(1000), vals.reshape(-1))
cmp, dt = best(lambda o: sk.compare(sk, 1000, reuse=o))
p = cmp.plan()
sh, tt = cmp.fetch(0, min(N, 64))
merged = float(tt.astype(np.float64).mean()) * N * N
fetched, t_fetch = timed(lambda: sk.fetch())
pairs = [(int(i), int(j)) for i, j in zip(rng.integers(0, min(N, 64), HOST_PAIRS), rng.integers(0, N, HOST_PAIRS))]
t = time.perf_counter()
for i, j in pairs:
    got = walk(vals[i], vals[j], 1000)
    assert got == (int(sh[i, j]), int(tt[i, j])), (i, j)
t_numpy = (time.perf_counter() - t) * N * N / len(pairs)
print(f"M1 {N} x {N} limit 1000: device {dt*1e3:.1f} ms  {N*N/dt/1e9:.3f} G cells/s  {merged/dt/1e9:.1f} G merged values/s | tiles {p['tiles']} rounds {p['rounds']}"
      f" ({p['rounds']/max(p['tiles'],1):.2f} a tile) most {p['max_rounds']} | host fetch {t_fetch*1e3:.0f} ms + numpy {t_numpy:.0f} s [from {len(pairs)} pairs, all equal to the device's]"
      f" | x{(t_fetch+t_numpy)/dt:.0f} | {p['plan']}", flush=True)
weighted_row(f"M1w {N} x {N} limit 1000", list(vals), list(rng.integers(1, 11, vals.shape).astype(np.uint32)), 1000, dt, p, 200)
cmp.close()
sk.close()
del vals

# ---- M2 ----
N2 = max(32, int(2000 * SCALE))
pool = rng.integers(0, 2**64, 1_000_000, dtype=U64)
sets = [np.unique(pool[rng.integers(0, len(pool), 10_000)]) for _ in range(N2)]
offs = np.zeros(N2 + 1, U64)
offs[1:] = np.cumsum([len(s) for s in sets])
s2 = eng.sets_from_arrays(offs, np.concatenate(sets))
cmp, dt = best(lambda o: s2.compare(s2, 0, reuse=o))
p = cmp.plan()
ix, t_build = timed(lambda: s2.index())
hits, t_search = best(lambda o: ix.search(s2, min_shared=1, reuse=o))
# the same numbers: every listed pair's shared count is the matrix's cell, every other cell is 0
ho, ht, hs = hits.fetch()
dense = np.zeros((N2, N2), np.uint32)
dense[np.repeat(np.arange(N2), np.diff(ho).astype(np.int64)), ht] = hs
assert np.array_equal(dense, cmp.shared)
print(f"M2 {N2} x {N2} sets of 10^4, limit 0: compare {dt*1e3:.1f} ms  {N2*N2/dt/1e6:.1f} M cells/s, rounds {p['rounds']/max(p['tiles'],1):.1f} a tile, most {p['max_rounds']}"
      f" | index build {t_build*1e3:.1f} ms + search {t_search*1e3:.1f} ms, {hits.info()['n_hits']} hits (equal)", flush=True)
weighted_row(f"M2w {N2} x {N2} sets of 10^4, limit 0", sets, [rng.integers(1, 11, len(x)).astype(np.uint32) for x in sets], 0, dt, p, 50)
for x in (cmp, hits, ix, s2):
    x.close()
del sets, dense

# ---- bsk_sets_bottom ----
n1 = max(1000, int(10_000_000 * SCALE))
v = np.cumsum(rng.integers(1, 1 << 58, size=(n1, 20), dtype=U64), axis=1, dtype=U64).reshape(-1)
reads = eng.sets_from_arrays(np.arange(n1 + 1, dtype=U64) * U64(20), v)
out, dt = best(lambda o: reads.bottom(8, into=o))
assert out.info()["n_values"] == 8 * n1
print(f"B1 {n1} sets of 20 values, n = 8: {dt*1e3:.2f} ms  {20*n1/dt/1e9:.2f} G input values/s  {8*n1/dt/1e9:.2f} G kept values/s", flush=True)
out.close()
reads.close()
cnt = rng.integers(1, 11, v.size).astype(np.uint32)
reads = eng.sets_from_arrays_counted(np.arange(n1 + 1, dtype=U64) * U64(20), v, cnt)
q, dt = best(lambda o: reads.sumsq())
_, dt_tot = best(lambda o: reads.totals())
assert np.array_equal(q, (cnt.astype(U64) ** U64(2)).reshape(n1, 20).sum(axis=1, dtype=U64))
print(f"Q1 sumsq of {n1} sets of 20 values: {dt*1e3:.2f} ms  {20*n1/dt/1e9:.2f} G values/s | totals {dt_tot*1e3:.2f} ms", flush=True)
reads.close()
del v, cnt
n2, s2n = max(10, int(1000 * SCALE)), 200_000
v = np.cumsum(rng.integers(1, 1 << 40, size=(n2, s2n), dtype=U64), axis=1, dtype=U64).reshape(-1)
big = eng.sets_from_arrays(np.arange(n2 + 1, dtype=U64) * U64(s2n), v)
out, dt = best(lambda o: big.bottom(1000, into=o))
assert out.info()["n_values"] == 1000 * n2
print(f"B2 {n2} sets of {s2n} values, n = 1000: {dt*1e3:.3f} ms  {n2*s2n/dt/1e9:.1f} G input values/s  {1000*n2/dt/1e9:.2f} G kept values/s", flush=True)
out.close()
big.close()
cnt = rng.integers(1, 11, v.size).astype(np.uint32)
big = eng.sets_from_arrays_counted(np.arange(n2 + 1, dtype=U64) * U64(s2n), v, cnt)
q, dt = best(lambda o: big.sumsq())
_, dt_tot = best(lambda o: big.totals())
assert np.array_equal(q, (cnt.astype(U64) ** U64(2)).reshape(n2, s2n).sum(axis=1, dtype=U64))
print(f"Q2 sumsq of {n2} sets of {s2n} values: {dt*1e3:.3f} ms  {n2*s2n/dt/1e9:.1f} G values/s | totals {dt_tot*1e3:.3f} ms", flush=True)
