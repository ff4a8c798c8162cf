"""dev helper: time the set algebra on device-resident sets (bsk_sets_op / bsk_sets_reduce) against the route a host has without it --
Sets.fetch, NumPy per set, Engine.sets_from_arrays -- on one GPU; best of three, wall time of the call.
P1  10^7 pairs of read-size sets (20 values each, 10 of them shared), all four ops
P2  one pair of 10^7-value sets, half of the values shared (union)
P3  1 000 sets of 1.8 * 10^5 values minus one broadcast set of 10^6 values
R1  union of 2 * 10^7 read sets in groups of two (P1's sets, interleaved)
R2  union of 1 000 groups of 50 sets of 4 * 10^3 values
The host route is timed in its three parts: both fetches and the upload in full, NumPy per pair (per group) on the first `host_items`
pairs of a scenario and scaled to all of them -- the pairs are independent and alike, and 10^7 NumPy calls per op would take minutes.
GB/s: (input values + output values) * 8 bytes over the time -- the bytes an ideal single pass would move.
usage: perf_setops.py [scale=1.0] [host_items=100000] [reps=3]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bio_amd import _lib as L
from bio_amd import sketches as S

SCALE = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
HOST_ITEMS = int(float(sys.argv[2])) if len(sys.argv) > 2 else 100_000
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
U64 = np.uint64
OPS = {"union": (L.SETOP_UNION, np.union1d), "intersect": (L.SETOP_INTERSECT, lambda a, b: np.intersect1d(a, b, assume_unique=True)),
       "diff": (L.SETOP_DIFF, lambda a, b: np.setdiff1d(a, b, assume_unique=True)), "symdiff": (L.SETOP_SYMDIFF, lambda a, b: np.setxor1d(a, b, assume_unique=True))}
eng = S.Engine(0)
rng = np.random.default_rng(1)


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


def host_route(inputs, n_items, per_item):
    """fetch every input, per_item(i, fetched) -> the i-th output set for the first min(n_items, HOST_ITEMS) items, scaled; upload"""
    fetched, t_fetch = timed(lambda: [s.fetch() for s in inputs])
    k = max(1, min(n_items, HOST_ITEMS))
    t = time.perf_counter()
    out = [per_item(i, fetched) for i in range(k)]
    t_numpy = (time.perf_counter() - t) * n_items / k
    # the upload of the whole result: the subset's sets, repeated to the full number of items
    sizes = np.array([len(x) for x in out], np.int64)
    reps = -(-n_items // k)
    offs = np.zeros(n_items + 1, U64)
    offs[1:] = np.cumsum(np.tile(sizes, reps)[:n_items])
    vals = np.tile(np.concatenate(out) if sizes.sum() else np.zeros(0, U64), reps)[: int(offs[-1])].astype(U64)
    up, t_up = timed(lambda: eng.sets_from_arrays(offs, vals))
    up.close()
    return t_fetch + t_numpy + t_up, (t_fetch, t_numpy, t_up, k)


def report(name, dev_s, out, n_in, host):
    n_out = out.info()["n_values"]
    gbs = (n_in + n_out) * 8 / dev_s / 1e9
    total, (tf, tn, tu, k) = host
    print(f"{name:<14} device {dev_s*1e3:10.3f} ms  {gbs:8.1f} GB/s | host {total*1e3:12.1f} ms (fetch {tf*1e3:.0f} + numpy {tn*1e3:.0f} [from {k} items] + upload {tu*1e3:.0f})"
          f" | x{total/dev_s:9.1f} | in {n_in} out {n_out} values; {out.plan()['plan']}", flush=True)


# ---- P1 / R1: pairs of read-size sets ----
N1 = max(1000, int(10_000_000 * SCALE))
v = np.cumsum(rng.integers(1, 1 << 58, size=(N1, 30), dtype=U64), axis=1, dtype=U64)  # 30 ascending values per pair: j % 3 == 0 shared, 1 a's, 2 b's
cols = np.arange(30)
a_vals, b_vals = np.ascontiguousarray(v[:, cols % 3 != 2]), np.ascontiguousarray(v[:, cols % 3 != 1])
del v
offs20 = np.arange(N1 + 1, dtype=U64) * U64(20)
A, B = eng.sets_from_arrays(offs20, a_vals.reshape(-1)), eng.sets_from_arrays(offs20, b_vals.reshape(-1))
for name, (op, fn) in OPS.items():
    out, dt = best(lambda o: A.op(B, op, into=o))
    host = host_route([A, B], N1, lambda i, f: fn(f[0][1][20 * i:20 * i + 20], f[1][1][20 * i:20 * i + 20]))
    report("P1 " + name, dt, out, 40 * N1, host)
    out.close()
A.close()
B.close()
inter = np.concatenate([a_vals, b_vals], axis=1).reshape(-1)  # a0 b0 a1 b1 ...
del a_vals, b_vals
R = eng.sets_from_arrays(np.arange(2 * N1 + 1, dtype=U64) * U64(20), inter)
del inter
go = np.arange(0, 2 * N1 + 1, 2, dtype=U64)
out, dt = best(lambda o: R.reduce(go, 1, into=o))
host = host_route([R], N1, lambda i, f: np.unique(f[0][1][40 * i:40 * i + 40]))
report("R1 pairs", dt, out, 40 * N1, host)
out.close()
R.close()

# ---- P2: one pair of large sets ----
N2 = max(3000, int(15_000_000 * SCALE))
pool = np.unique(rng.integers(0, 1 << 63, size=N2 + N2 // 64, dtype=U64))[:N2]
j = np.arange(len(pool))
a, b = pool[j % 3 != 2], pool[j % 3 != 1]
del pool, j
A, B = eng.sets_from_arrays(np.array([0, len(a)], U64), a), eng.sets_from_arrays(np.array([0, len(b)], U64), b)
out, dt = best(lambda o: A.union(B, into=o))
host = host_route([A, B], 1, lambda i, f: np.union1d(f[0][1], f[1][1]))
report("P2 union", dt, out, len(a) + len(b), host)
out.close()
A.close()
B.close()
del a, b

# ---- P3: many large sets minus one broadcast set ----
n3, s3, m3 = max(10, int(1000 * SCALE)), 180_000, 1_000_000
v = np.cumsum(rng.integers(1, 12, size=(n3, s3), dtype=U64), axis=1, dtype=U64).reshape(-1)  # values below ~1.2 * 10^6
mask = np.cumsum(rng.integers(1, 3, size=m3, dtype=U64), dtype=U64)                          # 10^6 values below ~1.5 * 10^6
A = eng.sets_from_arrays(np.arange(n3 + 1, dtype=U64) * U64(s3), v)
B = eng.sets_from_arrays(np.array([0, m3], U64), mask)
del v
out, dt = best(lambda o: A.difference(B, into=o))
host = host_route([A, B], n3, lambda i, f: np.setdiff1d(f[0][1][s3 * i:s3 * (i + 1)], f[1][1], assume_unique=True))
report("P3 masked", dt, out, n3 * s3 + m3, host)
out.close()
A.close()
B.close()

# ---- R2: groups of 50 sets ----
g4, k4, s4 = max(10, int(1000 * SCALE)), 50, 4000
v = np.cumsum(rng.integers(1, 11, size=(g4 * k4, s4), dtype=U64), axis=1, dtype=U64)  # a group's sets overlap: values below ~2.2 * 10^4 ...
v += (np.arange(g4 * k4, dtype=U64) // U64(k4) << U64(32))[:, None]                    # ... above the group's base
Rs = eng.sets_from_arrays(np.arange(g4 * k4 + 1, dtype=U64) * U64(s4), v.reshape(-1))
del v
go = np.arange(0, g4 * k4 + 1, k4, dtype=U64)
out, dt = best(lambda o: Rs.reduce(go, 1, into=o))
host = host_route([Rs], g4, lambda i, f: np.unique(f[0][1][k4 * s4 * i:k4 * s4 * (i + 1)]))
report("R2 groups", dt, out, g4 * k4 * s4, host)
out.close()
Rs.close()
