"""dev helper: time the selection by a measure (bsk_hits_filter, bsk_hits_top_by) on one GPU; best of `reps` wall times of the call, after
a first call that sizes the arrays, and the spread (worst - best) beside it.
(a) filter("jaccard", 1/2) and top_by(1, "jaccard") of Q rows x 20 hits with totals (DESIGN 3.15's fold shape: 34.2 M hits) against the route
    they replace -- fetch + NumPy + hits_from_arrays -- and the filter against the bytes it must move (12 B per hit in, 12 B per kept hit
    out, the offsets) over the rate a plain device copy of the hits reaches.
(b) top_by(n, "shared") against bsk_hits_top(n), which gathers no payload: n = 1 and n = 100, on the rows of (a) and on R rows of 600 hits.
(c) the global path: one row of 10^4 hits and one of BIG hits, top_by(100, "shared") against bsk_hits_top(100) (its key sort), and a filter
    in front of it.
usage: bench_select.py [Q=1710000] [R=20000] [BIG=1000000] [reps=3]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bio_amd import sketches as S

Q = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_710_000
R = int(float(sys.argv[2])) if len(sys.argv) > 2 else 20_000
BIG = int(float(sys.argv[3])) if len(sys.argv) > 3 else 1_000_000
REPS = int(sys.argv[4]) if len(sys.argv) > 4 else 3
U64, U32 = np.uint64, np.uint32
eng = S.Engine(0)
rng = np.random.default_rng(5)


def timed(fn):
    eng.lib.bsk_ctx_sync(eng.ctx)
    t = time.perf_counter()
    out = fn()
    eng.lib.bsk_ctx_sync(eng.ctx)
    return out, time.perf_counter() - t


def best(fn, reps=REPS):
    ts, out = [], None
    for i in range(reps + 1):  # (the first call sizes the result's arrays and the context's temporaries)
        out, dt = timed(lambda: fn(out))
        if i:
            ts.append(dt)
    return out, min(ts), max(ts) - min(ts)


def rows(nq, per, n_targets):
    """nq rows of `per` ascending targets, shared 1 .. 99, total = shared * 1 .. 4"""
    base = np.sort(rng.choice(max(2 * per, 400), per, replace=False))
    tgt = (rng.integers(0, n_targets - int(base[-1]) - 1, nq, dtype=np.int64)[:, None] + base[None, :]).reshape(-1).astype(U32)
    sh = rng.integers(1, 100, len(tgt)).astype(U32)
    return np.arange(nq + 1, dtype=U64) * U64(per), tgt, sh, sh * rng.integers(1, 5, len(tgt)).astype(U32)


def against_top(hits, what, ns=(1, 100), reps=REPS):
    for n in ns:
        a, ta, sa = best(lambda o: hits.top(n, reuse=o), reps)
        b, tb, sb = best(lambda o: hits.top_by(n, "shared", reuse=o), reps)
        assert all(np.array_equal(x, y) for x, y in zip(a.fetch(), b.fetch())), "top_by by shared differs from top"
        print(f"    {what}, n = {n}: bsk_hits_top {ta*1e3:.2f} ms (spread {sa*1e3:.2f}), bsk_hits_top_by {tb*1e3:.2f} ms (spread {sb*1e3:.2f}): x{tb/ta:.2f} | {b.plan()['plan']}",
              flush=True)
        a.close(), b.close()


if Q:
    offs, tgt, sh, tot = rows(Q, 20, 1_000_000)
    H = len(tgt)
    hits = eng.hits_from_arrays(offs, tgt, sh, tot)
    f, t, sp = best(lambda o: hits.filter("jaccard", (1, 2), reuse=o))
    K = f.info()["n_hits"]
    print(f"(a) filter jaccard >= 1/2 of {Q} rows x 20 hits ({H} hits, totals): {t*1e3:.2f} ms (spread {sp*1e3:.2f}), {K} kept | {f.plan()['plan']}", flush=True)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    po, pt, ps = hits.device()
    _, tc, _ = best(lambda o: (hip.hipMemcpy(ps, pt, H * 4, 3), hip.hipDeviceSynchronize()))
    hip.hipMemcpy(ps, sh.ctypes.data, H * 4, 1)
    rate = 2 * H * 4 / tc
    moved = H * 12 + K * 12 + (Q + 1) * 16
    print(f"    must move {moved/1e9:.2f} GB ({12} B per hit in, {12} B per kept hit out, offsets); a plain copy runs at {rate/1e12:.2f} TB/s -> {moved/rate*1e3:.2f} ms: "
          f"the filter takes x{t/(moved/rate):.1f} of that", flush=True)
    (host, t_fetch) = timed(lambda: hits.fetch() + (hits.fetch_totals(),))
    t1 = time.perf_counter()
    keep = host[2].astype(U64) * U64(2) >= host[3].astype(U64)
    q_of = np.repeat(np.arange(Q), 20)
    ko = np.concatenate([[0], np.cumsum(np.bincount(q_of[keep], minlength=Q))]).astype(U64)
    want = (ko, host[1][keep], host[2][keep], host[3][keep])
    t_model = time.perf_counter() - t1
    (up, t_up) = timed(lambda: eng.hits_from_arrays(*want))
    got = f.fetch()
    assert all(np.array_equal(x, y) for x, y in zip(got, want[:3])) and np.array_equal(f.fetch_totals(), want[3]), "the device's filter differs from the host's"
    host_ms = (t_fetch + t_model + t_up) * 1e3
    print(f"    host route: fetch {t_fetch*1e3:.1f} + NumPy {t_model*1e3:.1f} + hits_from_arrays {t_up*1e3:.1f} = {host_ms:.1f} ms: x{host_ms / (t * 1e3):.1f}", flush=True)
    up.close()
    b1, t, sp = best(lambda o: hits.top_by(1, "jaccard", reuse=o))
    print(f"    top_by(1, jaccard) of the same hits: {t*1e3:.2f} ms (spread {sp*1e3:.2f}) | {b1.plan()['plan']}", flush=True)
    t1 = time.perf_counter()
    frac = host[2].astype(np.float64) / host[3].astype(np.float64)  # (a float key: the host route most callers would write; exact here, shared and total are small)
    order = np.lexsort((host[1], -frac, q_of))
    first = order[::20]
    want = (np.arange(Q + 1, dtype=U64), host[1][first], host[2][first], host[3][first])
    t_model = time.perf_counter() - t1
    (up, t_up) = timed(lambda: eng.hits_from_arrays(want[0], np.zeros(Q, U32), want[2], want[3]))  # (rows of one hit: any target is ascending)
    assert all(np.array_equal(x, y) for x, y in zip(b1.fetch(), want[:3])), "the device's top_by differs from the host's"
    host_ms = (t_fetch + t_model + t_up) * 1e3
    print(f"    host route: fetch {t_fetch*1e3:.1f} + NumPy {t_model*1e3:.1f} + hits_from_arrays {t_up*1e3:.1f} = {host_ms:.1f} ms: x{host_ms / (t * 1e3):.1f}", flush=True)
    print("(b) top_by by shared against bsk_hits_top", flush=True)
    against_top(hits, f"{Q} rows x 20 hits")
    for x in (hits, f, b1, up):
        x.close()
    del host, keep, q_of, frac, order

if R:
    hits = eng.hits_from_arrays(*rows(R, 600, 1_000_000))
    against_top(hits, f"{R} rows x 600 hits")
    hits.close()

if BIG:
    print("(c) the global path: one row", flush=True)
    for c in (10_000, BIG):
        tg = np.sort(rng.choice(4 * c, c, replace=False)).astype(U32)
        s = rng.integers(1, 1000, c).astype(U32)
        hits = eng.hits_from_arrays(np.array([0, c], U64), tg, s, s * U32(2))
        against_top(hits, f"one row of {c} hits", ns=(100,), reps=2)
        f, tf, _ = best(lambda o: hits.filter("shared", 990, reuse=o), 2)
        b, tb, _ = best(lambda o: f.top_by(100, "shared", reuse=o), 2)
        print(f"    filter shared >= 990 first ({f.info()['n_hits']} kept): {tf*1e3:.2f} ms, then top_by(100) {tb*1e3:.2f} ms", flush=True)
        for x in (hits, f, b):
            x.close()
