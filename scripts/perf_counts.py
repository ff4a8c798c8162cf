"""dev helper: time the counted sets (bsk_result_sets_counted, bsk_sets_op_counted, bsk_sets_filter_counts, bsk_sets_totals) against the
uncounted entries and against the route a host had before -- fetch every tuple, np.unique(return_counts=True) -- on one GPU; best of
three after a sizing call, wall time of the call with its read-backs.
C1  10^7 reads of 150 bp, minimizer k=21 w=11: whole-batch counted sets at scale 1 and 100 | bsk_result_sets | fetch + np.unique
C2  the same reads per sequence: counted (general path) | bsk_result_sets (k_sets_rows) | bsk_result_sets on the general path
C3  ADD of two 10^7-value counted sets, half of the values shared | bsk_sets_op union
C4  KEEP of one 10^6-value sample against 1 000 sets of 1.8 * 10^5 values (a broadcast), then bsk_sets_totals | fetch + np.isin per set
C5  filter_counts(min_count=2) on C1's result | boolean mask on the host
usage: perf_counts.py [scale=1.0] [reps=3] [base]
base: only the uncounted entries -- what a library without the counted ones (BSK_LIB=... BSK_LIB_PARTIAL=1) can run, for the same-box
comparison of bsk_result_sets and bsk_sets_op before and after."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bio_amd import _lib as L
from bio_amd import sketches as S

SCALE = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
BASE = "base" in sys.argv[3:]
U64, U32 = np.uint64, np.uint32
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


def row(name, **ms):
    print(f"{name:<34} " + "  ".join(f"{k} {v * 1e3:10.3f} ms" if isinstance(v, float) else f"{k} {v}" for k, v in ms.items()), flush=True)


def reuse_plain(res, whole, scale):
    def call(out):
        h = out.h if out is not None else S.C.c_void_p()
        eng._chk(eng.lib.bsk_result_sets_reuse(eng.ctx, res.h, int(whole), scale, S.C.byref(h)))
        if out is None:
            return S.Sets(eng, h)
        out.h = h
        return out
    return call


# ---- C1 / C2 / C5 ----
N1 = max(1000, int(10_000_000 * SCALE))
batch = eng.synth(L.ALPHA_DNA, N1, 150, 0x5EED0011)
res = eng.run(batch, eng.params(L.MINIMIZER, 21, w=11))
n_tuples = res.info()["n_tuples"]
print(f"{N1} reads of 150 bp, k=21 w=11: {n_tuples} tuples", flush=True)
for scale in (1, 100):
    plain, t_plain = best(reuse_plain(res, True, scale))
    if BASE:
        row(f"C1 whole batch scale {scale}", uncounted=t_plain, values=plain.info()["n_values"])
        plain.close()
        continue
    counted, t_counted = best(lambda o: res.counted_sets(whole_batch=True, scale=scale, into=o))
    row(f"C1 whole batch scale {scale}", counted=t_counted, uncounted=t_plain, ratio=f"{t_counted / t_plain:.2f}", values=counted.info()["n_values"])
    if True:
        def host():
            _, _, h, _ = res.fetch()
            h = h[h <= U64((2**64 - 1) // scale)] if scale > 1 else h
            return np.unique(h, return_counts=True)
        (hv, hc), t_host = timed(host)
        assert np.array_equal(hv, counted.fetch()[1]) and np.array_equal(hc.astype(U32), counted.fetch_counts())
        row(f"C1 host route scale {scale}", host=t_host, speedup=f"x{t_host / t_counted:.0f}")
        del hv, hc
    if scale == 1:
        out, t_f = best(lambda o: counted.filter_counts(2, into=o))
        c = counted.fetch_counts()
        v = counted.fetch()[1]
        _, t_fetch = timed(lambda: (counted.fetch(), counted.fetch_counts()))
        t = time.perf_counter()
        keep = c >= 2
        hv, hc = v[keep], c[keep]
        t_mask = time.perf_counter() - t
        assert np.array_equal(hv, out.fetch()[1]) and np.array_equal(hc, out.fetch_counts())
        row("C5 filter_counts(min_count=2)", device=t_f, host=t_fetch + t_mask, speedup=f"x{(t_fetch + t_mask) / t_f:.0f}", kept=out.info()["n_values"])
        out.close()
        del c, v, hv, hc
    plain.close()
    counted.close()

plain, t_rows = best(reuse_plain(res, False, 1))
row("C2 per sequence, k_sets_rows", uncounted=t_rows, values=plain.info()["n_values"])
plain.close()
os.environ["BSK_SETS_NO_SMALL"] = "1"
eng.reload_options()
plain, t_general = best(reuse_plain(res, False, 1))
del os.environ["BSK_SETS_NO_SMALL"]
eng.reload_options()
row("C2 per sequence, general path", uncounted=t_general)
plain.close()
if not BASE:
    counted, t_counted = best(lambda o: res.counted_sets(whole_batch=False, scale=1, into=o))
    row("C2 per sequence, counted", counted=t_counted, vs_rows=f"{t_counted / t_rows:.2f}", vs_general=f"{t_counted / t_general:.2f}")
    counted.close()
res.close()
batch.close()

# ---- C3: one pair of large sets ----
N2 = max(3000, int(15_000_000 * SCALE))
pool = np.unique(rng.integers(0, 1 << 63, size=N2 + N2 // 64, dtype=U64))[:N2]
j = np.arange(len(pool))
a, b = pool[j % 3 != 2], pool[j % 3 != 1]
del pool, j
oa, ob = np.array([0, len(a)], U64), np.array([0, len(b)], U64)
A, B = eng.sets_from_arrays(oa, a), eng.sets_from_arrays(ob, b)
out, t_union = best(lambda o: A.union(B, into=o))
out.close()
if BASE:
    row("C3 pair of 10^7-value sets", union=t_union)
else:
    ca, cb = rng.integers(1, 100, size=len(a)).astype(U32), rng.integers(1, 100, size=len(b)).astype(U32)
    Ac, Bc = eng.sets_from_arrays_counted(oa, a, ca), eng.sets_from_arrays_counted(ob, b, cb)
    out, t_add = best(lambda o: Ac.add(Bc, into=o))

    def host():
        va, vb, xa, xb = Ac.fetch()[1], Bc.fetch()[1], Ac.fetch_counts(), Bc.fetch_counts()
        u, inv = np.unique(np.concatenate([va, vb]), return_inverse=True)
        s = np.zeros(len(u), U64)
        np.add.at(s, inv, np.concatenate([xa, xb]).astype(U64))
        return u, np.minimum(s, U64(2**32 - 1)).astype(U32)
    (hv, hc), t_host = timed(host)
    assert np.array_equal(hv, out.fetch()[1]) and np.array_equal(hc, out.fetch_counts())
    row("C3 pair of 10^7-value sets", add=t_add, union=t_union, ratio=f"{t_add / t_union:.2f}", host=t_host, speedup=f"x{t_host / t_add:.0f}")
    out.close()
    Ac.close()
    Bc.close()
    del ca, cb, hv, hc
A.close()
B.close()
del a, b

# ---- C4: one sample against many genomes ----
if not BASE:
    n3, s3, m3 = max(10, int(1000 * SCALE)), 180_000, 1_000_000
    v = np.cumsum(rng.integers(1, 12, size=(n3, s3), dtype=U64), axis=1, dtype=U64).reshape(-1)
    sample = np.cumsum(rng.integers(1, 3, size=m3, dtype=U64), dtype=U64)
    cs = rng.integers(1, 50, size=m3).astype(U32)
    G = eng.sets_from_arrays(np.arange(n3 + 1, dtype=U64) * U64(s3), v)
    Sm = eng.sets_from_arrays_counted(np.array([0, m3], U64), sample, cs)
    out, t_keep = best(lambda o: Sm.keep(G, into=o))
    tot, t_tot = best(lambda o: out.totals())

    def host():
        gv, sv, sc = G.fetch()[1], Sm.fetch()[1], Sm.fetch_counts()
        k = min(n3, 20)
        t = time.perf_counter()
        w = [int(sc[np.isin(sv, gv[s3 * i:s3 * (i + 1)], assume_unique=True)].astype(U64).sum()) for i in range(k)]
        return w, (time.perf_counter() - t) * (n3 / k - 1)  # (NumPy per genome on the first 20, scaled: the genomes are alike)
    (w, extra), t_host = timed(host)
    assert [int(x) for x in tot[:len(w)]] == w
    row("C4 KEEP sample x genomes + totals", keep=t_keep, totals=t_tot, host_extrapolated_from_20_genomes=t_host + extra, speedup=f"x{(t_host + extra) / (t_keep + t_tot):.0f}",
        plan=out.plan()["plan"])
