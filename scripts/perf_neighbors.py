"""dev helper: time the sparse all-pairs comparison (bsk_sets_neighbors) beside the dense one on one GPU; best of three wall times of the
call, after a first call that sizes the arrays.  The shape is DESIGN 3.9's M1 -- N sketches of 1 000 values from a pool of 20 000, all
against all, limit 1 000 -- with every fourth sketch followed by three near copies (100 of its values replaced), so that a threshold of
Jaccard 1/2 keeps the families and nothing else.
(a) bsk_sets_compare + bsk_compare_fetch of both matrices + the same filter in NumPy: the only route without the entry
(b) bsk_sets_neighbors, every pair            (c) ... with BSK_NEIGHBORS_UPPER            (d) (c) followed by bsk_hits_top(5)
(e) bsk_sets_neighbors_counted on the same values with counts 1 .. 9 attached, every pair and upper, beside (b) and (c) -- the calls
alternate, and every time of the repeats is printed, so the spread shows -- and beside bsk_sets_compare_counted + fetch + host filter
and the 46 400 x 46 400 case of one-value sets that the dense compare refuses.
Two commits against each other (the unweighted rows (b) and (c), whose kernel a change may not slow): check the other commit out beside
this one, build both, and run each tree's own copy of this script in turn, several times, alternating; rows (b) and (c) print every
repeat, so the spread of either tree shows beside the difference between them.
usage: perf_neighbors.py [N=10000] [reps=3]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bio_amd import sketches as S

N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
U64 = np.uint64
NUM, DEN = 1, 2
eng = S.Engine(0)
rng = np.random.default_rng(3)


def timed(fn):
    eng.lib.bsk_ctx_sync(eng.ctx)
    t = time.perf_counter()
    out = fn()
    eng.lib.bsk_ctx_sync(eng.ctx)
    return out, time.perf_counter() - t


def best(fn):
    b, out, best.times = 1e9, None, []
    for k in range(REPS + 1):  # (the first call sizes the result's arrays and the context's temporaries)
        out, dt = timed(lambda: fn(out))
        b = min(b, dt)
        if k:
            best.times.append(dt * 1e3)
    return out, b


pool = np.unique(rng.integers(0, 1 << 64, 20_200, dtype=U64))[:20_000]
fam = (N + 3) // 4
keys = rng.random((fam, len(pool)), dtype=np.float32)
order = np.argpartition(keys, 1100, axis=1)[:, :1100]  # 1 000 of the pool per family, and 100 spares
del keys
rows = []
for f in range(fam):
    base, spare = order[f, :1000], order[f, 1000:]
    rows.append(base)
    for _ in range(3):
        m = base.copy()
        m[rng.choice(1000, 100, replace=False)] = spare
        rows.append(m)
vals = np.sort(pool[np.array(rows[:N])], axis=1)
sk = eng.sets_from_arrays(np.arange(N + 1, dtype=U64) * U64(1000), vals.reshape(-1))


def dense_route(o):
    cmp = sk.compare(sk, 1000, reuse=o)
    sh, tt = cmp.fetch()
    keep = (sh >= 1) & (sh * np.uint32(DEN) >= np.uint32(NUM) * tt)  # (cells of at most 1 000: no product wraps)
    i, j = np.nonzero(keep)
    dense_route.out = (np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(U64), j.astype(np.uint32), sh[i, j], tt[i, j])
    return cmp


cmp, t_dense_only = best(lambda o: sk.compare(sk, 1000, reuse=o))
cmp, t_a = best(dense_route)
want = dense_route.out
p = cmp.plan()
cmp.close()
hb, t_b = best(lambda o: sk.neighbors(None, 1000, min_jaccard=(NUM, DEN), reuse=o))
got = (hb.offsets, hb.target, hb.shared, hb.total)
assert all(np.array_equal(x, y) for x, y in zip(got, want)), "neighbors differs from the filtered dense compare"
pb, ts_b = hb.plan()["plan"], " ".join("%.1f" % x for x in best.times)
hc, t_c = best(lambda o: sk.neighbors(None, 1000, min_jaccard=(NUM, DEN), upper=True, reuse=o))
pc, ts_c = hc.plan()["plan"], " ".join("%.1f" % x for x in best.times)
up = want[1].astype(np.int64) > np.repeat(np.arange(N), np.diff(want[0]).astype(np.int64))
assert np.array_equal(hc.target, want[1][up]) and np.array_equal(hc.shared, want[2][up])
top = None


def knn(o):
    global top
    h = sk.neighbors(None, 1000, min_jaccard=(NUM, DEN), upper=True, reuse=o)
    top = h.top(5, reuse=top)
    return h


hd, t_d = best(knn)
print(f"M1 {N} x {N} limit 1000, families of 4, keep Jaccard >= {NUM}/{DEN}: dense compare alone {t_dense_only*1e3:.1f} ms (tiles {p['tiles']} rounds {p['rounds']})", flush=True)
print(f"  (a) compare + fetch of both matrices + NumPy filter {t_a*1e3:.1f} ms, {len(want[1])} pairs kept", flush=True)
print(f"  (b) neighbors {t_b*1e3:.1f} ms (after the sizing call: {ts_b})  x{t_a/t_b:.1f} of (a), {t_b/t_dense_only:.3f} of the dense compare | {pb}", flush=True)
print(f"  (c) neighbors, upper {t_c*1e3:.1f} ms (after the sizing call: {ts_c})  {t_c/t_b:.3f} of (b), {hc.info()['n_hits']} pairs | {pc}", flush=True)
print(f"  (d) (c) + top(5) {t_d*1e3:.1f} ms, {top.info()['n_hits']} hits", flush=True)

# ---- (e) the weighted neighbours: the same values with counts attached, alternating with the unweighted calls ----
def weighted_rows():
    skc = eng.sets_from_arrays_counted(np.arange(N + 1, dtype=U64) * U64(1000), vals.reshape(-1), rng.integers(1, 10, vals.size).astype(np.uint32))
    routes = {
        "neighbors": lambda o: sk.neighbors(None, 1000, min_jaccard=(NUM, DEN), reuse=o),
        "neighbors, values of the counted sets": lambda o: skc.neighbors(None, 1000, min_jaccard=(NUM, DEN), reuse=o),
        "neighbors_counted": lambda o: skc.neighbors_counted(None, 1000, min_jaccard=(NUM, DEN), reuse=o),
        "neighbors, upper": lambda o: sk.neighbors(None, 1000, min_jaccard=(NUM, DEN), upper=True, reuse=o),
        "neighbors_counted, upper": lambda o: skc.neighbors_counted(None, 1000, min_jaccard=(NUM, DEN), upper=True, reuse=o),
        "compare": lambda o: sk.compare(sk, 1000, reuse=o),
        "compare_counted": lambda o: skc.compare_counted(skc, 1000, reuse=o),
    }
    held = {k: fn(None) for k, fn in routes.items()}  # (the sizing calls)
    times = {k: [] for k in routes}
    for _ in range(max(REPS, 5)):
        for k, fn in routes.items():
            held[k], dt = timed(lambda: fn(held[k]))
            times[k].append(dt * 1e3)
    hw = held["neighbors_counted"]
    assert all(np.array_equal(x, y) for x, y in zip((hw.offsets, hw.target, hw.shared, hw.total), want)), "neighbors_counted differs from the filtered dense compare"

    def dense_counted_route(o):
        cmp = skc.compare_counted(skc, 1000, reuse=o)
        sh, tt = cmp.fetch()
        dt, ms = cmp.fetch_weights()
        keep = (sh >= 1) & (sh * np.uint32(DEN) >= np.uint32(NUM) * tt)
        i, j = np.nonzero(keep)
        dense_counted_route.out = (dt[i, j], ms[i, j])
        return cmp

    held["compare_counted + fetch + filter"] = held.pop("compare_counted")
    times["compare_counted + fetch + filter"] = []
    for _ in range(REPS):
        held["compare_counted + fetch + filter"], dt = timed(lambda: dense_counted_route(held["compare_counted + fetch + filter"]))
        times["compare_counted + fetch + filter"].append(dt * 1e3)
    assert np.array_equal(hw.dot, dense_counted_route.out[0]) and np.array_equal(hw.min_sum, dense_counted_route.out[1]), "weights differ from the dense cells"
    print(f"  (e) weighted, counts 1..9, {max(REPS, 5)} alternating repeats: all times in ms, then min / median", flush=True)
    for k, t in times.items():
        print(f"      {k}: {' '.join('%.1f' % x for x in t)} | min {min(t):.1f} median {float(np.median(t)):.1f}", flush=True)
    mn = {k: min(t) for k, t in times.items()}
    print(f"      (i) neighbors_counted / neighbors {mn['neighbors_counted'] / mn['neighbors']:.3f} (upper {mn['neighbors_counted, upper'] / mn['neighbors, upper']:.3f}); "
          f"the dense pair, compare_counted / compare {mn['compare_counted'] / mn['compare']:.3f}", flush=True)
    print(f"      (ii) neighbors_counted / (compare_counted + fetch + filter) {mn['neighbors_counted'] / mn['compare_counted + fetch + filter']:.3f} | {hw.plan()['plan']}", flush=True)
    for x in list(held.values()) + [skc]:
        x.close()


weighted_rows()
for x in (hb, hc, hd, top, sk):
    x.close()

# ---- beyond 2^31 cells ----
n = 46_400
one = eng.sets_from_arrays(np.arange(n + 1, dtype=U64), np.arange(n, dtype=U64) // U64(2))
h, t_full = best(lambda o: one.neighbors(reuse=o))
assert h.info()["n_hits"] == 2 * n
pf = h.plan()["plan"]
h, t_up = best(lambda o: one.neighbors(upper=True, reuse=o))
assert h.info()["n_hits"] == n // 2
print(f"P1 {n} x {n} sets of one value ({n*n} cells), limit 0: neighbors {t_full*1e3:.1f} ms | {pf}", flush=True)
print(f"   upper {t_up*1e3:.1f} ms | {h.plan()['plan']}", flush=True)
