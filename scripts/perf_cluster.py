"""dev helper: time the clustering of a neighbour graph (bsk_hits_cluster) on one GPU; best of three wall times of the call, after a
first call that sizes the arrays.
(a) DESIGN 3.12's M1 shape -- N sketches of 1 000 values from a pool of 20 000, every fourth followed by three near copies, all against
    all under a limit of 1 000, BSK_NEIGHBORS_UPPER, Jaccard >= 1/2: the neighbours call that makes the graph, then both methods on it, and
    beside them the host route: bsk_hits_fetch + a union-find on the host.
(b) a graph stated directly (hits_from_arrays): n nodes and m random edges, upper form; both methods, under index order and under random
    scores; the host route again.
The host union-find is scipy.sparse.csgraph.connected_components where SciPy is installed, else hook-and-jump in NumPy.
usage: perf_cluster.py [N=10000] [n=1000000] [m=10000000] [reps=3]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bio_amd import sketches as S

try:  # (imported here: the import is not part of the host route's time)
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
except ImportError:
    coo_matrix = connected_components = None

N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000
BIG_N = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
BIG_M = int(float(sys.argv[3])) if len(sys.argv) > 3 else 10_000_000
REPS = int(sys.argv[4]) if len(sys.argv) > 4 else 3
U64, U32 = np.uint64, np.uint32
eng = S.Engine(0)
rng = np.random.default_rng(3)


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


def host_components(n, offsets, target):
    """labels of the connected components from fetched CSR hits -> (the smallest member of every node's component, which tool did it)"""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets).astype(np.int64))
    cols = target.astype(np.int64)
    if connected_components is not None:
        _, lab = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n, n)), directed=False)
        first = np.full(lab.max() + 1 if n else 0, n, np.int64)
        np.minimum.at(first, lab, np.arange(n))
        return first[lab], "scipy"
    f = np.arange(n, dtype=np.int64)
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    while True:
        fn = f.copy()
        fu, fv = f[lo], f[hi]
        a = fu < fv
        np.minimum.at(fn, fv[a], fu[a])
        np.minimum.at(fn, hi[a], fu[a])
        b = fv < fu
        np.minimum.at(fn, fu[b], fv[b])
        np.minimum.at(fn, lo[b], fv[b])
        fn = np.minimum(fn, f[f])
        if np.array_equal(fn, f):
            return f, "numpy"
        f = fn


def report(tag, hits, score=None, host=True):
    n = hits.info()["n_queries"]
    out = {}
    for method in ("components", "greedy"):
        c, t = best(lambda o: hits.cluster(method, score, reuse=o))
        p, inf = c.plan(), c.info()
        out[method] = (c.label.copy(), c.rep.copy())
        print(f"  {tag} {method}: {t*1e3:.2f} ms, {inf['n_clusters']} clusters, largest {inf['largest']} | {p['plan']}", flush=True)
        c.close()
    if host:
        (res, t_fetch) = timed(lambda: hits.fetch())
        (lab, t_uf) = timed(lambda: host_components(n, res[0], res[1]))
        first, tool = lab
        rep = out["components"][1][out["components"][0]] if score is None else None
        assert rep is None or np.array_equal(rep.astype(np.int64), first), "the device's components differ from the host's"
        print(f"  {tag} host route: fetch {t_fetch*1e3:.2f} ms + union-find ({tool}) {t_uf*1e3:.2f} ms = {(t_fetch+t_uf)*1e3:.2f} ms", flush=True)


# ---- (a) the graph of a neighbours call ----
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
h, t_nb = best(lambda o: sk.neighbors(None, 1000, min_jaccard=(1, 2), upper=True, reuse=o))
print(f"(a) M1 {N} x {N} limit 1000, families of 4, upper, Jaccard >= 1/2: neighbors {t_nb*1e3:.1f} ms, {h.info()['n_hits']} pairs", flush=True)
report("(a)", h)
report("(a) score = random", h, score=rng.integers(0, 1 << 64, N, dtype=U64), host=False)
h.close()
sk.close()

# ---- (b) a graph from the host ----
if BIG_N and BIG_M:
    u, v = rng.integers(0, BIG_N, BIG_M, dtype=np.int64), rng.integers(0, BIG_N, BIG_M, dtype=np.int64)
    k = np.unique(np.minimum(u, v) * BIG_N + np.maximum(u, v))
    k = k[k // BIG_N != k % BIG_N]
    src, tgt = k // BIG_N, (k % BIG_N).astype(U32)
    offsets = np.zeros(BIG_N + 1, U64)
    offsets[1:] = np.cumsum(np.bincount(src, minlength=BIG_N), dtype=U64)
    g, t_up = timed(lambda: eng.hits_from_arrays(offsets, tgt, np.ones(len(tgt), U32)))
    print(f"(b) {BIG_N} nodes, {len(tgt)} random edges (upper form), hits_from_arrays {t_up*1e3:.1f} ms", flush=True)
    report("(b)", g)
    report("(b) score = random", g, score=rng.integers(0, 1 << 64, BIG_N, dtype=U64), host=False)
    g.close()
