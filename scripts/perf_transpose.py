"""dev helper: time the hits by target (bsk_hits_transpose, bsk_hits_tally) on one GPU beside the host route they replace; best of
three wall times of the call, after a first call that sizes the arrays.
(T1) classified reads: 10^7 reads, one hit each, over 1 000 targets
(T2) multi-hit rows: 10^6 rows of 10 hits over 10^4 targets, with weights (a search of counted queries against a counted index)
(T3) a neighbour graph: about 4 10^4 nodes of 32 neighbours each, with totals
Per shape: transpose; tally on the path its n_targets takes and -- where n_targets is within the LDS bound -- on the other path too, by
asking for a table of 4 096 targets; the host routes: fetch + stable np.argsort + gather + hits_from_arrays (which brings shared and
totals back, not weights), and fetch + three np.bincount.
usage: perf_transpose.py [scale=1.0] [reps=3]   (scale < 1 shrinks the row counts)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bio_amd import sketches as S

SCALE = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
U64, U32 = np.uint64, np.uint32
eng = S.Engine(0)
rng = np.random.default_rng(7)


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


def host_transpose(h, nt):
    o, t, s = h.fetch()
    tot = h.fetch_totals() if h.has_totals() else None
    order = np.argsort(t, kind="stable")
    rows = np.repeat(np.arange(len(o) - 1, dtype=U32), np.diff(o).astype(np.int64))
    oo = np.concatenate([[0], np.cumsum(np.bincount(t, minlength=nt))]).astype(U64)
    return eng.hits_from_arrays(oo, rows[order], s[order], None if tot is None else tot[order])


def host_tally(h, nt):
    o, t, s = h.fetch()
    lens = np.diff(o).astype(np.int64)
    alone = np.repeat(lens == 1, lens)
    return np.bincount(t, minlength=nt), np.bincount(t[alone], minlength=nt), np.bincount(t, weights=s, minlength=nt)


def report(name, h, nt):
    inf = h.info()
    tr, t_tr = best(lambda o: h.transpose(nt, reuse=o))
    tl, t_tl = best(lambda o: h.tally(nt, into=o))
    plan = tl.plan()
    other = ""
    if nt <= 2048:  # the same hits into a table beyond the LDS bound: the other path
        tg, t_g = best(lambda o: h.tally(4096, into=o))
        other = f"; tally, global path (4 096 targets) {t_g*1e3:.2f} ms"
        assert np.array_equal(tg.rows[:nt], tl.rows) and np.array_equal(tg.shared[:nt], tl.shared)
        tg.close()
    ht, t_ht = best(lambda o: host_transpose(h, nt))
    assert all(np.array_equal(x, y) for x, y in zip(ht.fetch(), tr.fetch())), "the host route differs"
    hl, t_hl = best(lambda o: host_tally(h, nt))
    assert np.array_equal(hl[0].astype(U64), tl.rows) and np.array_equal(hl[1].astype(U64), tl.unique)
    print(f"{name}: {inf['n_queries']} rows, {inf['n_hits']} hits, {nt} targets", flush=True)
    print(f"  transpose {t_tr*1e3:.2f} ms | host route {t_ht*1e3:.1f} ms (x{t_ht/t_tr:.0f}) | {tr.plan()['plan']}", flush=True)
    print(f"  tally {t_tl*1e3:.2f} ms{other} | host route {t_hl*1e3:.1f} ms (x{t_hl/t_tl:.0f}) | {plan}", flush=True)
    for x in (tr, tl, ht):
        x.close()


# (T1)
n = int(10_000_000 * SCALE)
h = eng.hits_from_arrays(np.arange(n + 1, dtype=U64), rng.integers(0, 1000, n).astype(U32), rng.integers(1, 100, n).astype(U32))
report("T1 classified reads", h, 1000)
h.close()

# (T2): target t holds the values 1 000 t .. 1 000 t + 999; a query holds one value of each of 10 targets
n, nt = int(1_000_000 * SCALE), 10_000
tv = np.arange(nt * 1000, dtype=U64)
targets = eng.sets_from_arrays_counted(np.arange(nt + 1, dtype=U64) * U64(1000), tv, rng.integers(1, 5, len(tv)).astype(U32))
first = rng.integers(0, nt - 10 * 7, n)
qt = first[:, None] + 7 * np.arange(10)[None, :]  # ten targets, ascending
qv = (qt * 1000 + rng.integers(0, 1000, (n, 10))).astype(U64)
queries = eng.sets_from_arrays_counted(np.arange(n + 1, dtype=U64) * U64(10), qv.reshape(-1), rng.integers(1, 5, n * 10).astype(U32))
ix = targets.index_counted()
h = ix.search_counted(queries)
assert h.info()["n_hits"] == 10 * n and h.has_weights()
report("T2 multi-hit rows, weights", h, nt)
for x in (h, ix, queries, targets):
    x.close()

# (T3)
n = int(40_000 * SCALE)
nb = np.sort((np.arange(n)[:, None] + rng.choice(np.arange(1, 2000), size=32, replace=False)[None, :] * (1 + np.arange(n)[:, None] % 3)) % n, axis=1)
nb = [np.unique(r) for r in nb]
o = np.concatenate([[0], np.cumsum([len(r) for r in nb])]).astype(U64)
t = np.concatenate(nb).astype(U32)
s = rng.integers(1, 500, len(t)).astype(U32)
h = eng.hits_from_arrays(o, t, s, s + rng.integers(0, 500, len(t)).astype(U32))
report("T3 neighbour graph, totals", h, n)
h.close()
