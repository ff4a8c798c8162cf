"""dev helper: time the window sets (bsk_result_sets_windows) and the folded hits (bsk_hits_fold) on one GPU; best of `reps` wall times of
the call, after a first call that sizes the arrays, and the spread (worst - best) beside it.
(a) G synthetic genomes of L bases, minimizer k = 21 w = 11: window sets with count = 10 and with window = L / 10, step = L / 20, against
    the route that exists without the entry: bsk_result_fetch + the NumPy model of tests/window_cases.py + bsk_sets_from_host.
(b) bsk_result_sets per sequence on R reads of 150 bases (the entry whose host code the windows share): run it on the parent commit too.
(c) bsk_hits_fold of Q rows x 20 hits into groups of 10 targets, against fetch + the NumPy model + hits_from_arrays, and against the
    bytes it must move (8 B per hit in, 12 B per kept hit out, the offsets) over the rate a plain device copy of the hits reaches.
usage: perf_windows.py [G=1000] [L=4000000] [R=10000000] [Q=10000000] [reps=3]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bio_amd import _lib as L_
from bio_amd import sketches as S
from tests import window_cases as WC

G = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1000
LEN = int(float(sys.argv[2])) if len(sys.argv) > 2 else 4_000_000
R = int(float(sys.argv[3])) if len(sys.argv) > 3 else 10_000_000
Q = int(float(sys.argv[4])) if len(sys.argv) > 4 else 10_000_000
REPS = int(sys.argv[5]) if len(sys.argv) > 5 else 3
U64, U32 = np.uint64, np.uint32
eng = S.Engine(0)
rng = np.random.default_rng(5)


def timed(fn):
    eng.lib.bsk_ctx_sync(eng.ctx)
    t = time.perf_counter()
    out = fn()
    eng.lib.bsk_ctx_sync(eng.ctx)
    return out, time.perf_counter() - t


def best(fn):
    ts, out = [], None
    for i in range(REPS + 1):  # (the first call sizes the result's arrays and the context's temporaries)
        out, dt = timed(lambda: fn(out))
        if i:
            ts.append(dt)
    return out, min(ts), max(ts) - min(ts)


# ---- (a) window sets of genomes ----
if G:
    b = eng.synth(L_.ALPHA_DNA, G, LEN, 0x5EED0A)
    res = eng.run(b, eng.params(L_.MINIMIZER, 21, w=11))
    print(f"(a) {G} genomes of {LEN} bases: {res.info()['n_tuples']} minimizers (k=21 w=11), {res.plan()['kernel']}", flush=True)
    for kw in (dict(count=10), dict(window=LEN // 10, step=LEN // 20)):
        ws, t, sp = best(lambda o: res.window_sets(into=o, **kw))
        inf = ws.info()
        print(f"  window_sets {kw}: {t*1e3:.2f} ms (spread {sp*1e3:.2f}), {inf['n_sets']} sets, {inf['n_values']} values", flush=True)
        (host, t_fetch) = timed(lambda: res.fetch())
        t0 = time.perf_counter()
        want = WC.windows_model(host[0], host[2], host[3], **kw)
        t_model = time.perf_counter() - t0
        (up, t_up) = timed(lambda: eng.sets_from_arrays(want[1], want[2]))
        assert WC.same(ws.fetch(), want[1:3]) and np.array_equal(ws.group_offsets, want[0]), "the device's windows differ from the host's"
        host_ms = (t_fetch + t_model + t_up) * 1e3
        print(f"  host route: fetch {t_fetch*1e3:.1f} + NumPy {t_model*1e3:.1f} + from_host {t_up*1e3:.1f} = {host_ms:.1f} ms: x{host_ms / (t * 1e3):.1f}", flush=True)
        up.close()
        ws.close()
        del host, want
    res.close()
    b.close()

# ---- (b) per-sequence sets of reads: the path the refactor must leave as it was ----
if R:
    b = eng.synth(L_.ALPHA_DNA, R, 150, 0x5EED0B)
    res = eng.run(b, eng.params(L_.MINIMIZER, 21, w=11))
    h = C.c_void_p()

    def per_sequence(_):
        rc = eng.lib.bsk_result_sets_reuse(eng.ctx, res.h, L_.SETS_PER_SEQUENCE, 1, C.byref(h))
        assert rc == L_.OK
        return h

    _, t, sp = best(per_sequence)
    print(f"(b) bsk_result_sets per sequence, {R} reads of 150 bases: {t*1e3:.2f} ms (spread {sp*1e3:.2f})", flush=True)
    if hasattr(eng.lib, "bsk_result_sets_windows"):  # (absent from a parent commit's library loaded through BSK_LIB with BSK_LIB_PARTIAL=1)
        ws, t, sp = best(lambda o: res.window_sets(window=64, into=o))
        print(f"    window_sets(window=64) of the same reads: {t*1e3:.2f} ms (spread {sp*1e3:.2f}), {ws.info()['n_sets']} sets", flush=True)
        ws.close()
    eng.lib.bsk_sets_release(h)
    res.close()
    b.close()

# ---- (c) folded hits ----
if Q:
    n_targets = 1_000_000
    t0 = (rng.integers(0, n_targets - 400, Q, dtype=np.int64))[:, None] + np.sort(rng.choice(400, 20, replace=False))[None, :]  # 20 ascending targets a row
    tgt = t0.reshape(-1).astype(U32)
    del t0
    offs = np.arange(Q + 1, dtype=U64) * U64(20)
    sh = rng.integers(1, 100, len(tgt)).astype(U32)
    go = np.arange(0, n_targets + 1, 10, dtype=U64)
    hits = eng.hits_from_arrays(offs, tgt, sh)
    f, t, sp = best(lambda o: hits.fold(go, reuse=o))
    K = f.info()["n_hits"]
    moved = len(tgt) * 8 + K * 12 + (Q + 1) * 16
    print(f"(c) fold of {Q} rows x 20 hits into {len(go) - 1} groups of 10: {t*1e3:.2f} ms (spread {sp*1e3:.2f}), {K} kept | {f.plan()['plan']}", flush=True)
    # the rate a plain device-to-device copy of the hits reaches (read + write), as the yardstick of the bytes the fold must move
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    po, pt, ps = hits.device()
    nbytes = len(tgt) * 4
    _, tc, _ = best(lambda o: (hip.hipMemcpy(ps, pt, nbytes, 3), hip.hipDeviceSynchronize()))
    hip.hipMemcpy(ps, sh.ctypes.data, nbytes, 1)
    rate = 2 * nbytes / tc
    print(f"    must move {moved/1e9:.2f} GB; a plain copy runs at {rate/1e12:.2f} TB/s -> {moved/rate*1e3:.2f} ms: the fold takes x{t/(moved/rate):.1f} of that", flush=True)
    (host, t_fetch) = timed(lambda: hits.fetch())
    t1 = time.perf_counter()
    want = WC.fold_model(host[0], host[1], host[2], go)
    t_model = time.perf_counter() - t1
    (up, t_up) = timed(lambda: eng.hits_from_arrays(want[0], want[1], want[2]))
    assert WC.same(f.fetch(), want[:3]) and np.array_equal(f.members, want[3]), "the device's fold differs from the host's"
    host_ms = (t_fetch + t_model + t_up) * 1e3
    print(f"    host route: fetch {t_fetch*1e3:.1f} + NumPy {t_model*1e3:.1f} + hits_from_arrays {t_up*1e3:.1f} = {host_ms:.1f} ms: x{host_ms / (t * 1e3):.1f}", flush=True)
