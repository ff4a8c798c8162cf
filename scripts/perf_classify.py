"""dev helper: reads in host memory -> the best target of every read, end to end, two ways on the same data.
S1 of perf_search.py: G synthetic genomes of 1 Mbp -> index of their per-sequence minimizer sets (k = 21, w = 11); R reads of 150 bp cut from
them (half reverse-complemented), top_n = 1.
  hits sink: bsk_pipeline_open_memory_search (BSK_SINK_HITS) -- every worker sketches, reduces to sets, searches its handle of the index and
             keeps the best hit per read on the device; the chunks carry hits.
  yardstick: the route without it -- BSK_SINK_SETS brings every read's set to the host, the consumer sends the values back up
             (bsk_sets_from_host), searches on ONE context (bsk_index_search) and fetches every hit (bsk_hits_fetch), chunk by chunk.
Both with the same devices and streams, alternating, `reps` runs each after a warm-up of both.
usage: perf_classify.py [G=1000] [R=1e7] [streams=3] [reps=3] [chunk_records=262144]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bio_amd import _lib as L
from bio_amd import sketches as S

G = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1000
R = int(float(sys.argv[2])) if len(sys.argv) > 2 else 10_000_000
STREAMS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
REPS = int(sys.argv[4]) if len(sys.argv) > 4 else 3
CHUNK = int(sys.argv[5]) if len(sys.argv) > 5 else 1 << 18
eng = S.Engine(0)

glen, rlen = 1_000_000, 150
gb = eng.synth(L.ALPHA_DNA, G, glen, 0x5EED0007)
p = eng.params(L.MINIMIZER, 21, w=11)
gsets = eng.run(gb, p).device_sets()
ix = gsets.index()
gsets.close()
gdata, _ = gb.fetch_ascii(0, G)
gb.close()
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
data = reads.reshape(-1)
roffs = np.arange(R + 1, dtype=np.uint64) * np.uint64(rlen)
up_bytes = R * (40 + 8)
print(f"S1: {G} genomes, {R} reads of {rlen} bp, {STREAMS} streams, chunks of {CHUNK}; index {ix.info()}", flush=True)


def run_hits():
    t = time.perf_counter()
    correct = best = down = 0
    with S.Engine.pipeline_open(p, data=data, offsets=roffs, devices=[0], n_streams=STREAMS, chunk_records=CHUNK, sink=L.SINK_HITS, alphabet=L.ALPHA_DNA,
                                search=ix, top_n=1) as pl:
        for c in pl.chunks():
            has = np.diff(c.offsets) > 0
            best += int(has.sum())
            correct += int((c.target == src[c.first_record:c.first_record + c.n_records][has]).sum())
            down += c.link_bytes
    dt = time.perf_counter() - t
    return dt, pl.stats, dict(reads_with_a_hit=best, best_is_the_source=correct, down=down, up=up_bytes)


def run_yardstick():
    t = time.perf_counter()
    correct = best = down = up = 0
    search_s = 0.0
    hits = None
    with S.Engine.pipeline_open(p, data=data, offsets=roffs, devices=[0], n_streams=STREAMS, chunk_records=CHUNK, sink=L.SINK_SETS, sets_scale=1,
                                alphabet=L.ALPHA_DNA) as pl:
        for c in pl.chunks():
            t0 = time.perf_counter()
            o64 = c.offsets.astype(np.uint64)
            qs = eng.sets_from_arrays(o64, c.hash)
            hits = ix.search(qs, reuse=hits)
            o, tg, sh = hits.fetch()
            qs.close()
            search_s += time.perf_counter() - t0
            # the best hit of every read, on the host (a classifier keeps one)
            cnt = np.diff(o).astype(np.int64)
            has = cnt > 0
            if len(tg):
                q = np.repeat(np.arange(len(cnt)), cnt)
                order = np.lexsort((tg, -sh.astype(np.int64), q))
                firsts = order[o[:-1][has].astype(np.int64)]
                best += int(has.sum())
                correct += int((tg[firsts] == src[c.first_record:c.first_record + c.n_records][has]).sum())
            down += c.link_bytes + 8 * (len(o) + len(tg))
            up += 8 * (len(o64) + len(c.hash))
    dt = time.perf_counter() - t
    st = dict(pl.stats)
    st["consumer_search_seconds"] = search_s
    return dt, st, dict(reads_with_a_hit=best, best_is_the_source=correct, down=down, up=up_bytes + up)


def show(name, dt, st, x):
    print(f"{name}: {dt:7.3f} s  {R/dt/1e6:7.2f} M reads/s  {R*rlen/dt/1e9:6.2f} Gbases/s | up {x['up']/R:6.1f} B/read, down {x['down']/R:6.1f} B/read | "
          f"h2d+pack {st['h2d_pack_seconds']:.2f} s, kernel {st['kernel_seconds']:.2f} s, fetch {st['fetch_seconds']:.2f} s (summed over {st['n_streams']} workers)"
          + (f", consumer search {st['consumer_search_seconds']:.2f} s" if "consumer_search_seconds" in st else "")
          + f" | {x['reads_with_a_hit']} reads with a hit, {x['best_is_the_source']} best = source", flush=True)


run_hits()
run_yardstick()  # warm-up of both: pinned buffers, pools, the index's first use
res = {"hits": [], "yard": []}
for i in range(REPS):
    for name, fn in (("hits sink", run_hits), ("yardstick", run_yardstick)):
        dt, st, x = fn()
        show(f"{name} run {i}", dt, st, x)
        res["hits" if fn is run_hits else "yard"].append(dt)
h, y = min(res["hits"]), min(res["yard"])
spread = max(res["yard"]) - min(res["yard"])
print(f"best: hits sink {h:.3f} s ({R/h/1e6:.2f} M reads/s), yardstick {y:.3f} s ({R/y/1e6:.2f} M reads/s), yardstick spread {spread:.3f} s; "
      f"hits sink {'is not slower' if h <= y + spread else 'IS SLOWER'} ({y/h:.2f}x)")
ix.close()
