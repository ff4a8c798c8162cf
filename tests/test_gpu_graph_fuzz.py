"""GPU: seeded programs over the compare, hits and clusters objects of the sets side against their NumPy model (tests/graph_programs.py),
exactly -- the second stateful campaign, beside tests/test_gpu_algebra_fuzz.py.

A program loads four collections, at least one counted and one uncounted (sometimes one comes from a sketch result), then chains 10 to
16 calls: the sets-making entries of the first campaign (they make the operands, and the objects whose counts array is stale), and
bsk_sets_compare / _compare_counted into one pool of compare objects, bsk_sets_neighbors / _neighbors_counted, an index build + search,
bsk_hits_top and bsk_hits_from_host into one pool of hits objects -- every writer into objects the others made --, bsk_hits_cluster of any
live hits whose targets fit (symmetric neighbour results, the one-directional graph of a top(n), square search results, host graphs) into
a pool of clusters objects, and calls the library must refuse with BSK_ERR_ARG.  After EVERY step the device's result is compared with
the model: everything the object can be asked -- info, the arrays, the payload flags (has_total, has_weights, weighted) and the payloads
they announce, the plan's tiles= / skipped= / rounds= / edges= figures, bsk_sets_sumsq on every sets object; the step's operands are
fetched again and must be what they were.  At the end of a program every sets, compare, hits and clusters object still alive is
fetched once more.  Every comparison is exact.  Odd programs run on a second context of the same device.

A failure names its seed and step and prints the program up to there; `python -m tests.graph_programs SEED` prints all of it.
tests/test_graph_programs.py shows on the CPU what the campaign reaches and that this comparison catches each of thirteen wrong models."""
import ctypes as C

import numpy as np
import pytest

from bio_amd import _lib as L
from tests import algebra_programs as AP
from tests import graph_programs as GP
from tests import neighbor_cases as NC
from tests.test_gpu_algebra_fuzz import Run as SetsRun
from tests.test_gpu_algebra_fuzz import second_engine, snap  # noqa: F401  (second_engine: the fixture)

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
SLICE = 10  # programs per test, half a block of the campaign: the 16 tests took 0.29-0.66 s each on an MI355X, model included


def hits_record(h):
    inf, (o, t, s), ht, hw = h.info(), h.fetch(), h.has_totals(), h.has_weights()
    d, m = h.fetch_weights() if hw else (None, None)
    return dict(n_queries=inf["n_queries"], n_hits=inf["n_hits"], offsets=o, target=t, shared=s, has_total=ht, has_weights=hw,
                total=h.fetch_totals() if ht else None, dot=d, min_sum=m)


def compare_record(c):
    inf, (sh, tt), w = c.info(), c.fetch(), c.weighted
    d, m = c.fetch_weights() if w else (None, None)
    return dict(n_a=inf["n_a"], n_b=inf["n_b"], limit=inf["limit"], shared=sh, total=tt, weighted=w, dot=d, min_sum=m)


def clusters_record(k):
    inf, (label, rep, offsets, members) = k.info(), k.fetch()
    return dict(n_items=inf["n_items"], n_clusters=inf["n_clusters"], largest=inf["largest"], label=label, rep=rep, offsets=offsets, members=members)


class Run(SetsRun):
    """one program on one engine: the device side of graph_programs.apply (the sets-making kinds are the first campaign's)"""

    def __init__(self, engine, other, prog):
        SetsRun.__init__(self, engine, other, prog)
        self.hits, self.clusters = {}, {}

    def refused(self, step):
        lib, ctx, what = self.eng.lib, self.eng.ctx, step["what"]
        sets = {i: self.live[i] for i in dict.fromkeys(step[x] for x in ("a", "b") if step[x] is not None)}
        hits = {i: self.hits[i] for i in dict.fromkeys(step[x] for x in ("hits", "hslot") if step[x] is not None)}
        pool = self.clusters if step["kslot"] is not None else self.hits
        mine = pool.get(step["kslot"] if step["kslot"] is not None else step["hslot"])
        slot = C.c_void_p(mine.h.value) if mine is not None else C.c_void_p()
        extra = []
        if "other engine" in what:  # an object of the slot's type that the second engine made
            extra.append(self.other.hits_from_arrays(np.array([0, 1, 2], U64), np.array([1, 0], U32), np.ones(2, U32)))
            if what.startswith("clusters"):
                extra.append(extra[0].cluster())
            slot = C.c_void_p(extra[-1].h.value)
        before = slot.value
        neighbors = lib.bsk_sets_neighbors_counted if step["counted"] else lib.bsk_sets_neighbors
        cp = L.ClusterParams(L.CLUSTER_GREEDY if step["counted"] else L.CLUSTER_COMPONENTS, 0)
        if what in ("cluster of rectangular hits", "clusters of the other engine in the slot"):
            rc = lib.bsk_hits_cluster(ctx, self.hits[step["hits"]].h, C.byref(cp), None, C.byref(slot))
        elif what in ("fetch_weights of hits without weights", "fetch_totals of hits without totals"):
            h = self.hits[step["hits"]]
            n, room = h.info()["n_queries"], h.info()["n_hits"] + 1
            d, m, t = np.zeros(room, U64), np.zeros(room, U64), np.zeros(room, U32)
            rc = lib.bsk_hits_fetch_weights(ctx, h.h, 0, n, d.ctypes.data, m.ctypes.data, room) if "weights" in what else \
                lib.bsk_hits_fetch_totals(ctx, h.h, 0, n, t.ctypes.data, room)
        elif what == "fetch_weights of an unweighted compare":
            c = self.cmps[step["cmp"]]
            inf = c.info()
            d, m = np.zeros(inf["n_a"] * inf["n_b"] + 1, U64), np.zeros(inf["n_a"] * inf["n_b"] + 1, U64)
            rc = lib.bsk_compare_fetch_weights(ctx, c.h, 0, inf["n_a"], d.ctypes.data, m.ctypes.data, d.size)
        elif what.startswith("neighbors") or what == "hits of the other engine in the slot":
            np_ = L.NeighborParams(1, 2 if "flag" in what else 0, 3 if "jaccard" in what else 0, 2 if "jaccard" in what else 0)
            rc = neighbors(ctx, self.live[step["a"]].h, self.live[step["b"]].h, 0, C.byref(np_), C.byref(slot))
        elif what == "hits_from_host with a row not strictly ascending":
            o, t, s = np.array([0, 1, 3], U64), np.array([0, 1, 1], U32), np.ones(3, U32)  # (the second row holds 1 twice)
            rc = lib.bsk_hits_from_host(ctx, o.ctypes.data, 2, t.ctypes.data, s.ctypes.data, None, C.byref(slot))
        else:
            assert what == "top into its own input", what
            rc = lib.bsk_hits_top(ctx, self.hits[step["hits"]].h, 1, C.byref(slot))
        rec = dict(rc="ERR_ARG" if rc == L.ERR_ARG and slot.value == before else "rc %d, the slot %s -> %s" % (rc, before, slot.value),
                   sets={i: snap(x) for i, x in sets.items()}, hits={i: hits_record(x) for i, x in hits.items()},
                   compares={i: compare_record(self.cmps[i]) for i in [step["cmp"]] if i is not None},
                   clusters={i: clusters_record(self.clusters[i]) for i in [step["kslot"]] if i is not None})
        for x in reversed(extra):
            x.close()
        return rec

    def step(self, step):
        k, live = step["kind"], self.live
        if k == "refused":
            return self.refused(step)
        if k in GP.SETS_KINDS:
            rec = SetsRun.step(self, dict(step, keep=True))
            rec["sumsq"] = live[step["out"]].sumsq()
            if not step.get("keep", True):
                live.pop(step["out"]).close()
            return rec
        if k in GP.CMP_ENTRY:
            a, b = live[step["a"]], live[step["b"]]
            c = (a.compare if k == "compare" else a.compare_counted)(b, step["limit"], reuse=self.cmps.get(step["cmp"]))
            self.cmps[step["cmp"]] = c
            pl = c.plan()
            return dict(compare_record(c), figures=(pl["tiles"], pl["rounds"], pl["max_rounds"]), operands={i: snap(live[i]) for i in (step["a"], step["b"])})
        if k == "cluster":
            src = self.hits[step["hits"]]
            c = src.cluster(step["method"], step["score"], reuse=self.clusters.get(step["slot"]))
            self.clusters[step["slot"]] = c
            pl = c.plan()
            return dict(clusters_record(c), figures=(pl["rounds"], pl["edges"]), input=hits_record(src))
        reuse = self.hits.get(step["slot"])
        extra = {}
        if k in ("neighbors", "neighbors_counted"):
            a, b = live[step["a"]], live[step["b"]]
            h = (a.neighbors if k == "neighbors" else a.neighbors_counted)(b, step["limit"], step["min_shared"], step["min_jaccard"], step["upper"], reuse=reuse)
            fig = NC.plan_figures(h.plan()["plan"])
            extra = dict(tiles=fig["tiles"], skipped=fig["skipped"])
            ops = (step["a"], step["b"])
        elif k == "search":
            ix = live[step["a"]].index()
            try:
                h = ix.search(live[step["q"]], min_shared=step["min_shared"], reuse=reuse)
            finally:
                ix.close()
            ops = (step["a"], step["q"])
        elif k == "top":
            h, ops = self.hits[step["hits"]].top(step["n"], reuse=reuse), ()
        else:
            assert k == "hits_load", k
            h, ops = self.eng.hits_from_arrays(step["offsets"], step["target"], step["shared"], step["total"], reuse=reuse), ()
        self.hits[step["slot"]] = h
        rec = dict(hits_record(h), **extra)
        if ops:
            rec["operands"] = {i: snap(live[i]) for i in ops}
        if k == "top":
            rec["input"] = hits_record(self.hits[step["hits"]])
        return rec

    def end(self):
        return dict(pool={i: snap(s) for i, s in self.live.items()}, compares={i: compare_record(c) for i, c in self.cmps.items()},
                    hits={i: hits_record(h) for i, h in self.hits.items()}, clusters={i: clusters_record(c) for i, c in self.clusters.items()})

    def close(self):
        for pool in (self.hits, self.clusters):
            for x in pool.values():
                x.close()
        SetsRun.close(self)


def run_program(engine, other, seed):
    prog, want = GP.program_and_records(seed)
    run = Run(engine, other, prog)
    try:
        sk = [s for s in prog if s["kind"] == "sketch"]
        if sk:
            want = GP.run_model(prog, read_values=run.sketch(sk[0]))  # (the generator's records stand on stand-in values)
        for i, step in enumerate(prog):
            diff = AP.same(want[i], run.step(step))
            assert not diff, GP.message(seed, i, prog, diff)
        diff = AP.same(want[-1], run.end())
        assert not diff, GP.message(seed, len(prog) - 1, prog, ["at the end of the program"] + diff)
    finally:
        run.close()


@pytest.mark.parametrize("part", range(GP.PER_BLOCK // SLICE))
@pytest.mark.parametrize("block", range(GP.BLOCKS))
def test_graph_programs(engine, second_engine, block, part):  # noqa: F811
    for n, seed in enumerate(GP.seeds(block)[part * SLICE:(part + 1) * SLICE]):
        engines = (engine, second_engine) if (part * SLICE + n) % 2 == 0 else (second_engine, engine)
        run_program(*engines, seed)
