"""GPU: seeded programs over the long-lived indexes, the window sets and the weighted and folded hits against their NumPy model
(tests/index_programs.py), exactly -- the third stateful campaign, beside tests/test_gpu_algebra_fuzz.py and tests/test_gpu_graph_fuzz.py.

A program loads four collections, at least one counted and one uncounted, one of them from a sketch result, then chains 10 to 16 calls:
the sets-making entries of the first campaign, bsk_result_sets_windows into any live sets, a window object reduced by its own
group_offsets, sets loaded on the second context; bsk_index_build / _build_counted of any live sets (stale counts and window sets
included), bsk_index_attach to the other context, handles closed while a sibling lives, the source sets overwritten or closed while the
index lives; bsk_index_search / _search_counted with min_shared and both covers through any live handle, bsk_hits_fold by a window
object's group_offsets or by random runs, bsk_hits_top, bsk_sets_neighbors / _neighbors_counted and bsk_hits_from_host -- every writer into
hits the others made --, and calls the library must refuse with BSK_ERR_ARG.  After EVERY step the device's result is compared with the
model: everything the object can be asked -- info, the arrays, has_total / has_weights / has_members with the payloads they announce,
n_large_queries, the plan's weights tail and groups= runs= kept=, an index's info and both norms through the handle in use --; the step's
operands are fetched again and must be what they were.  At the end of a program every sets, index and hits object still alive is fetched once
more and every hits object is asked its formulas: containment() and jaccard(), and of weighted hits cosine() and its kin -- "stale" where an
operand was written or closed since the call.  Every comparison is exact.  Odd programs run on a second context of the same device.

A failure names its seed and step and prints the program up to there; `python -m tests.index_programs SEED` prints all of it.
tests/test_index_programs.py shows on the CPU what the campaign reaches and that this comparison catches each of thirteen wrong models."""
import ctypes as C
import re

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import algebra_programs as AP
from tests import graph_programs as GP
from tests import index_programs as IP
from tests import neighbor_cases as NC
from tests.test_gpu_algebra_fuzz import KIND, second_engine, sets_record, snap  # noqa: F401  (second_engine: the fixture)
from tests.test_gpu_graph_fuzz import Run as GraphRun

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
SLICE = 10  # programs per test, half a block of the campaign: the 16 tests took 0.18-0.32 s each on an MI355X, model included
FOLD_PLAN = re.compile(r"bsk_hits_fold: .*, groups=(\d+) runs=(\d+) kept=(\d+)")


def hits_record(h):
    inf, (o, t, s), ht, hw, hm = h.info(), h.fetch(), h.has_totals(), h.has_weights(), h.has_members()
    d, m = h.fetch_weights() if hw else (None, None)
    return dict(n_queries=inf["n_queries"], n_hits=inf["n_hits"], offsets=o, target=t, shared=s, has_total=ht, has_weights=hw, has_members=hm,
                total=h.fetch_totals() if ht else None, dot=d, min_sum=m, members=h.fetch_members() if hm else None)


def index_record(ix):
    """bsk_index_counted, bsk_index_info and bsk_index_fetch_norms through this handle (not the norms the owner may have inherited)"""
    inf, eng = ix.info(), ix.eng
    n = inf["n_targets"]
    q, t = np.zeros(max(n, 1), U64), np.zeros(max(n, 1), U64)
    eng._chk(eng.lib.bsk_index_fetch_norms(eng.ctx, ix.h, 0, n, q.ctypes.data, t.ctypes.data))
    return dict(inf, counted=ix.counted, sumsq=q[:n], totals=t[:n], target_sizes=ix.target_sizes)


def formulas(h, sizes_known):
    """what the owner answers at the end of a program"""
    out = dict(plain=None, weighted=None)
    with np.errstate(all="ignore"):
        if sizes_known:
            out["plain"] = dict(containment=IP.fbits(h.containment()), jaccard=IP.fbits(h.jaccard()))
        if h.has_weights():
            try:
                w = {name: IP.fbits(getattr(h, name)()) for name in IP.FORMULAS[:4]}
            except ValueError as e:
                out["weighted"] = "stale" if "written or closed since the call" in str(e) else "closed" if "index was closed" in str(e) else "limit" if "whole sets" in str(e) else repr(e)
                return out
            try:
                w["weighted_containment"] = IP.fbits(h.weighted_containment())
            except ValueError:
                w["weighted_containment"] = "undefined"
            out["weighted"] = w
    return out


class Run(GraphRun):
    """one program on two engines: the device side of index_programs.apply (the sets-making kinds are the first campaign's)"""

    def __init__(self, engine, other, prog):
        GraphRun.__init__(self, engine, other, prog)
        self.engs = (engine, other)
        self.fsets, self.idx, self.core, self.known = {}, {}, {}, {}

    def sketch(self, step):
        """the sketch step's result and its tuples: what the model is made of"""
        self.batch = self.eng.batch(step["reads"])
        self.res = self.eng.run(self.batch, self.eng.params(KIND[step["sketch"]], step["k"], w=step["w"]))
        offs, _, hash_, pos = self.res.fetch()
        return offs, hash_, pos

    def result_sets(self, step, into):
        if step["counted"] or into is None:
            return GraphRun.result_sets(self, step, into)
        from tests.test_gpu_counts import switches
        with switches(self.eng, ("BSK_SETS_NO_SMALL",) if step["no_small"] else ()):  # bsk_result_sets_reuse has no owner method: the owners' own take-over
            S._take_over(self.eng, into, lambda out: self.eng.lib.bsk_result_sets_reuse(self.eng.ctx, self.res.h, int(step["whole"]), step["scale"], out))
        into.group_offsets = None
        return into

    def sets(self, i):
        return self.live[i] if i in self.live else self.fsets[i]

    def refused(self, step):
        what, eng = step["what"], self.engs[step["eng"]]
        lib, ctx, far = eng.lib, eng.ctx, self.engs[1 - step["eng"]]
        mine = self.hits.get(step["hslot"]) if step["hslot"] is not None else self.live.get(step["sslot"]) if step["sslot"] is not None else None
        slot = C.c_void_p(mine.h.value) if mine is not None else C.c_void_p()
        extra, sp = [], L.SearchParams(1, 0, 0.0, 0.0)
        if what == "search_counted into hits of the other engine":
            extra.append(far.hits_from_arrays(np.array([0, 1, 2], U64), np.array([1, 0], U32), np.ones(2, U32)))
            slot = C.c_void_p(extra[0].h.value)
        before = slot.value
        if what.startswith("fold"):
            go = np.ascontiguousarray(step["groups"], U64)
            rc = lib.bsk_hits_fold(ctx, self.hits[step["hits"]].h, go.ctypes.data, len(go) - 1, None, C.byref(slot))
        elif what == "fetch_members of hits without members":
            h = self.hits[step["hits"]]
            buf = np.zeros(h.info()["n_hits"] + 1, U32)
            rc = lib.bsk_hits_fetch_members(ctx, h.h, 0, h.info()["n_queries"], buf.ctypes.data, buf.size)
        elif what == "fetch_norms with a range outside the targets":
            ix, buf = self.idx[step["x"]], np.zeros(3, U64)
            rc = lib.bsk_index_fetch_norms(ctx, ix.h, max(ix.info()["n_targets"] - 2, 0), 3, buf.ctypes.data, None)
        elif what == "search_counted with queries of the other engine":
            extra.append(far.sets_from_arrays(np.array([0, 1], U64), np.array([5], U64)))
            rc = lib.bsk_index_search_counted(ctx, self.idx[step["x"]].h, extra[0].h, C.byref(sp), C.byref(slot))
        elif what == "search_counted into hits of the other engine":
            rc = lib.bsk_index_search_counted(ctx, self.idx[step["x"]].h, self.sets(step["a"]).h, C.byref(sp), C.byref(slot))
        elif what == "index_build_counted of foreign sets":
            if step["a"] is None:
                extra.append(far.sets_from_arrays_counted(np.array([0, 2], U64), np.array([5, 7], U64), np.array([1, 2], U32)))
            rc = lib.bsk_index_build_counted(ctx, (self.live[step["a"]] if step["a"] is not None else extra[0]).h, C.byref(slot))
        else:
            assert what == "window_sets with window == 0 and count == 0", what
            wp, go = L.WindowParams(0, 0, 0, 0), np.zeros(self.res.info()["n_reads"] + 1, U64)
            rc = lib.bsk_result_sets_windows(ctx, self.res.h, C.byref(wp), 1, C.byref(slot), go.ctypes.data)
        rec = dict(rc="ERR_ARG" if rc == L.ERR_ARG and slot.value == before else "rc %d, the slot %s -> %s" % (rc, before, slot.value),
                   sets={i: snap(self.sets(i)) for i in dict.fromkeys(step[x] for x in ("a", "sslot") if step[x] is not None)},
                   hits={i: hits_record(self.hits[i]) for i in dict.fromkeys(step[x] for x in ("hits", "hslot") if step[x] is not None)},
                   indexes={i: index_record(self.idx[i]) for i in [step["x"]] if i is not None})
        for x in extra:
            x.close()
        return rec

    def step(self, step):
        k, live = step["kind"], self.live
        if k == "refused":
            return self.refused(step)
        if k in GP.SETS_KINDS:
            return GraphRun.step(self, step)
        if k == "windows":
            r = self.res.window_sets(step.get("window", 0), step.get("step", 0), step.get("count", 0), step["scale"], step["counted"], into=live.get(step["out"]) if step["into"] else None)
            live[step["out"]] = r
            rec = dict(sets_record(r, {}), sumsq=r.sumsq(), group_offsets=r.group_offsets)
            if not step.get("keep", True):
                live.pop(step["out"]).close()
            return rec
        if k == "copy":
            o, v, c = snap(live[step["a"]])
            f = self.other.sets_from_arrays(o, v) if c is None else self.other.sets_from_arrays_counted(o, v, c)
            self.fsets[step["out"]] = f
            rec = sets_record(f, {step["a"]: live[step["a"]]})
            return dict(rec, sumsq=f.sumsq())
        if k == "close_sets":
            (live if step["a"] in live else self.fsets).pop(step["a"]).close()
            return dict(closed=step["a"])
        if k == "index":
            a = live[step["a"]]
            self.idx[step["out"]], self.core[step["out"]] = a.index_counted() if step["counted"] else a.index(), step["out"]
            return dict(index_record(self.idx[step["out"]]), operands={step["a"]: snap(a)})
        if k == "attach":
            src = self.idx[step["x"]]
            self.idx[step["out"]], self.core[step["out"]] = src.attach(self.other if src.eng is self.eng else self.eng), self.core[step["x"]]
            return index_record(self.idx[step["out"]])
        if k == "close_index":
            self.idx.pop(step["x"]).close()
            return dict(closed=step["x"], siblings={i: index_record(ix) for i, ix in self.idx.items() if self.core[i] == self.core[step["x"]]})
        reuse, extra = self.hits.get(step["slot"]), {}
        if k in ("search", "search_counted"):
            ix, q = self.idx[step["x"]], self.sets(step["q"])
            h = (ix.search if k == "search" else ix.search_counted)(q, step["min_shared"], step["min_query_cov"], step["min_target_cov"], reuse=reuse)
            pl = h.plan()
            extra = dict(n_large_queries=pl["n_large_queries"], operands={step["q"]: snap(q)}, index=index_record(ix))
            if k == "search_counted":
                extra["plan_tail"] = pl["plan"][pl["plan"].index("; weights:"):] if "; weights:" in pl["plan"] else pl["plan"]
            known = True
        elif k == "fold":
            src = self.hits[step["hits"]]
            h = src.fold(step["groups"], step["rule"].get("min_members", 1), step["rule"].get("frac"), reuse=reuse)
            pl = h.plan()
            m = FOLD_PLAN.fullmatch(pl["plan"])
            extra = dict(n_large_queries=pl["n_large_queries"], figures=tuple(int(x) for x in m.groups()) if m else pl["plan"], input=hits_record(src))
            known = self.known[step["hits"]]
        elif k == "top":
            src = self.hits[step["hits"]]
            h = src.top(step["n"], reuse=reuse)
            extra, known = dict(input=hits_record(src)), self.known[step["hits"]]
        elif k == "hits_load":
            h, known = self.engs[step["eng"]].hits_from_arrays(step["offsets"], step["target"], step["shared"], step["total"], reuse=reuse), False
        else:
            assert k in ("neighbors", "neighbors_counted"), k
            a, b = live[step["a"]], live[step["b"]]
            h = (a.neighbors if k == "neighbors" else a.neighbors_counted)(b, step["limit"], step["min_shared"], step["min_jaccard"], step["upper"], reuse=reuse)
            fig = NC.plan_figures(h.plan()["plan"])
            extra, known = dict(tiles=fig["tiles"], skipped=fig["skipped"], operands={i: snap(live[i]) for i in (step["a"], step["b"])}), True
        self.hits[step["slot"]], self.known[step["slot"]] = h, known
        return dict(hits_record(h), **extra)

    def end(self):
        return dict(pool={i: snap(s) for i, s in self.live.items()}, groups={i: s.group_offsets for i, s in self.live.items() if s.group_offsets is not None},
                    foreign={i: snap(s) for i, s in self.fsets.items()}, indexes={i: index_record(ix) for i, ix in self.idx.items()},
                    hits={i: dict(hits_record(h), **formulas(h, self.known[i])) for i, h in self.hits.items()})

    def close(self):
        for pool in (self.idx, self.fsets):
            for x in pool.values():
                x.close()
        GraphRun.close(self)


COUNTS = dict(programs=0, calls=0, objects=0)


def run_program(engine, other, seed):
    prog, want = IP.program_and_records(seed)
    run = Run(engine, other, prog)
    try:
        sk = [s for s in prog if s["kind"] == "sketch"][0]
        want, steps = IP.run_concrete(prog, tuples=run.sketch(sk))  # (the generator's records stand on stand-in tuples; the steps with the group offsets that follow the tuples)
        for i, step in enumerate(steps):
            diff = AP.same(want[i], run.step(step))
            assert not diff, IP.message(seed, i, prog, diff)
        end = run.end()
        diff = AP.same(want[-1], end)
        assert not diff, IP.message(seed, len(prog) - 1, prog, ["at the end of the program"] + diff)
        COUNTS["programs"] += 1
        COUNTS["calls"] += len(prog)
        COUNTS["objects"] += len(prog) + sum(len(end[p]) for p in ("pool", "foreign", "indexes", "hits"))
    finally:
        run.close()


@pytest.mark.parametrize("part", range(IP.PER_BLOCK // SLICE))
@pytest.mark.parametrize("block", range(IP.BLOCKS))
def test_index_programs(engine, second_engine, block, part):  # noqa: F811
    for n, seed in enumerate(IP.seeds(block)[part * SLICE:(part + 1) * SLICE]):
        engines = (engine, second_engine) if (part * SLICE + n) % 2 == 0 else (second_engine, engine)
        run_program(*engines, seed)
    print("so far: %(programs)d programs, %(calls)d calls, %(objects)d objects compared" % COUNTS)
