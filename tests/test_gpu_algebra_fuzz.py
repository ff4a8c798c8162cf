"""GPU: seeded programs over the sets-side entries against their NumPy model (tests/algebra_programs.py), exactly.

A program loads a few collections (sometimes one comes from a sketch result), then chains 8 to 14 calls -- bsk_sets_op, _op_counted,
_reduce, _filter_counts, _bottom, _compare, an index build + search + bsk_hits_top, bsk_result_sets_reuse / _counted -- over the objects
alive at that point, half of them `into` an object another entry made, and a few calls the library must refuse with BSK_ERR_ARG.
After EVERY step the device's result is compared with the model: info, offsets, values, the counted flag, counts, totals, the pairs per
path (ops), both matrices and the round figures (compare), the hits and their top-n (search); the step's operands are fetched again and
must be what they were.  At the end of a program every object still alive is fetched once more: a later call must not have damaged an
earlier result.  Odd programs run on a second context of the same device.

A failure names its seed and step and prints the program up to there; `python -m tests.algebra_programs SEED` prints all of it.
tests/test_algebra_programs.py shows on the CPU what the campaign reaches and that this comparison catches each of eleven wrong models."""
import ctypes as C

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import algebra_programs as AP
from tests.test_gpu_counts import switches

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
KIND = {"nthash": L.NTHASH, "minimizer": L.MINIMIZER}
SLICE = 10  # programs per test, half a block of the campaign: 20 took 0.35-0.53 s on an MI355X, the slowest test of test_gpu_setops.py 0.42 s


@pytest.fixture(scope="module")
def second_engine():
    eng = S.Engine(0)
    yield eng
    eng.close()


def snap(s):
    o, v = s.fetch()
    return o, v, s.fetch_counts() if s.counted else None


def sets_record(s, operands, paths=False):
    inf, (o, v), counted = s.info(), s.fetch(), s.counted
    rec = dict(n_sets=inf["n_sets"], n_values=inf["n_values"], offsets=o, values=v, counted=counted, counts=s.fetch_counts() if counted else None,
               totals=s.totals(), operands={i: snap(x) for i, x in operands.items()})
    if paths:
        rec["paths"] = s.plan()["n_by_path"]
    return rec


class Run:
    """one program on one engine: the device side of algebra_programs.apply"""

    def __init__(self, engine, other, prog):
        self.eng, self.other, self.prog = engine, other, prog
        self.live, self.cmps, self.tops = {}, {}, {}
        self.batch = self.res = None

    def sketch(self, step):
        """the sketch step's result and every read's values: what the model is made of"""
        self.batch = self.eng.batch(step["reads"])
        self.res = self.eng.run(self.batch, self.eng.params(KIND[step["sketch"]], step["k"], w=step["w"]))
        return [self.res.read(i)[1] for i in range(len(step["reads"]))]

    def result_sets(self, step, into):
        with switches(self.eng, ("BSK_SETS_NO_SMALL",) if step["no_small"] and not step["counted"] else ()):
            if step["counted"]:
                return self.res.counted_sets(step["whole"], step["scale"], into=into)
            if into is None:
                return self.res.device_sets(step["whole"], step["scale"])
            h = C.c_void_p(into.h.value)
            rc = self.eng.lib.bsk_result_sets_reuse(self.eng.ctx, self.res.h, int(step["whole"]), step["scale"], C.byref(h))
            into.h = h if h.value else None
            assert rc == L.OK, rc
            return into

    def refused(self, step):
        lib, ctx, a = self.eng.lib, self.eng.ctx, self.live[step["a"]]
        slot = C.c_void_p(self.live[step["into"]].h.value) if step["into"] is not None else C.c_void_p()
        before, what, extra = slot.value, step["what"], None
        ns = a.info()["n_sets"]
        if what == "into is an operand":
            rc = lib.bsk_sets_op(ctx, a.h, self.live[step["b"]].h, L.SETOP_UNION, C.byref(slot))
        elif what == "set numbers mismatched":
            extra = self.eng.sets_from_arrays(np.arange(ns + 2, dtype=U64), np.arange(ns + 1, dtype=U64))  # one set more than a, and not one
            rc = lib.bsk_sets_op(ctx, a.h, extra.h, L.SETOP_UNION, C.byref(slot))
        elif what == "operand of the other engine":
            extra = self.other.sets_from_arrays(np.arange(ns + 1, dtype=U64), np.arange(ns, dtype=U64))
            rc = lib.bsk_sets_op(ctx, a.h, extra.h, L.SETOP_UNION, C.byref(slot))
        elif what == "filter_counts of uncounted sets":
            rc = lib.bsk_sets_filter_counts(ctx, a.h, 1, AP.SAT, C.byref(slot))
        elif what == "fetch_counts of uncounted sets":
            buf = np.zeros(a.info()["n_values"] + 1, U32)
            rc = lib.bsk_sets_fetch_counts(ctx, a.h, 0, ns, buf.ctypes.data, buf.size)
        elif what == "bottom(0)":
            rc = lib.bsk_sets_bottom(ctx, a.h, 0, C.byref(slot))
        else:
            assert what == "min_count of 0", what
            rc = lib.bsk_sets_filter_counts(ctx, a.h, 0, 5, C.byref(slot))
        if extra is not None:
            extra.close()
        ids = dict.fromkeys(step[x] for x in ("a", "b", "into") if step[x] is not None)
        return dict(rc="ERR_ARG" if rc == L.ERR_ARG and slot.value == before else "rc %d, *out %s -> %s" % (rc, before, slot.value),
                    operands={i: snap(self.live[i]) for i in ids})

    def step(self, step):
        k, live = step["kind"], self.live
        if k == "refused":
            return self.refused(step)
        into = live.get(step["out"]) if step.get("into") else None
        paths = k in ("op", "op_counted")
        if k == "load":
            r = self.eng.sets_from_arrays(step["offsets"], step["values"]) if step["counts"] is None else \
                self.eng.sets_from_arrays_counted(step["offsets"], step["values"], step["counts"])
            ops = []
        elif k in ("sketch", "result_sets"):
            r, ops = self.result_sets(step, into), []
        elif k == "op":
            r, ops = live[step["a"]].op(live[step["b"]], step["op"], into), [step["a"], step["b"]]
        elif k == "op_counted":
            r, ops = live[step["a"]].op_counted(live[step["b"]], step["op"], into), [step["a"], step["b"]]
        elif k == "reduce":
            r, ops = live[step["a"]].reduce(step["groups"], step["m"], into), [step["a"]]
        elif k == "filter":
            r, ops = live[step["a"]].filter_counts(step["lo"], step["hi"], into), [step["a"]]
        elif k == "bottom":
            r, ops = live[step["a"]].bottom(step["n"], into), [step["a"]]
        elif k == "compare":
            a, b = live[step["a"]], live[step["b"]]
            c = a.compare(b, step["limit"], reuse=self.cmps.get(step["cmp"]))
            self.cmps[step["cmp"]] = c
            inf, pl, (sh, tt) = c.info(), c.plan(), c.fetch()
            return dict(n_a=inf["n_a"], n_b=inf["n_b"], limit=inf["limit"], shared=sh, total=tt, figures=(pl["tiles"], pl["rounds"], pl["max_rounds"]),
                        operands={i: snap(live[i]) for i in (step["a"], step["b"])})
        else:
            assert k == "search", k
            ix = live[step["a"]].index()
            hits = ix.search(live[step["q"]], min_shared=step["min_shared"])
            inf, (o, t, s) = hits.info(), hits.fetch()
            rec = dict(n_queries=inf["n_queries"], n_hits=inf["n_hits"], offsets=o, targets=t, shared=s,
                       operands={i: snap(live[i]) for i in (step["a"], step["q"])})
            if step["top"]:
                top = hits.top(step["top"], reuse=self.tops.get(step["hits"]))
                self.tops[step["hits"]] = top
                rec["top_offsets"], rec["top_targets"], rec["top_shared"] = top.fetch()
            hits.close()
            ix.close()
            return rec
        live[step["out"]] = r
        rec = sets_record(r, {i: live[i] for i in ops}, paths)
        if not step.get("keep", True):
            live.pop(step["out"]).close()
        return rec

    def end(self):
        return dict(pool={i: snap(s) for i, s in self.live.items()}, compares={i: tuple(c.fetch()) for i, c in self.cmps.items()},
                    tops={i: tuple(h.fetch()) for i, h in self.tops.items()})

    def close(self):
        for pool in (self.live, self.cmps, self.tops):
            for x in pool.values():
                x.close()
        for x in (self.res, self.batch):
            if x is not None:
                x.close()


def run_program(engine, other, seed):
    prog, want = AP.program_and_records(seed)
    run = Run(engine, other, prog)
    try:
        sk = [s for s in prog if s["kind"] == "sketch"]
        if sk:
            want = AP.run_model(prog, read_values=run.sketch(sk[0]))  # (the generator's records stand on stand-in values)
        for i, step in enumerate(prog):
            diff = AP.same(want[i], run.step(step))
            assert not diff, AP.message(seed, i, prog, diff)
        diff = AP.same(want[-1], run.end())
        assert not diff, AP.message(seed, len(prog) - 1, prog, ["at the end of the program"] + diff)
    finally:
        run.close()


@pytest.mark.parametrize("part", range(AP.PER_BLOCK // SLICE))
@pytest.mark.parametrize("block", range(AP.BLOCKS))
def test_algebra_programs(engine, second_engine, block, part):
    for n, seed in enumerate(AP.seeds(block)[part * SLICE:(part + 1) * SLICE]):
        engines = (engine, second_engine) if (part * SLICE + n) % 2 == 0 else (second_engine, engine)
        run_program(*engines, seed)
