"""GPU: every capped grid of the sets side through its grid-stride loop (BSK_GRID_CAP; DESIGN.md "Switches").

On an MI355X a launch of 256-item workgroups at 16 per CU takes a second trip of its loop beyond a million items, so at the shapes of
the other suites most of these kernels never take one.  BSK_GRID_CAP=N gives every such launch at most N workgroups; this file runs
the entries at caps 1 (one workgroup walks everything: as many trips as blocks) and 3 (an odd stride, the blocks interleave) over shapes
of 600 sets -- 2 x 256 + 64 + 24: three trips of a per-set loop at cap 1, the last of one full wavefront and a partial one -- and more
than 3 x 256 x 2 values, edges or records.

Every call is compared exactly with the CPU model its own suite uses, and its record -- every array, info() and the plan figures -- must
be the record of the same call with the switch unset.  The models and generators are the existing ones (tests/*_cases.py,
tests/algebra_programs.py); nothing is modelled here.

Not vacuous: around every entry call the test reads bsk_ctx_grid_stats.  With the switch unset no grid of these shapes is cut (but the
1 444 tiles of the 600 x 600 comparison, which outnumber four workgroups per CU: counted, exactly); at cap 1
every grid the call sized is cut, except the ones listed with the call -- launches whose work is, by the shape the case is about, no
more than one workgroup.  UNCUT names every such site, the kernels behind it and the reason; a call passes the names that apply to it
and the count must be exactly their number."""
import contextlib
import ctypes as C
import functools
import os
import time

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import algebra_programs as AP
from tests import cluster_cases as CL
from tests import compare_cases as CC
from tests import compare_counted_cases as CW
from tests import counts_cases as CN
from tests import neighbor_cases as NC
from tests import search_cases as SR
from tests import setops_cases as SO
from tests import sets_cases as ST
from tests.test_gpu_hits_top import branches, crafted, one_pass, parse_plan

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
GRID_CAPS = (1, 3)
N = 600  # sets, nodes, queries: 2 x 256 + 64 + 24
LOOPS = 3 * 256 * 2  # values, edges, records: above it a launch of 256-item workgroups loops at cap 3 too
SO_CAPS, CMP_CAPS = SO.read_caps(), CC.read_caps()

# The grids that stay whole at cap 1: site -> (kernels, why the work is one workgroup by the case's construction).
UNCUT = {
    "heads of one set": ("k_mark_heads", "a whole-batch call makes ONE set: one head to mark"),
    "offsets of one set": ("k_new_offsets", "a whole-batch call makes ONE set: two offsets"),
    "group offsets": ("k_rd_goff", "bsk_sets_reduce over about 70 groups: 71 offsets"),
    "reduced offsets": ("k_rd_offsets", "bsk_sets_reduce over about 70 groups: 71 offsets"),
    "few records: keys": ("k_nb_keys", "the upper triangle of 33 x 17 sets keeps 136 pairs, 112 under a limit of 7: one workgroup's"),
    "few records: place": ("k_nb_place", "the upper triangle of 33 x 17 sets keeps 136 pairs, 112 under a limit of 7: one workgroup's"),
    "few hits: check": ("k_cl_check", "a 257-node generator of tests/cluster_cases.py with at most 256 hits: no or one edge, the upper form of a path or star, the sparse ones"),
    "few hits: edges": ("k_cl_edges, k_cl_hook, k_cl_mis_scan, k_cl_assign", "the same generators: one grid serves every edge kernel of a call"),
}


# ---- the switch, the counter, the comparison ----
@contextlib.contextmanager
def environment(env):
    """the variables of env set (a value of None: unset) for the block; what they held before comes back after it"""
    before = {k: os.environ.get(k) for k in env}

    def put(values):
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    put(env)
    try:
        yield
    finally:
        put(before)


@contextlib.contextmanager
def switches(engines, env):
    engines = engines if isinstance(engines, (tuple, list)) else (engines,)
    try:
        with environment(env):
            for e in engines:
                e.reload_options()
            yield
    finally:
        for e in engines:
            e.reload_options()


def grid_stats(engine):
    out = (C.c_uint64 * 2)()
    assert engine.lib.bsk_ctx_grid_stats(engine.ctx, out) == L.OK
    return int(out[0]), int(out[1])


class Probe:
    """the grids sized and cut around every entry call of one pass over a case list"""

    def __init__(self, engine, cap):
        self.engine, self.cap, self.sized, self.cut, self.calls = engine, cap, 0, 0, 0

    def __call__(self, what, call, uncut=(), natural=0):
        """natural: the grids of the call that the device's own cap cuts, switch or no switch (one case has such a grid)"""
        assert all(u in UNCUT for u in uncut), uncut
        s0, c0 = grid_stats(self.engine)
        out = call()
        s1, c1 = grid_stats(self.engine)
        sized, cut = s1 - s0, c1 - c0
        self.sized, self.cut, self.calls = self.sized + sized, self.cut + cut, self.calls + 1
        assert sized > 0, (what, "the call sized no grid through the helper")
        if self.cap is None:
            assert cut == natural, (what, sized, cut, natural, "grids of this shape cut with the switch unset")
        elif self.cap == 1:
            assert sized - cut == len(uncut), (what, "grids sized %d, cut %d, allowed whole %d %s" % (sized, cut, len(uncut), list(uncut)))
        return out


def run_cases(engine, name, cases, env=None):
    """every case with the switch unset, then at every cap: the model inside the case, the record against the unset one's"""
    records = {}
    for cap in (None,) + GRID_CAPS:
        more = dict(env or {}, BSK_GRID_CAP=None if cap is None else str(cap))
        t0 = time.perf_counter()
        with switches(engine, more):
            probe = Probe(engine, cap)
            got = [case(engine, probe) for case in cases]
        took = time.perf_counter() - t0
        records[cap] = got
        assert probe.calls and (cap is None or probe.cut > 0), (name, cap, "nothing was cut")
        print("%s, %s: %d calls, %d grids sized, %d cut, %.3f s" % (name, "switch unset" if cap is None else "cap %d" % cap, probe.calls, probe.sized, probe.cut, took))
    for cap in GRID_CAPS:
        for i, (want, got) in enumerate(zip(records[None], records[cap])):
            diff = AP.same(want, got)
            assert not diff, (name, "cap %d, case %d differs from the same call with the switch unset" % (cap, i), diff)


def sets_record(s, with_paths=False):
    inf, (o, v) = s.info(), s.fetch()
    rec = dict(info=inf, offsets=o, values=v, counted=s.counted, counts=s.fetch_counts() if s.counted else None)
    if with_paths:
        rec["plan"] = s.plan()
    return rec


def model_sets(rec, want, what):
    o, v, c = want
    assert rec["info"] == dict(n_sets=len(o) - 1, n_values=len(v)), what
    assert np.array_equal(rec["offsets"], o) and np.array_equal(rec["values"], v), what
    assert rec["counted"] == (c is not None) and (c is None or (rec["counts"].dtype == U32 and np.array_equal(rec["counts"], c))), what


# ---- sets.hip: the sets of a sketch result, its compact and narrow fetches ----
@functools.lru_cache(None)
def _reads():
    rng = np.random.default_rng(600)
    reads = [ST.rand_read(rng, int(rng.integers(0, 85))) for _ in range(N)]  # at most 64 values of k = 21: the small path unless the switch forbids it
    reads[5] = reads[6] = reads[7]  # (whole-batch counts above one)
    return reads


def d2h(engine, ptr, n, dt):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    a = np.empty(n, dt)
    if n:
        assert ptr
        engine.sync()
        assert hip.hipMemcpy(a.ctypes.data, ptr, a.nbytes, 2) == 0
    return a


def fetch_case_of(res, n, plain):
    """bsk_result_compact and bsk_result_fetch_narrow (all of it, and a range) of one result against its full fetch `plain`"""
    narrow_pos = None if plain[3] is None else ((plain[3] & U32(0x7FFF)) | ((plain[3] >> U32(16)) & U32(0x8000))).astype(np.uint16)

    def run(engine, probe):
        po, ph, pp, nt = probe("compact", lambda: res.compact())
        rec = dict(n_tuples=nt, offsets=d2h(engine, po, n + 1, U64), hash=d2h(engine, ph, nt, U64), pos=d2h(engine, pp, nt, U32) if pp else None)
        assert nt == len(plain[2]) and np.array_equal(rec["offsets"], plain[0]) and np.array_equal(rec["hash"], plain[2])
        assert (rec["pos"] is None) == (plain[3] is None) and (plain[3] is None or np.array_equal(rec["pos"], plain[3]))
        o, st, h, p = probe("fetch_narrow", lambda: res.fetch_narrow())
        rec.update(narrow_offsets=o, narrow_status=st, narrow_hash=h, narrow_pos=p)
        assert o.dtype == U32 and np.array_equal(o, plain[0]) and np.array_equal(st, plain[1]) and np.array_equal(h, plain[2])
        assert (p is None) == (narrow_pos is None) and (p is None or (p.dtype == np.uint16 and np.array_equal(p, narrow_pos)))
        first, count = 70, 333  # a range that starts and ends inside a workgroup's 256 sequences
        o, st, h, p = probe("fetch_narrow, a range", lambda: res.fetch_narrow(first, count))
        rec.update(range_offsets=o, range_hash=h, range_pos=p)
        a, e = int(plain[0][first]), int(plain[0][first + count])
        assert np.array_equal(o.astype(U64), plain[0][first:first + count + 1] - plain[0][first]) and np.array_equal(h, plain[2][a:e])
        assert p is None or np.array_equal(p, narrow_pos[a:e])
        return rec
    return run


def test_sets_of_a_sketch_result(engine, oracle):
    """bsk_result_sets, _sets_counted and _sets_reuse per sequence and for the whole batch, at scale 1 and 3, on the small path and under
    BSK_SETS_NO_SMALL on the general one; bsk_result_compact and bsk_result_fetch_narrow of the same result"""
    case = dict(kind="nthash", pk=dict(k=21), reads=_reads())
    vals = ST.values_of(oracle, case)
    assert max(len(v) for v in vals) <= ST.SMALL_CAP and sum(len(v) for v in vals) > 4 * LOOPS
    batch = engine.batch(case["reads"])
    res = engine.run(batch, engine.params(L.NTHASH, 21))
    plain = res.fetch()  # (the full fetch, before any cap: what the two device-side fetches are held to, beside the oracle)
    assert np.array_equal(np.diff(plain[0]).astype(np.int64), [len(v) for v in vals])
    assert all(np.array_equal(plain[2][int(plain[0][i]):int(plain[0][i + 1])], v) for i, v in enumerate(vals))
    one_set = ("heads of one set", "offsets of one set")

    def sets_case(whole, scale):
        def run(engine, probe):
            what = ("sets", whole, scale)
            uncut = one_set if whole else ()
            small = not whole and "BSK_SETS_NO_SMALL" not in os.environ
            rec = {}
            s = probe(what, lambda: res.device_sets(whole, scale), () if small else uncut)
            rec["plain"] = sets_record(s)
            model_sets(rec["plain"], ST.ref_sets(vals, scale, whole) + (None,), what)
            c = probe(what + ("counted",), lambda: res.counted_sets(whole, scale), uncut)
            rec["counted"] = sets_record(c)
            model_sets(rec["counted"], CN.ref_counted(vals, scale, whole), what)
            assert np.array_equal(c.totals(), CN.ref_totals(CN.ref_counted(vals, scale, whole)))
            h = C.c_void_p(c.h.value)  # bsk_result_sets_reuse into the counted object: its counts go
            rc = probe(what + ("reuse",), lambda: engine.lib.bsk_result_sets_reuse(engine.ctx, res.h, int(whole), scale, C.byref(h)), () if small else uncut)
            c.h = h if h.value else None
            assert rc == L.OK
            rec["reused"] = sets_record(c)
            model_sets(rec["reused"], ST.ref_sets(vals, scale, whole) + (None,), what + ("reuse",))
            s.close()
            c.close()
            return rec
        return run

    fetch_case = fetch_case_of(res, len(vals), plain)
    cases = [sets_case(whole, scale) for whole in (False, True) for scale in (1, 3)]
    run_cases(engine, "result sets", cases + [fetch_case])
    run_cases(engine, "result sets, BSK_SETS_NO_SMALL", cases, env={"BSK_SETS_NO_SMALL": "1"})
    run_cases(engine, "result fetches, BSK_NO_GROUP_GATHER", [fetch_case], env={"BSK_NO_GROUP_GATHER": "1"})  # k_compact and k_gather_narrow
    res.close()
    batch.close()


def test_fetches_of_a_unit_row_result(engine, oracle):
    """the same two fetches of a k_minimizer_ring result -- unit rows, positions and strands: k_gather_groups' other layout, the u16
    positions of the narrow fetch -- and the per-sequence sets of such a result"""
    rng = np.random.default_rng(601)
    reads = [ST.rand_read(rng, int(rng.choice((200, 250, 290)))) for _ in range(N)]
    reads[64], reads[65], reads[127] = "", "ACGT", ""
    case = dict(kind="minimizer", pk=dict(k=21, w=11), reads=reads)
    vals = ST.values_of(oracle, case)
    batch = engine.batch(reads)
    res = engine.run(batch, engine.params(L.MINIMIZER, 21, w=11))
    assert "k_minimizer_ring" in res.plan()["kernel"], res.plan()
    plain = res.fetch()
    assert plain[3] is not None and all(np.array_equal(plain[2][int(plain[0][i]):int(plain[0][i + 1])], v) for i, v in enumerate(vals))

    def sets_case(engine, probe):
        s = probe("sets of unit rows", lambda: res.device_sets(False, 1))
        rec = sets_record(s)
        model_sets(rec, ST.ref_sets(vals, 1, False) + (None,), "sets of unit rows")
        s.close()
        return rec

    fetch_case = fetch_case_of(res, N, plain)
    run_cases(engine, "unit rows", [fetch_case, sets_case])
    run_cases(engine, "unit rows, BSK_NO_GROUP_GATHER", [fetch_case, sets_case], env={"BSK_NO_GROUP_GATHER": "1"})
    res.close()
    batch.close()


# ---- setops.hip and counts.hip ----
CLASS_WEIGHTS = (0.05, 0.15, 0.10, 0.12, 0.13, 0.15, 0.15, 0.15)


@functools.lru_cache(None)
def _collections():
    """two collections of 600 sets and one of one set: sizes across every class of algebra_programs.size_classes(), values drawn so that
    the sets of a pair share some; counts for the counted entries"""
    rng = np.random.default_rng(0x600)
    classes = AP.size_classes()
    pool = rng.permutation(np.unique(rng.integers(0, SO.MAX64, size=9000, dtype=U64, endpoint=True)))
    w = np.array(CLASS_WEIGHTS)

    def draw(n, weights):
        pick = rng.choice(len(weights), size=n, p=weights / weights.sum())
        sizes = [int(rng.integers(classes[c][0], classes[c][1] + 1)) for c in pick]
        sets = [np.sort(rng.choice(pool[:max(4 * s, 48)], size=s, replace=False)).astype(U64) for s in sizes]
        o, v = SO.collection(sets)
        return o, v, AP._counts(rng, len(v))

    a, b = draw(N, w), draw(N, w)
    one = draw(1, np.array([0, 0, 0, 0, 0, 1.0, 0, 0]))  # about 515 values: against it the smaller sets take the wave kernel, the larger ones tiles
    for x in (a, b):
        assert {AP.size_class(int(s)) for s in np.diff(x[0])} == set(range(len(classes))), "every size class"
    return a, b, one


def _tiles(a_offs, b_offs):
    t = SO.pair_t(a_offs, b_offs)
    return int((-(-t[t > SO_CAPS["SO_WAVE_CAP"]] // SO_CAPS["SO_TILE"])).sum())


def test_set_algebra(engine):
    """bsk_sets_op (four ops) and bsk_sets_op_counted (three) over 600 pairs and against the one-set operand, every path's pairs and
    tiles beyond one workgroup's"""
    a, b, one = _collections()
    M = AP.Model()
    for x, y in ((a, b), (a, one)):
        paths = SO.path_counts(x[0], y[0], SO_CAPS)
        # k_so_group 16 pairs a workgroup (none against the one large set), k_so_wave 4, k_so_tile 4 tiles, k_so_cuts 256 tiles, k_so_list 256 pairs
        assert (paths[0] > 3 * 16 or y is one) and paths[1] > 3 * 4 and _tiles(x[0], y[0]) > 2 * 256 and int(x[0][-1]) + int(y[0][-1]) > LOOPS, (paths, _tiles(x[0], y[0]))
    da, db, d1 = (engine.sets_from_arrays_counted(*x) for x in (a, b, one))
    pa, pb, p1 = (engine.sets_from_arrays(*x[:2]) for x in (a, b, one))

    def op_case(x, y, dx, dy, op, counted):
        want = M.op_counted(x, y, op) if counted else M.op((x[0], x[1], None), (y[0], y[1], None), op)  # (once: the three passes share it)
        paths = (CN if counted else SO).path_counts(x[0], y[0], SO_CAPS)

        def run(engine, probe):
            what = ("op_counted" if counted else "op", op, len(y[0]) - 1)
            r = probe(what, lambda: dx.op_counted(dy, op) if counted else dx.op(dy, op))
            rec = sets_record(r, with_paths=True)
            model_sets(rec, want, what)
            assert rec["plan"]["n_by_path"] == paths, what
            r.close()
            return rec
        return run

    cases = [op_case(a, y, pa, py, op, False) for y, py in ((b, pb), (one, p1)) for op in SO.OPS]
    cases += [op_case(a, y, da, dy, op, True) for y, dy in ((b, db), (one, d1)) for op in CN.OPS]
    cases += [op_case(one, b, d1, db, CN.ADD, True), op_case(a, (b[0], b[1], None), da, pb, CN.ADD, True)]  # the one set as a; an uncounted operand counts 1
    run_cases(engine, "set algebra", cases)
    for x in (da, db, d1, pa, pb, p1):
        x.close()


def test_reduce_filter_totals_bottom(engine):
    """bsk_sets_reduce over about 70 groups (a number of members, and all of them), bsk_sets_filter_counts, bsk_sets_totals and
    bsk_sets_sumsq, bsk_sets_bottom of 1, 17 and 129 values, counted and not"""
    a, b, _ = _collections()
    M = AP.Model()
    rng = np.random.default_rng(70)
    groups = np.concatenate([[0, 0], np.sort(rng.choice(np.arange(1, N), size=68, replace=False)), [N, N]]).astype(U64)  # an empty group first and last
    assert len(groups) - 1 == 71 and int(a[0][-1]) > 3 * SO_CAPS["RD_CHUNK"]
    da, pa = engine.sets_from_arrays_counted(*a), engine.sets_from_arrays(*a[:2])
    plain = (a[0], a[1], None)
    csets = SO.split(a[0], a[2])

    def reduce_case(m):
        want = M.reduce(plain, groups, m)

        def run(engine, probe):
            r = probe(("reduce", m), lambda: pa.reduce(groups, m), ("group offsets", "reduced offsets"))
            rec = sets_record(r, with_paths=True)
            model_sets(rec, want, ("reduce", m))
            r.close()
            return rec
        return run

    def filter_case(lo, hi):
        want = M.filter(a, lo, CN.SAT if hi is None else hi)

        def run(engine, probe):
            r = probe(("filter", lo, hi), lambda: da.filter_counts(lo, hi))
            rec = sets_record(r)
            model_sets(rec, want, ("filter", lo, hi))
            rec["totals"] = probe(("totals of the filtered",), lambda: r.totals())
            assert np.array_equal(rec["totals"], M.totals(want))
            r.close()
            return rec
        return run

    def totals_case(engine, probe):
        rec = dict(counted=probe("totals", lambda: da.totals()), plain=probe("totals, uncounted", lambda: pa.totals()),
                   sumsq=probe("sumsq", lambda: da.sumsq()), sumsq_plain=probe("sumsq, uncounted", lambda: pa.sumsq()))
        assert np.array_equal(rec["counted"], M.totals(a)) and np.array_equal(rec["plain"], M.totals(plain))
        assert np.array_equal(rec["sumsq"], CW.ref_sumsq(csets)) and np.array_equal(rec["sumsq_plain"], np.diff(a[0]))
        return rec

    def bottom_case(n, counted):
        src = a if counted else plain
        want = M.bottom(src, n)

        def run(engine, probe):
            r = probe(("bottom", n, counted), lambda: (da if counted else pa).bottom(n))
            rec = sets_record(r)
            model_sets(rec, want, ("bottom", n, counted))
            r.close()
            return rec
        return run

    cases = [reduce_case(m) for m in (1, 2, SO.MEMBERS_ALL)] + [filter_case(1, None), filter_case(2, 4), filter_case(3, 3), totals_case]
    cases += [bottom_case(n, counted) for n in (1, 17, 129) for counted in (False, True)]
    run_cases(engine, "reduce, filter, totals, bottom", cases)
    da.close()
    pa.close()


# ---- compare.hip ----
def _compare_record(c):
    inf, pl, (sh, tt) = c.info(), c.plan(), c.fetch()
    rec = dict(info=inf, shared=sh, total=tt, plan=pl)
    if c.weighted:
        rec["dot"], rec["min_sum"] = c.fetch_weights()
    return rec


def _hits_record(h):
    o, t, s = h.fetch()
    return dict(info=h.info(), offsets=o, target=t, shared=s, total=h.fetch_totals() if h.has_totals() else None, plan=h.plan())


def test_compare_and_neighbors(engine):
    """bsk_sets_compare, _compare_counted and bsk_sets_neighbors on 33 x 17 and 33 x 33 sets (6 and 9 tiles), limits 0 and 7; the
    neighbours plain, upper and with a first room of 8 records, where the second run's k_nb_keys and k_nb_place loop too"""
    R, COLS = CMP_CAPS["CMP_ROWS"], CMP_CAPS["CMP_COLS"]
    A, B, _ = CC.tile_edges(R, COLS)
    A, B = A[:33], B[:33]
    CA, CB = CW.attach(A, 1, 9, 33), CW.attach(B, 1, 9, 34)
    dA = engine.sets_from_arrays_counted(*CC.collection(A), CW.flat(CA))
    dBs = {nb: engine.sets_from_arrays_counted(*CC.collection(B[:nb]), CW.flat(CB[:nb])) for nb in (17, 33)}
    assert {CC.n_tiles(33, nb, CMP_CAPS) for nb in (17, 33)} == {6, 9}
    refs = {(nb, limit): CC.ref_compare(A, B[:nb], limit) for nb in (17, 33) for limit in (0, 7)}

    def compare_case(nb, limit, weighted):
        want = CW.ref_compare(A, CA, B[:nb], CB[:nb], limit) if weighted else refs[(nb, limit)]
        figures = CC.plan_figures(A, B[:nb], limit, CMP_CAPS)

        def run(engine, probe):
            what = ("compare_counted" if weighted else "compare", nb, limit)
            c = probe(what, lambda: dA.compare_counted(dBs[nb], limit) if weighted else dA.compare(dBs[nb], limit))
            rec = _compare_record(c)
            assert rec["info"] == dict(n_a=33, n_b=nb, limit=limit), what
            assert np.array_equal(rec["shared"], want[0]) and np.array_equal(rec["total"], want[1]), what
            assert not weighted or (np.array_equal(rec["dot"], want[2]) and np.array_equal(rec["min_sum"], want[3])), what
            assert (rec["plan"]["tiles"], rec["plan"]["rounds"], rec["plan"]["max_rounds"]) == tuple(int(x) for x in figures), (what, rec["plan"])
            c.close()
            return rec
        return run

    def neighbors_case(nb, limit, upper, runs):
        want = NC.filter_matrices(*refs[(nb, limit)], upper=upper)
        kept = len(want[1])
        few = ("few records: keys", "few records: place") if kept <= 256 else ()
        assert kept > 8, (nb, limit, upper, kept)

        def run(engine, probe):
            what = ("neighbors", nb, limit, upper, runs)
            h = probe(what, lambda: dA.neighbors(dBs[nb], limit, upper=upper), few)
            rec = _hits_record(h)
            assert NC.same((rec["offsets"], rec["target"], rec["shared"], rec["total"]), want), what
            fig = NC.plan_figures(rec["plan"]["plan"])
            assert (fig["tiles"], fig["skipped"]) == NC.expected_tiles(33, nb, upper, CMP_CAPS) and fig["runs"] == runs and fig["rounds"] >= fig["tiles"], (what, fig)
            h.close()
            return rec
        return run

    shapes = [(nb, limit) for nb in (17, 33) for limit in (0, 7)]
    run_cases(engine, "compare", [compare_case(nb, limit, w) for nb, limit in shapes for w in (False, True)])
    run_cases(engine, "neighbors", [neighbors_case(nb, limit, upper, 1) for nb, limit in shapes for upper in (False, True)])
    run_cases(engine, "neighbors, BSK_NB_ROOM=8", [neighbors_case(nb, limit, upper, 2) for nb, limit in shapes for upper in (False, True)], env={"BSK_NB_ROOM": "8"})
    for x in [dA] + list(dBs.values()):
        x.close()


def test_neighbors_of_600_sets(engine):
    """600 sets of three values, set i = {3 (i // 2), + 1, + 2}, against themselves: 1 444 tiles, every set meets itself and one other --
    1 200 records, more than three workgroups of k_nb_keys and k_nb_place; upper: the 300 pairs (2 m, 2 m + 1)"""
    i = np.arange(N, dtype=np.int64)
    offs = np.arange(N + 1, dtype=U64) * U64(3)
    vals = (3 * np.repeat(i // 2, 3) + np.tile(np.arange(3), N)).astype(U64)
    s = engine.sets_from_arrays(offs, vals)
    tiles = CC.n_tiles(N, N, CMP_CAPS)
    assert tiles == 38 * 38
    # the one grid of this file that the device's own cap cuts: 1 444 tiles against CMP_BLOCKS_PER_CU = 4 workgroups per CU (1 024 on 256 CUs)
    natural = int(tiles > one_pass()["cus"] * CMP_CAPS["CMP_BLOCKS_PER_CU"])

    def full(engine, probe):
        h = probe("neighbors 600 x 600", lambda: s.neighbors(), natural=natural)
        rec = _hits_record(h)
        assert rec["info"] == dict(n_queries=N, n_hits=2 * N) and 2 * N > 3 * 256
        assert np.array_equal(rec["offsets"], 2 * np.arange(N + 1, dtype=U64)) and np.array_equal(rec["target"].reshape(N, 2), np.stack([i - i % 2, i - i % 2 + 1], 1))
        assert (rec["shared"] == 3).all() and (rec["total"] == 3).all()
        fig = NC.plan_figures(rec["plan"]["plan"])
        assert (fig["tiles"], fig["skipped"]) == NC.expected_tiles(N, N, False, CMP_CAPS) == (tiles, 0) and fig["runs"] == 1, fig
        h.close()
        return rec

    def upper(engine, probe):
        h = probe("neighbors 600 x 600, upper", lambda: s.neighbors(upper=True), natural=natural)
        rec = _hits_record(h)
        assert rec["info"] == dict(n_queries=N, n_hits=N // 2)
        assert np.array_equal(np.diff(rec["offsets"].astype(np.int64)), (i % 2 == 0).astype(np.int64)) and np.array_equal(rec["target"], np.arange(1, N, 2, dtype=U32))
        assert (rec["shared"] == 3).all() and (rec["total"] == 3).all()
        fig = NC.plan_figures(rec["plan"]["plan"])
        assert (fig["tiles"], fig["skipped"]) == NC.expected_tiles(N, N, True, CMP_CAPS) and fig["skipped"] == 38 * 37 // 2, fig
        h.close()
        return rec

    def dense(engine, probe):  # the matrix of the same operands: 1 444 tiles of k_cmp_tile
        c = probe("compare 600 x 600", lambda: s.compare(), natural=natural)
        rec = _compare_record(c)
        same = (i[:, None] // 2) == (i[None, :] // 2)
        assert np.array_equal(rec["shared"], np.where(same, 3, 0)) and np.array_equal(rec["total"], np.where(same, 3, 6)) and rec["plan"]["tiles"] == tiles
        c.close()
        return rec

    run_cases(engine, "neighbors of 600 sets", [full, upper, dense])
    s.close()


# ---- search.hip ----
@functools.lru_cache(None)
def _search_case():
    """test_gpu_hits_top's crafted queries, 600 of them: hit counts around every cap of bsk_hits_top, 24 queries beyond the LDS sort's
    keys (the sort path, and with shared counts of 1 .. 3 the search's large path), runs of queries without hits"""
    base = [0, 1, 5, 15, 16, 17, 40, 63, 64, 65, 130, 0, 2, 16, 18, 33, 300, 1, 0, 17, 64, 9, 1023, 1024, 1025]
    counts = (base * (N // len(base)))[:N - 4] + [2000, 0, 1500, 1025]
    assert len(counts) == N
    tg, qs = crafted(counts, "mixed", seed=600)
    want = SR.ref_search(*tg, *qs)
    assert list(np.diff(want[0])) == counts and len(tg[0]) - 1 >= N
    return tg, qs, want


def test_index_search_and_top(engine):
    """bsk_index_build and bsk_index_search over 600 queries on both paths, bsk_hits_top of 1, 17 and 2 000 on the group, wave (64
    queries a wavefront step under the cap) and sort paths, bsk_hits_from_host, bsk_sets_fetch_narrow"""
    tg, qs, want = _search_case()
    n_large = int((SR.posting_sums(*tg, *qs) > SR.SR_CAP).sum())
    assert n_large > 3 * 4 and int(want[0][-1]) > LOOPS and int(tg[0][-1]) > LOOPS  # k_lg_emit: 4 large queries a workgroup
    dt, dq = engine.sets_from_arrays(*tg), engine.sets_from_arrays(*qs)
    tops = {n: SR.ref_top(*want, n) for n in (1, 17, 2000)}
    state = {}

    def build(engine, probe):
        ix = probe("index build", lambda: dt.index())
        state["ix"] = ix
        inf = ix.info()
        d = SR.directory(tg[1])
        assert inf["n_targets"] == len(tg[0]) - 1 and inf["n_postings"] == len(tg[1]) and inf["n_distinct"] == d["n_distinct"] and inf["max_bucket"] == d["max_bucket"], inf
        assert inf["n_distinct"] >= 512  # (k_ix_maxb walks 2^bits <= n_distinct buckets: more than one workgroup's)
        return {k: v for k, v in inf.items()}

    def search(engine, probe):
        hits = probe("search", lambda: state["ix"].search(dq))
        state["hits"] = hits
        rec = _hits_record(hits)
        assert NC.same((rec["offsets"], rec["target"], rec["shared"]), want) and rec["plan"]["n_large_queries"] == n_large > 0, rec["plan"]
        return rec

    def search_thresholds(engine, probe):
        kw = dict(min_shared=2, min_query_cov=0.3)
        h = probe("search, thresholds", lambda: state["ix"].search(dq, **kw))
        rec = _hits_record(h)
        assert NC.same((rec["offsets"], rec["target"], rec["shared"]), SR.ref_search(*tg, *qs, 2, 0.3, 0.0))
        h.close()
        return rec

    def top_case(n):
        def run(engine, probe):
            top = probe(("top", n), lambda: state["hits"].top(n))
            rec = _hits_record(top)
            assert NC.same((rec["offsets"], rec["target"], rec["shared"]), tops[n]) and rec["total"] is None, n
            got_n, got = parse_plan(top)
            b = branches(want[0], n)
            assert got_n == n and got == b and b["group"] > 3 * 16 and b["wave"] > 3 * 4, (n, got, b)
            assert (b["kernel"], b["sort"] > 3 * 4) == (("k_top_select", False) if n == 1 else ("k_top_lds", True)), b
            top.close()
            return rec
        return run

    def from_host(engine, probe):
        # bsk_hits_from_host launches nothing; the top of what it loaded does: the same hits by another way
        h = engine.hits_from_arrays(*want)
        top = probe("top of hits from the host", lambda: h.top(17))
        rec = _hits_record(top)
        assert NC.same((rec["offsets"], rec["target"], rec["shared"]), tops[17])
        top.close()
        h.close()
        return rec

    def narrow(engine, probe):
        o32, v = np.zeros(len(qs[0]), U32), np.zeros(len(qs[1]) + 1, U64)
        rc = probe("sets fetch_narrow", lambda: engine.lib.bsk_sets_fetch_narrow(engine.ctx, dq.h, o32.ctypes.data, v.ctypes.data, len(qs[1])))
        assert rc == L.OK and np.array_equal(o32.astype(U64), qs[0]) and np.array_equal(v[:-1], qs[1])
        return dict(offsets=o32, values=v)

    def close(engine, probe):
        state.pop("hits").close()
        state.pop("ix").close()
        return {}

    run_cases(engine, "index, search, top", [build, search, search_thresholds] + [top_case(n) for n in (1, 17, 2000)] + [from_host, narrow, close])
    dt.close()
    dq.close()


# ---- cluster.hip ----
@functools.lru_cache(None)
def _graphs():
    """every generator of cluster_cases.cases() with more than 256 nodes, and from the same generators a G(n, p) graph and a shuffled
    path of 600 nodes -> [(name, n, directed pairs)]"""
    out = [c for c in CL.cases() if c[1] > 256]
    extra = [("gnp_600", N, CL.gnp(N, 0.012, seed=100 + N), [(v, v) for v in range(0, N, 7)]), ("path_shuffled_600", N, CL.path(N, seed=N), [])]
    for name, n, edges, diag in extra:
        for form, pairs in CL.forms(edges).items():
            out.append((f"{name}-{form}", n, pairs + diag))
    assert len(out) == 3 * 12 and len(CL.forms(extra[0][2])["upper"]) > LOOPS
    return out


def _cluster_case(name, n, pairs, method, sname, seed):
    o, t, s = CL.csr(n, pairs)
    score = CL.scores(n, seed=seed)[sname]
    want, rounds = CL.ROUND_MODELS[method](n, o, t, score)
    assert CL.same(want, CL.MODELS[method](n, o, t, score)), (name, method, sname)
    edges, H = CL.n_offdiagonal(o, t), len(t)
    # bsk_hits_cluster sizes three grids: k_cl_check's over the hits (when there are any), one over the nodes, one over the hits again
    uncut = () if H > 256 else ("few hits: check", "few hits: edges") if H else ("few hits: edges",)
    kernels = "k_cl_mis" if method == "greedy" else "k_cl_hook+k_cl_jump"

    def run(engine, probe):
        what = (name, method, sname)
        hits = engine.hits_from_arrays(o, t, s)
        c = probe(what, lambda: hits.cluster(method, score), uncut)
        label, rep, offsets, members = c.fetch()
        rec = dict(info=c.info(), plan=c.plan(), label=label, rep=rep, offsets=offsets, members=members)
        assert rec["info"] == dict(n_items=n, n_clusters=len(want[1]), largest=int(want[4])), what
        assert CL.same((label, rep, offsets, members, rec["info"]["largest"]), want), what
        assert rec["plan"] == dict(plan=f"{kernels}, n={n} edges={edges} rounds={rounds}", rounds=rounds, edges=edges), (what, rec["plan"], rounds)
        c.close()
        hits.close()
        return rec
    return run


@pytest.mark.parametrize("method", CL.METHODS)
def test_clusters(engine, method):
    """every graph of more than 256 nodes under no score, random scores and few distinct ones (the class sort that breaks their ties)"""
    cases = [_cluster_case(name, n, pairs, method, sname, k) for k, (name, n, pairs) in enumerate(_graphs()) for sname in ("none", "random", "few")]
    run_cases(engine, "clusters, " + method, cases)


def test_clusters_of_the_long_path(engine):
    """the shuffled path of 4 096 nodes: 16 trips of every per-node loop at cap 1"""
    n = 4096
    pairs = CL.forms(CL.path(n, seed=4096))["upper"]
    run_cases(engine, "clusters, 4 096 nodes", [_cluster_case("path_shuffled_4096-upper", n, pairs, m, sname, 4096) for m in CL.METHODS for sname in ("none", "few")])


# ---- the two stateful campaigns ----
def test_algebra_programs_under_a_cap_of_one(engine):
    """the first programs of block 0 of tests/algebra_programs.py through test_gpu_algebra_fuzz's own run_program, every grid one workgroup"""
    from tests.test_gpu_algebra_fuzz import SLICE, run_program
    t0 = time.perf_counter()
    with switches(engine, {"BSK_GRID_CAP": "1"}):
        second = S.Engine(0)  # (created under the switch: it reads it)
        try:
            before = [grid_stats(e) for e in (engine, second)]
            for n, seed in enumerate(AP.seeds(0)[:SLICE]):
                run_program(*((engine, second) if n % 2 == 0 else (second, engine)), seed)
            after = [grid_stats(e) for e in (engine, second)]
        finally:
            second.close()
    cut = [a[1] - b[1] for a, b in zip(after, before)]
    print("algebra programs, cap 1: grids cut per context %s, %.3f s" % (cut, time.perf_counter() - t0))
    assert min(cut) > 0, cut


def test_sketch_programs_under_a_cap_of_one(engine, oracle):
    """the first programs of block 0 of tests/sketch_programs.py through test_gpu_sketch_programs' own run_program: every small pass
    around a sketch call (packing, binning, tiles, adoption of a class plan's parts, the fetches) in one workgroup.  What that file
    remembers of the seeds a context has run (for its own failure messages) is put back: these ran under a cap."""
    from tests import sketch_programs as SP
    from tests import test_gpu_sketch_programs as TSP
    t0 = time.perf_counter()
    history = {k: list(v) for k, v in TSP.HISTORY.items()}
    try:
        with switches(engine, {"BSK_GRID_CAP": "1"}):
            second = S.Engine(0)  # (created under the switch: it reads it)
            try:
                engines = (engine, second)
                before = [grid_stats(e) for e in engines]
                for n, seed in enumerate(SP.seeds(0)[:TSP.SLICE]):
                    TSP.run_program(engines[n % 2], n % 2, 0, seed, oracle)
                after = [grid_stats(e) for e in engines]
            finally:
                second.close()
    finally:
        TSP.HISTORY.clear()
        TSP.HISTORY.update(history)
    cut = [a[1] - b[1] for a, b in zip(after, before)]
    print("sketch programs, cap 1: grids cut per context %s, %.3f s" % (cut, time.perf_counter() - t0))
    assert min(cut) > 0, cut


# ---- the pipeline's hits sink: the one entry whose launches run on contexts of the library's own ----
def test_hits_sink_of_a_pipeline(engine):
    """hits_fetch_narrow (k_off_u32: the hits' offsets narrowed to u32 on the device) is reached from a BSK_SINK_HITS pipeline only, on its
    workers' contexts.  Those read BSK_GRID_CAP when the pipeline creates them; bsk_ctx_grid_stats cannot be asked about them, so here the
    cut is argued from the launch expressions: a chunk of 700 records is 701 offsets, three workgroups of 256 against a cap of one (and 44
    of k_sr_small, 3 of k_top_classes, ...).  Every chunk against test_gpu_pipeline_hits' own one_batch, made by the engine with the switch
    unset, and byte for byte against the pipeline with the switch unset."""
    from tests.test_gpu_pipeline_hits import K, W, assert_equals_batch, build_index, collect, make_case, one_batch
    n, chunk = 1500, 700
    assert chunk >= N and (chunk + 1 + 255) // 256 >= 3
    genomes, reads = make_case(n, 41, glen=4000)
    p = engine.params(L.MINIMIZER, K, w=W)
    with environment({"BSK_GRID_CAP": None}):
        engine.reload_options()
        ix = build_index(engine, genomes, p, 1)
        wants = {top_n: one_batch(engine, ix, reads, p, 1, top_n) for top_n in (0, 2)}
    assert int(wants[0][0][-1]) > n  # (reads of the shared halves have two targets)
    got = {}
    for cap in (None,) + GRID_CAPS:
        with environment({"BSK_GRID_CAP": None if cap is None else str(cap)}):
            for top_n in (0, 2):
                with S.Engine.pipeline_open(p, data=reads[0], offsets=reads[1], devices=[0], n_streams=2, chunk_records=chunk, sink=L.SINK_HITS, sets_scale=1,
                                            alphabet=L.ALPHA_DNA, host_checksum=True, search=ix, top_n=top_n) as pl:
                    chunks = collect(pl)
                assert [c["n"] for c in chunks] == [700, 700, 100], (cap, top_n)
                assert_equals_batch(chunks, wants[top_n], n)
                got[(cap, top_n)] = [{k: v for k, v in c.items() if k != "device"} for c in chunks]
    engine.reload_options()
    for cap in GRID_CAPS:
        for top_n in (0, 2):
            diff = AP.same(got[(None, top_n)], got[(cap, top_n)])
            assert not diff, (cap, top_n, diff)
    ix.close()
