"""GPU: every planned sketch kernel's unit loop through several tickets a wave (BSK_UNIT_GRID; DESIGN.md "Switches" and section 7).

On 256 CUs a batch of the other suites is one ticket per wave at most: what a wave carries from one unit to the next and from one ticket to
the next -- request-ahead registers, double LDS buffers, the list cursor of list_append, the slab overflow cursor, the re-take after a
successful ticket -- only runs at 10^7 reads.  BSK_UNIT_GRID=G gives every such launch min(G, its own grid) workgroups; tests/unit_trips.py
holds the cases (83 units of 64 reads, G = 1: one wave does everything in order, G = 3: three waves race for 11 or 21 tickets) and
tests/test_unit_trips.py holds them against the sources.

Per row and cap: the exact plan name of the atlas row, plan()["grid"] == G, bsk_ctx_unit_grid_stats moved and every grid sized was cut
(83 and, for the ASCII side launch, 28 units against 1 or 3 workgroups), k_minimizer_pk's BSK_TIMING line says whole tickets (tk 0) and
where the small ones start, EVERY read against the oracle's state machines on one fetch -- values, positions, strand bits, status code,
first-window-tie and non-ACGT flags --, the digest against the same batch with the switch unset (83 workgroups, one unit each: the other
ticketing), and a second run into the same result: the same bytes (stale tickets, list counts or look-back granules would show).

The full segment (unit_trips.EDGES): batches of nothing but exact-tie reads at one workgroup -- 1 024 reads fill the segment to its last
entry and the packed kernel's plan stays, 1 025 raise the flag and the call ends on the 64-bit kernel -- and 3 x 1 024 + 1 at three.  Both
sides together say that every tie read was listed and that the cursor counted across all 16 / 17 units.
"""
import ctypes as C
import re
import time

import numpy as np
import pytest

from bio_amd import _lib as L
from tests import plan_atlas as A
from tests import unit_trips as T
from tests.test_gpu_grid_caps import switches
from tests.test_gpu_plan_atlas import KINDS, assert_plan, expected

pytestmark = pytest.mark.gpu
U64 = np.uint64
POSITIONAL = ("minimizer", "syncmer", "prot_minimizer")


def unit_grid_stats(engine):
    out = (C.c_uint64 * 2)()
    assert engine.lib.bsk_ctx_unit_grid_stats(engine.ctx, out) == L.OK
    return int(out[0]), int(out[1])


def reference(oracle, case, seqs):
    """what the reference yields for every read, as the arrays of one fetch: offsets, status codes, flag bits (-1: the kind has none), values,
    positions, strand bits"""
    counts, codes, flags, hs, ps, ss = [], [], [], [], [], []
    for q in seqs:
        code, fl, h, pos, strand = expected(oracle, case, q)
        counts.append(len(h))
        codes.append(code)
        flags.append(-1 if fl is None else int(fl))
        hs.append(np.asarray(h, U64))
        if case.kind in POSITIONAL:
            ps.append(np.asarray(pos if pos is not None else np.zeros(0, np.uint32), np.uint32))
            ss.append(np.asarray(strand, np.uint32) if strand is not None else np.zeros(len(h), np.uint32))
    offs = np.zeros(len(seqs) + 1, U64)
    np.cumsum(counts, out=offs[1:])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return dict(offs=offs, codes=np.array(codes, np.uint8), flags=np.array(flags, np.int64), h=cat(hs, U64), pos=cat(ps, np.uint32), strand=cat(ss, np.uint32),
                has_strand=case.kind in ("minimizer", "syncmer"))


def first_bad_read(offs, mask):
    """the read that holds the first tuple where mask is set"""
    return int(np.searchsorted(offs, int(np.flatnonzero(mask)[0]), side="right") - 1)


def compare_fetch(case, ref, got, what):
    """one fetch of the whole result against the reference, read by read"""
    offs, status, h, p = got
    n = len(ref["codes"])
    assert len(offs) == n + 1 and len(status) == n, (what, len(offs), len(status), n)
    bad = np.flatnonzero((status & L.ST_CODE_MASK) != ref["codes"])
    assert not len(bad), (what, "status code of read %d: %#x, expected code %d" % (bad[0], status[bad[0]], ref["codes"][bad[0]]))
    bad = np.flatnonzero(np.diff(offs.astype(np.int64)) != np.diff(ref["offs"].astype(np.int64)))
    assert not len(bad), (what, "read %d: %d tuples, expected %d" % (bad[0], offs[bad[0] + 1] - offs[bad[0]], ref["offs"][bad[0] + 1] - ref["offs"][bad[0]]))
    assert len(h) == len(ref["h"]) > 0, (what, len(h), len(ref["h"]))
    ne = h != ref["h"]
    assert not ne.any(), (what, "values of read %d" % first_bad_read(offs, ne))
    if case.kind in POSITIONAL:
        ne = (p & L.POS_MASK) != ref["pos"]
        assert not ne.any(), (what, "positions of read %d" % first_bad_read(offs, ne))
        if ref["has_strand"]:
            ne = (p >> 31) != ref["strand"]
            assert not ne.any(), (what, "strand bits of read %d" % first_bad_read(offs, ne))
        has = ref["flags"] >= 0
        if case.kind == "prot_minimizer":
            bad = np.flatnonzero(has & (((status & L.ST_FIRST_WINDOW_TIE) != 0) != (ref["flags"] > 0)))
        else:
            bad = np.flatnonzero(has & ((status & 0xF0) != (ref["flags"] & 0xF0)))
        assert not len(bad), (what, "flags of read %d: status %#x, expected flags %#x" % (bad[0], status[bad[0]], ref["flags"][bad[0]]))


def same_bytes(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


class Prepared:
    """a case's reads, their reference and the run with the switch unset -- made once, shared by the caps (one case at a time is kept)"""
    slot = None

    @classmethod
    def get(cls, engine, oracle, key, case, seqs_of, env):
        if cls.slot is None or cls.slot.key != key:
            cls.slot = cls(engine, oracle, key, case, seqs_of(), env)
        return cls.slot

    def __init__(self, engine, oracle, key, case, seqs, env):
        self.key, self.seqs = key, seqs
        self.ref = reference(oracle, case, seqs)
        with switches(engine, dict(env, BSK_UNIT_GRID=None)):
            s0 = unit_grid_stats(engine)
            b = engine.batch(seqs, L.ALPHA_PROTEIN if case.alphabet == "protein" else L.ALPHA_DNA)
            res = engine.run(b, engine.params(KINDS[case.kind], **case.p))
            s1 = unit_grid_stats(engine)
            self.plan, self.digest = res.plan(), res.digest()
            compare_fetch(case, self.ref, res.fetch(0, len(seqs)), (key, "switch unset"))
            res.close()
            b.close()
        assert s1[0] > s0[0] and s1[1] == s0[1], (key, "switch unset: grids sized %d, cut %d" % (s1[0] - s0[0], s1[1] - s0[1]))  # the default build cuts nothing


def run_capped(engine, oracle, capfd, key, case, seqs_of, env, cap, check_plan, timing=None, uncut_max=0, cut_min=1, same_plan=True):
    """the case at BSK_UNIT_GRID=cap: plan, grid, counters, every read, the unset run's digest, and a second run into the same result"""
    t0 = time.perf_counter()
    prep = Prepared.get(engine, oracle, key, case, seqs_of, env)
    n = len(prep.seqs)
    more = dict(env, BSK_UNIT_GRID=str(cap))
    if timing:
        more["BSK_TIMING"] = "1"
    with switches(engine, more):
        s0 = unit_grid_stats(engine)
        b = engine.batch(prep.seqs, L.ALPHA_PROTEIN if case.alphabet == "protein" else L.ALPHA_DNA)
        prm = engine.params(KINDS[case.kind], **case.p)
        capfd.readouterr()
        res = engine.run(b, prm)
        err = capfd.readouterr().err
        s1 = unit_grid_stats(engine)
        plan = res.plan()
        check_plan(plan)
        if same_plan:
            assert plan["kernel"] == prep.plan["kernel"], (key, cap, plan, prep.plan)  # no plan string moves with the switch
        assert plan["grid"] == min(cap, prep.plan["grid"]) and prep.plan["grid"] > cap, (key, cap, plan, prep.plan)
        sized, cut = s1[0] - s0[0], s1[1] - s0[1]
        assert cut >= cut_min and 0 <= sized - cut <= uncut_max, (key, cap, "grids sized %d, cut %d (at least %d), may stay whole %d" % (sized, cut, cut_min, uncut_max))
        if timing:
            said = [tuple(int(x) for x in m) for m in re.findall(r"k_minimizer_pk: \S+ form, tk (\d+), tk_t0 (\d+), tk_small (\d+)", err)]
            assert said and all(s == timing for s in said), (key, cap, said, timing)
        got = res.fetch(0, n)
        compare_fetch(case, prep.ref, got, (key, "cap %d" % cap))
        d = res.digest()
        assert d == prep.digest, (key, cap, d, prep.digest)
        again = engine.run(b, prm, reuse=res)
        assert again.plan() == plan, (key, cap, again.plan(), plan)
        assert same_bytes(again.fetch(0, n), got), (key, cap, "a second run into the same result differs")
        assert again.digest() == d
        again.close()
        b.close()
    print("%s, cap %d: %s, grid %d of %d, %d grids sized, %d cut, %.2f s" % (key, cap, plan["kernel"], plan["grid"], prep.plan["grid"], sized, cut, time.perf_counter() - t0))


@pytest.mark.parametrize("rid,cap", [(r.id, cap) for r in T.ROWS for cap in T.CAPS])
def test_row(engine, oracle, capfd, rid, cap):
    row = T.BY_ID[rid]
    timing = None
    if T.family(row.name) == "k_minimizer_pk":
        t0, small, _ = T.pk_tail(T.launch_rules(), T.UNITS, cap)
        timing = (0, t0, small)
    run_capped(engine, oracle, capfd, rid, row, row.reads, row.env, cap, lambda plan: assert_plan(row, plan), timing=timing)


@pytest.mark.parametrize("cid,cap", [(c.id, cap) for c in T.CASES for cap in T.CAPS])
def test_case(engine, oracle, capfd, cid, cap):
    """tiles (the tile unit kernel over >= 83 units of tiles, k_tile_count, k_two_strand; k_tile_stitch keeps its own grid), length-binned
    units (k_bin_desc) and a class plan (k_class_cut)"""
    case = T.CASE_BY_ID[cid]

    def check_plan(plan):
        assert all(s in plan["kernel"] for s in case.plan_has), (cid, plan, case.plan_has)

    timing = None
    if case is T.BINNED_CASE:
        t0, small, _ = T.pk_tail(T.launch_rules(), T.UNITS, cap)
        timing = (0, t0, small)
    run_capped(engine, oracle, capfd, cid, case, case.reads, case.env, cap, check_plan, timing=timing, uncut_max=case.uncut_max(cap), cut_min=case.cut_min(cap))


@pytest.mark.parametrize("eid", [e.id for e in T.EDGES])
@pytest.mark.parametrize("n,cap,full", [(1024, 1, False), (1025, 1, True), (3073, 3, True)], ids=["1024 reads at 1", "1025 reads at 1", "3073 reads at 3"])
def test_full_segment(engine, oracle, eid, n, cap, full):
    e = T.EDGE_BY_ID[eid]
    row = e.row
    assert full == (n > cap * T.segment(n, cap)) and n in T.edge_sizes(cap)
    seqs = e.reads(n)
    ref = reference(oracle, row, seqs)
    with switches(engine, dict(row.env, BSK_NO_BIN="1", BSK_UNIT_GRID=str(cap))):
        b = engine.batch(seqs)
        prm = engine.params(KINDS[row.kind], **row.p)
        res = engine.run(b, prm)
        plan = res.plan()
        if full:  # a segment took one read too many: the call ends on the 64-bit kernel
            assert plan["kernel"].startswith(e.falls_to) and not any(s in plan["kernel"] for s in A.SUFFIXES), (eid, n, cap, plan)
        else:  # exactly full: the packed kernel's
            assert_plan(row, plan)
        assert plan["grid"] == cap, (eid, n, cap, plan)
        got = res.fetch(0, n)
        compare_fetch(row, ref, got, (eid, n, cap))
        assert int((got[1] & L.ST_CODE_MASK == L.ST_OK).sum()) == n  # every read long enough: every read had windows to tie in
        again = engine.run(b, prm, reuse=res)
        assert again.plan() == plan and same_bytes(again.fetch(0, n), got), (eid, n, cap)
        again.close()
        b.close()
