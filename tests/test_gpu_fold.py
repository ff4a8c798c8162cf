"""GPU: bsk_hits_fold against the NumPy model of tests/window_cases.py (fold_model: host hits in, exact integers out)."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import window_cases as WC

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32


def random_hits(rng, nq, n_targets, most=12):
    offs, tg = [0], []
    for _ in range(nq):
        t = np.sort(rng.choice(n_targets, size=int(rng.integers(0, most + 1)), replace=False))
        tg.append(t)
        offs.append(offs[-1] + len(t))
    tg = np.concatenate(tg).astype(U32) if tg else np.zeros(0, U32)
    return np.array(offs, U64), tg, rng.integers(1, 100000, len(tg)).astype(U32)


def check(engine, o, t, s, go, reuse=None, total=None, **kw):
    h = engine.hits_from_arrays(o, t, s, total)
    f = h.fold(go, reuse=reuse, **{("min_fraction" if k == "frac" else k): v for k, v in kw.items()})
    want = WC.fold_model(o, t, s, go, **kw)
    assert WC.same(f.fetch(), want[:3]) and np.array_equal(f.fetch_members(), want[3]) and np.array_equal(f.members, want[3]), (kw, go)
    assert f.has_members() and not f.has_totals() and not f.has_weights() and f.total is None and f.dot is None
    assert f.info() == dict(n_queries=len(o) - 1, n_hits=len(want[1]))
    p = f.plan()
    m = re.fullmatch(r"bsk_hits_fold: k_fold_map \+ k_fold_check \+ k_fold_runs \+ k_fold_place, groups=(\d+) runs=(\d+) kept=(\d+)", p["plan"])
    assert m and int(m.group(1)) == len(go) - 1 and int(m.group(3)) == len(want[1]) and p["n_large_queries"] == 0, p
    if len(o) > 1:
        assert WC.same(f.top(1).fetch(), WC.top1_model(*want[:3]))  # the best GROUP of every row, not the best target
    h.close()
    return f


GROUPS = np.array([0, 0, 3, 3, 10, 11, 20, 20, 20], U64)  # empty groups at the start, in the middle and at the end
RULES = [dict(), dict(min_members=0), dict(min_members=2), dict(frac=(1, 1)), dict(frac=(8, 10)), dict(frac=(1, 3)), dict(min_members=2, frac=(1, 3))]


@pytest.mark.parametrize("nq", [0, 1, 300])
def test_random_rows_every_rule(engine, nq):
    o, t, s = random_hits(np.random.default_rng(nq + 1), nq, 20)
    f = None
    for kw in RULES:
        f = check(engine, o, t, s, GROUPS, reuse=f, **kw)
    f.close()


def test_a_run_longer_than_a_workgroup_and_the_identity(engine):
    n = 5000
    o, t, s = np.array([0, n], U64), np.arange(n, dtype=U32), (np.arange(n, dtype=U32) % U32(977)) + U32(1)
    f = check(engine, o, t, s, np.array([0, n], U64))  # one row of 5 000 hits into ONE group
    assert list(f.members) == [n] and int(f.shared[0]) == int(s.astype(np.int64).sum())
    g = check(engine, o, t, s, np.arange(n + 1, dtype=U64), reuse=f)  # ... into 5 000 singleton groups: the identity
    assert (g.members == 1).all() and np.array_equal(g.shared, s) and np.array_equal(g.target, t)
    g.close()


def test_boundaries_saturation_and_exact_fractions(engine):
    # a group boundary exactly at a row boundary: row 0 ends with the last target of group 0, row 1 starts with the first of group 1
    check(engine, np.array([0, 2, 4], U64), np.array([3, 4, 5, 6], U32), np.array([1, 2, 3, 4], U32), np.array([0, 5, 10], U64)).close()
    # the same group on both sides of a row boundary: two runs
    f = check(engine, np.array([0, 2, 4], U64), np.array([1, 2, 3, 4], U32), np.array([1, 2, 3, 4], U32), np.array([0, 5], U64))
    assert list(f.offsets) == [0, 1, 2] and list(f.shared) == [3, 7]
    f.close()
    f = check(engine, np.array([0, 2], U64), np.array([0, 1], U32), np.array([0xFFFFFFFF, 1], U32), np.array([0, 2], U64))
    assert list(f.shared) == [0xFFFFFFFF] and list(f.members) == [2]  # saturation
    f.close()
    # members * den == num * size exactly: 8 of 10 against (8, 10), 1 of 3 against (1, 3); and one member short of (9, 10) and (2, 3)
    o, t, s, go = np.array([0, 9], U64), np.array([0, 1, 2, 3, 4, 5, 6, 7, 10], U32), np.ones(9, U32), np.array([0, 10, 13], U64)
    for frac, groups in (((8, 10), [0]), ((1, 3), [0, 1]), ((9, 10), []), ((2, 3), [0]), ((1, 1), [])):
        f = check(engine, o, t, s, go, frac=frac)
        assert list(f.target) == groups, frac
        f.close()


def test_totals_and_weights_do_not_survive_and_reuse_of_an_object_that_held_totals(engine):
    o, t, s = random_hits(np.random.default_rng(3), 40, 20)
    with_totals = engine.hits_from_arrays(o, t, s, s + U32(5))
    assert with_totals.has_totals()
    f = check(engine, o, t, s, GROUPS, total=s + U32(5))  # input with totals -> output without
    o2, t2, s2 = random_hits(np.random.default_rng(4), 50, 20)
    check(engine, o2, t2, s2, GROUPS, reuse=with_totals, min_members=2)  # an object that held totals, re-used for folded hits
    assert not with_totals.has_totals() and with_totals.has_members()
    engine.hits_from_arrays(o, t, s, reuse=f)  # and folded hits re-used by a writer without members: they go, like the totals
    assert not f.has_members() and f.members is None
    # weighted neighbours in, neither totals nor weights out
    vals = np.arange(1, 41, dtype=U64)
    a = engine.sets_from_arrays_counted(np.array([0, 10, 25, 40], U64), vals, np.full(40, 2, U32))
    b = engine.sets_from_arrays_counted(np.array([0, 20, 40], U64), vals, np.full(40, 3, U32))
    nb = a.neighbors_counted(b)
    assert nb.has_weights() and nb.has_totals()
    fo = nb.fold(np.array([0, 2], U64))
    want = WC.fold_model(*nb.fetch(), np.array([0, 2], U64))
    assert WC.same(fo.fetch(), want[:3]) and np.array_equal(fo.members, want[3]) and not fo.has_weights() and not fo.has_totals()
    for x in (with_totals, f, a, b, nb, fo):
        x.close()


def test_folded_twice_equals_folded_once(engine):
    """chunks -> genomes -> genera equals chunks -> genera with the composed offsets (shared below saturation)"""
    rng = np.random.default_rng(11)
    o, t, s = random_hits(rng, 120, 60, most=30)
    genomes = np.array([0, 4, 4, 10, 25, 31, 40, 52, 60], U64)  # of chunks
    genera = np.array([0, 2, 3, 3, 8], U64)                     # of genomes
    h = engine.hits_from_arrays(o, t, s)
    twice = h.fold(genomes).fold(genera)
    once = h.fold(genomes[genera.astype(np.int64)])
    assert WC.same(twice.fetch(), once.fetch()) and WC.same(once.fetch(), WC.fold_model(o, t, s, genomes[genera.astype(np.int64)])[:3])
    assert np.array_equal(twice.members, WC.fold_model(*h.fold(genomes).fetch(), genera)[3])  # members of the second fold: genomes hit


def test_errors_keep_the_slot(engine):
    o, t, s = random_hits(np.random.default_rng(5), 30, 20)
    h = engine.hits_from_arrays(o, t, s)
    f = h.fold(GROUPS)
    before, slot, lib = f.fetch(), C.c_void_p(f.h.value), engine.lib
    go = GROUPS

    def call(ctx, hh, g, ng, fp, out):
        return lib.bsk_hits_fold(ctx, hh, g.ctypes.data if g is not None else None, ng, C.byref(fp) if fp is not None else None, out)

    other = S.Engine(0)
    foreign = other.hits_from_arrays(o, t, s)
    FP = L.FoldParams
    bad = [(engine.ctx, None, go, 8, None), (engine.ctx, h.h, None, 8, None), (None, h.h, go, 8, None), (engine.ctx, h.h, go, 8, FP(1, 1, 0, 0)),
           (engine.ctx, h.h, go, 8, FP(1, 0, 3, 2)), (other.ctx, h.h, go, 8, None), (engine.ctx, foreign.h, go, 8, None),
           (engine.ctx, h.h, np.array([0, 5, 3, 20], U64), 3, None), (engine.ctx, h.h, np.array([1, 5, 20], U64), 2, None),
           (engine.ctx, h.h, np.array([0, 5, int(t.max())], U64), 2, None),  # a target beyond the last offset: the largest one equals it
           (engine.ctx, h.h, np.array([0, 2**32 + 1], U64), 1, None)]
    for ctx, hh, g, ng, fp in bad:
        assert call(ctx, hh, g, ng, fp, C.byref(slot)) == L.ERR_ARG and slot.value == f.h.value, (g, ng)
    # a top() result as input: its rows are in order of shared count
    o3, t3, s3 = np.array([0, 3], U64), np.array([1, 5, 9], U32), np.array([1, 9, 5], U32)
    h3 = engine.hits_from_arrays(o3, t3, s3)
    t3top = h3.top(3)
    assert list(t3top.target) == [5, 9, 1]
    assert call(engine.ctx, t3top.h, go, 8, None, C.byref(slot)) == L.ERR_ARG and slot.value == f.h.value
    assert b"strictly ascending" in lib.bsk_last_error(engine.ctx)
    assert call(engine.ctx, f.h, go, 8, None, C.byref(slot)) == L.ERR_ARG and slot.value == f.h.value  # *out == h
    assert call(engine.ctx, h.h, go, 8, None, None) == L.ERR_ARG
    fslot = C.c_void_p(foreign.h.value)
    assert call(engine.ctx, h.h, go, 8, None, C.byref(fslot)) == L.ERR_ARG and fslot.value == foreign.h.value
    assert WC.same(f.fetch(), before)  # kept means intact
    buf = np.zeros(4, U32)
    assert lib.bsk_hits_fetch_members(engine.ctx, h.h, 0, 1, buf.ctypes.data, 4) == L.ERR_ARG  # hits without members
    assert lib.bsk_hits_fetch_members(engine.ctx, f.h, 0, 31, buf.ctypes.data, 4) == L.ERR_ARG  # a range outside the hits
    assert lib.bsk_hits_fetch_members(other.ctx, f.h, 0, 1, buf.ctypes.data, 4) == L.ERR_ARG
    for x in (foreign, other):
        x.close()


@contextlib.contextmanager
def grid_cap(engine, cap):
    try:
        os.environ["BSK_GRID_CAP"] = str(cap)
        engine.reload_options()
        yield
    finally:
        os.environ.pop("BSK_GRID_CAP", None)
        engine.reload_options()


def test_capped_grids_and_repeatability(engine):
    o, t, s = random_hits(np.random.default_rng(6), 600, 400, most=40)
    go = np.arange(0, 401, 10, dtype=U64)
    plain = check(engine, o, t, s, go, min_members=2)
    want = plain.fetch() + (plain.members,)
    out = (C.c_uint64 * 2)()
    for cap in (1, 3):
        with grid_cap(engine, cap):
            engine.lib.bsk_ctx_grid_stats(engine.ctx, out)
            c0 = int(out[1])
            f = check(engine, o, t, s, go, min_members=2)
            engine.lib.bsk_ctx_grid_stats(engine.ctx, out)
            # cap 1 cuts all six grids of the fold; cap 3 those over the hits and the runs (400 targets, 600 rows: three workgroups cover them)
            assert int(out[1]) - c0 >= (6 if cap == 1 else 3), (cap, int(out[1]) - c0)
            assert WC.same(f.fetch() + (f.members,), want)  # bit-identical from call to call, capped or not
            f.close()
