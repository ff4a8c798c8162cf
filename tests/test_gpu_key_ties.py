"""Accidental 27-bit key ties on every packed window machine, bit-exact against the oracle's state machine.

The packed minimizer and syncmer kernels compare one 32-bit word per element (hash >> 37 | slot) and are exact only because every
min operation keeps tmin = min(a ^ b) and a read that saw tmin < 32 is run again by the exact 64-bit machine (kernels_pk.hpp header;
PkMin, RgMin, SynPk::tie).  Real 64-bit ties (homopolymers, repeats) set that check off in every min operation at once; the reads here
hold ONE crafted pair of different hashes with equal keys (tests/golden/key_ties.json), with the smaller hash on either side.
Minimizers: every d < W at every block offset, in the first, an interior and the last partial block and across tile boundaries.
Syncmers: every d < W in both orientations, and some pairs W..2W-1 apart, at the offsets where random flanks give the read teeth.
Every read has teeth (tests/test_key_tie_fixtures.py): a machine that missed the check at that place would select differently.  Tie
reads sit between plain random reads, so only some lanes of a unit go to the exact machine.
Syncmers, furthermore (KT.SYN_CELLS2, one test case per cell, run and W, each with its exact plan string): a pair at a tile seam with
teeth in a named tile, over forced tiles of 16 and 64 positions and over default tiles; the long staged plan k_syncmer_pkl<W> for W <= 20;
and a pair in the last blocks of a read whose neighbours are 3W .. 6W bases longer.  A closing test holds the (kernel, W) pairs these
cases reached with a tie read against KT.SYN_REACH.
"""
import functools

import numpy as np
import pytest

from bio_amd import _lib as L
from tests import key_ties as KT

pytestmark = pytest.mark.gpu

_SWITCHES = ("BSK_NO_RING", "BSK_NO_DENSE", "BSK_RING", "BSK_TILE_MIN", "BSK_TILE_POS", "BSK_TILE_DENSE", "BSK_NO_SYN_PF")
_REACHED = {}  # (cell, mode, w) of KT.SYN_CASES2 -> ((kernel, w), tie reads run) of a case that passed


@functools.lru_cache(maxsize=None)
def _min_reads(oracle, name, w, k):
    return KT.min_set_reads(oracle, name, w, k=k)[0]


@functools.lru_cache(maxsize=None)
def _syn_reads(oracle, w):
    return KT.syn_reads(oracle, w)[0]


def _set_env(monkeypatch, env):
    for v in _SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for v, x in env.items():
        monkeypatch.setenv(v, x)


def _run_and_check(engine, oracle, kind, k, w, s, reads, plan, seed, not_in_plan=None):
    seqs, at = KT.with_plain_reads(reads, seed)
    return _check_seqs(engine, oracle, kind, k, w, s, seqs, at, plan, not_in_plan=not_in_plan)


def _check_seqs(engine, oracle, kind, k, w, s, seqs, at, plan, not_in_plan=None, exact_plan=False):
    """every read of the batch bit-exact against the oracle's state machine; the plan string holds `plan` (exact_plan: is `plan`)"""
    b = engine.batch(seqs)
    p = engine.params(L.MINIMIZER, k, w=w) if kind == "minimizer" else engine.params(L.SYNCMER, k, s=s)
    res = engine.run(b, p)
    name = res.plan()["kernel"]
    assert (plan == name) if exact_plan else (plan in name), (plan, name)
    assert not_in_plan is None or not_in_plan not in name, name
    ties = set(at)
    for i, q in enumerate(seqs):
        st, h, pos = res.read(i)
        if kind == "minimizer":
            mh, mp, ms, fl = oracle.minimizer(q, k, w)       # closed=False: the state machine
        else:
            mh, mp, ms, fl = oracle.syncmer(q, k, s)
        where = (kind, k, w, s, i, i in ties, len(q))
        assert (st & L.ST_CODE_MASK) == L.ST_OK, where
        assert bool(st & L.ST_FIRST_WINDOW_TIE) == bool(fl & oracle.FLAG_FIRST_WINDOW_TIE), where
        assert np.array_equal(h, mh), where
        assert np.array_equal(pos & L.POS_MASK, mp) and np.array_equal(pos >> 31, ms), where
    res.close()
    b.close()
    return len(at)


@pytest.mark.parametrize("cell", [c[0] for c in KT.MIN_CELLS])
def test_minimizer_key_ties(engine, oracle, monkeypatch, cell):
    _, env, rset, ws, plan = next(c for c in KT.MIN_CELLS if c[0] == cell)
    _set_env(monkeypatch, env)
    for w in ws:
        reads = _min_reads(oracle, rset, w, KT.MIN_K)
        assert len(reads) == 2 * w * (w - 1) * len(KT.MIN_SETS[rset][2]), (cell, w, len(reads))   # every layout (test_key_tie_fixtures)
        n = _run_and_check(engine, oracle, "minimizer", KT.MIN_K, w, 0, reads, plan % w if "%d" in plan else plan,
                           KT.hash_seed(cell, w), not_in_plan="k_minimizer_pft" if cell.startswith("tiles") else None)
        assert n > 0, (cell, w)


@pytest.mark.parametrize("k,ws", KT.MIN_OTHER_K)
def test_minimizer_key_ties_other_k(engine, oracle, monkeypatch, k, ws):
    _set_env(monkeypatch, {"BSK_NO_RING": "1", "BSK_NO_DENSE": "1"})
    for w in ws:
        reads = _min_reads(oracle, "short", w, k)
        assert not KT.missing_classes(reads, w), (k, w)
        assert _run_and_check(engine, oracle, "minimizer", k, w, 0, reads, "k_minimizer_pk<%d,false>" % w, KT.hash_seed("k", k, w)) > 0


@pytest.mark.parametrize("cell", [c[0] for c in KT.SYN_CELLS])
def test_syncmer_key_ties(engine, oracle, monkeypatch, cell):
    _, env, ws, plan = next(c for c in KT.SYN_CELLS if c[0] == cell)
    _set_env(monkeypatch, env)
    for w in ws:
        by_s = _syn_reads(oracle, w)
        assert not KT.missing_classes([t for v in by_s.values() for t in v], w), (cell, w)
        total = 0
        for s, reads in sorted(by_s.items()):
            total += _run_and_check(engine, oracle, "syncmer", s + w, w, s, reads, plan(w), KT.hash_seed(cell, w, s))
        assert total > 0, (cell, w)


# ---- syncmer ties at tile seams, on the long staged plan and at ragged ends (KT.SYN_CELLS2) --------------------------------------------
@functools.lru_cache(maxsize=None)
def _cell_reads(oracle, cell, w):
    return KT.syn_cell_reads(oracle, cell, w)[0]


def _run_syn_cell(engine, oracle, monkeypatch, cell, mode, w):
    """one case of KT.SYN_CASES2: the cell's tie reads of W between plain reads, in batches of one s and at most KT.BATCH_TIES tie reads;
    the plan string is the kernel KT.SYN_PLANS names for (cell, mode, W) + the cell's suffix, and nothing else"""
    if (cell, mode, w) in _REACHED:
        return _REACHED[cell, mode, w]
    suffix = next(c for c in KT.SYN_CELLS2 if c[0] == cell)[2]
    kernel = KT.SYN_PLANS[cell, mode][w]
    _set_env(monkeypatch, KT.syn_cell_env(cell, mode))
    by_s = _cell_reads(oracle, cell, w)
    reads = [t for v in by_s.values() for t in v]
    if cell in ("syn_tiles16", "syn_tiles64"):
        assert not KT.missing_seam_classes(reads, w), (cell, w)
    else:
        assert not KT.missing_classes(reads, w), (cell, w)
    total = 0
    for s, v in sorted(by_s.items()):
        for i, part in enumerate(KT.chunks(v, KT.BATCH_TIES)):
            seed = KT.hash_seed(cell, mode, w, s, i)
            seqs, at = KT.with_ragged_neighbours(part, seed) if cell == "syn_ragged" else KT.with_plain_reads(part, seed)
            total += _check_seqs(engine, oracle, "syncmer", s + w, w, s, seqs, at, kernel + suffix, exact_plan=True)
    assert total == len(reads) > 0, (cell, mode, w)
    _REACHED[cell, mode, w] = ((kernel.split("<")[0], w), total)
    return _REACHED[cell, mode, w]


@pytest.mark.parametrize("cell,mode,w", KT.SYN_CASES2, ids=["%s-%s-%d" % c for c in KT.SYN_CASES2])
def test_syncmer_key_ties_at_seams_long_plan_and_ragged_ends(engine, oracle, monkeypatch, cell, mode, w):
    """syn_tiles16 / syn_tiles64: a pair at a tile seam, with teeth in the tile before the seam, in the one after it, or in both
    (KT.build_syncmer_seam_reads), over forced tiles of 16 and 64 positions -- each of the two tiles must list ITSELF for the exact machine
    and run there with its own first idx, end rule and keep range.  syn_tiles_default: sequences of 449 .. 1 500 bases over the tiles the
    planner sizes itself; the library does not report its tile size, so these reads carry read-level teeth only (the pair across a
    multiple of 16, as every tile start is).  syn_long: k_syncmer_pkl<W> for W <= 20, the long columns and their block schedule.  syn_ragged:
    the pair in the last blocks of a read whose neighbours are 3W .. 6W bases longer, in batch order: the lane runs on past its read's end
    on made-up keys.  mode 'pf': the fused-emit kernels where they are planned; 'pk': BSK_NO_SYN_PF"""
    _run_syn_cell(engine, oracle, monkeypatch, cell, mode, w)


def test_syncmer_key_tie_reach(engine, oracle, monkeypatch):
    """the (kernel, W) pairs the cases above ran a tie read on are exactly KT.SYN_REACH: every packed syncmer instantiation (a case the
    session did not run before is run here; k_syncmer_fast<4>, the 64-tile case of W = 4, is no packed kernel and counts for nothing)"""
    got = {_run_syn_cell(engine, oracle, monkeypatch, *c)[0] for c in KT.SYN_CASES2}
    assert {g for g in got if g[0] != "k_syncmer_fast"} == KT.SYN_REACH
    assert {g for g in got if g[0] == "k_syncmer_fast"} == {("k_syncmer_fast", 4)}
