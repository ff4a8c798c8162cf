"""Accidental 27-bit key ties on every packed window machine, bit-exact against the oracle's state machine.

The packed minimizer and syncmer kernels compare one 32-bit word per element (hash >> 37 | slot) and are exact only because every
min operation keeps tmin = min(a ^ b) and a read that saw tmin < 32 is run again by the exact 64-bit machine (kernels_pk.hpp header;
PkMin, RgMin, SynPk::tie).  Real 64-bit ties (homopolymers, repeats) set that check off in every min operation at once; the reads here
hold ONE crafted pair of different hashes with equal keys (tests/golden/key_ties.json), with the smaller hash on either side.
Minimizers: every d < W at every block offset, in the first, an interior and the last partial block and across tile boundaries.
Syncmers: every d < W in both orientations, and some pairs W..2W-1 apart, at the offsets where random flanks give the read teeth.
Every read has teeth (tests/test_key_tie_fixtures.py): a machine that missed the check at that place would select differently.  Tie
reads sit between plain random reads, so only some lanes of a unit go to the exact machine.
"""
import functools

import numpy as np
import pytest

from bio_amd import _lib as L
from tests import key_ties as KT

pytestmark = pytest.mark.gpu

_SWITCHES = ("BSK_NO_RING", "BSK_NO_DENSE", "BSK_RING", "BSK_TILE_MIN", "BSK_TILE_POS", "BSK_TILE_DENSE", "BSK_NO_SYN_PF")


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
    b = engine.batch(seqs)
    p = engine.params(L.MINIMIZER, k, w=w) if kind == "minimizer" else engine.params(L.SYNCMER, k, s=s)
    res = engine.run(b, p)
    name = res.plan()["kernel"]
    assert plan in name, (plan, name)
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
