"""The crafted key-tie fixtures (tests/golden/key_ties.json) hold, and every read tests/test_gpu_key_ties.py builds from them has teeth.

The packed window machines compare hash >> 37 (27 bits) plus a slot number and trust that only where no two elements of a window share
the minimal key; every min operation checks for such a pair (kernels_pk.hpp header).  These tests keep the evidence for that check
honest without a GPU: each fixture is re-derived from oracle.nthash, and each GPU read is shown to select differently under a machine
that ignores the low 37 bits (leftmost-first or rightmost-first among equal keys) -- so a missing check fails the GPU test somewhere.
"""
import random

import numpy as np
import pytest

from tests import key_ties as KT


def test_fixtures_are_accidental_key_ties(oracle):
    fx = KT.fixtures()
    assert fx["key_shift"] == KT.KEY_SHIFT
    for fam in ("minimizer", "syncmer"):
        for e in fx[fam]:
            k, d, core = e["k"], e["d"], e["core"]
            h = [int(v) for v in oracle.nthash(core, k)[0]]
            assert len(core) == k + d and e["a"] == 0 and e["b"] == d, e
            ha, hb = h[0], h[d]
            assert (str(ha), str(hb)) == (e["hash_a"], e["hash_b"]), e
            assert ha >> KT.KEY_SHIFT == hb >> KT.KEY_SHIFT and ha != hb, e        # a key tie, not a 64-bit tie
            assert e["smaller"] == ("left" if ha < hb else "right"), e
            assert all(v > max(ha, hb) for v in h[1:d]), e                         # below every element between them


def test_fixtures_cover_every_distance_in_both_orientations():
    have = {(fam, e["k"], e["d"], e["smaller"]) for fam in ("minimizer", "syncmer") for e in KT.fixtures()[fam]}
    for k in (21, 15, 31, 40):
        for d in range(1, 13):
            for side in ("left", "right"):
                assert ("minimizer", k, d, side) in have, (k, d, side)
    for d in range(1, 48):   # d < 2W for W up to 24
        for side in ("left", "right"):
            assert ("syncmer", KT.syn_s(d), d, side) in have, (d, side)


@pytest.mark.parametrize("k,w", [(21, 2), (21, 11), (15, 5), (40, 13), (5, 3)])
def test_closed_minimizer_equals_oracle(oracle, k, w):
    rng = random.Random(k * 31 + w)
    seqs = [KT.rand_seq(rng, rng.randint(k + w - 1, 400)) for _ in range(150)] + ["A" * 80, "AC" * 60]
    for q in seqs:
        h = oracle.nthash(q, k)[0]
        eh, ep, es, fl = oracle.minimizer(q, k, w, closed=True)
        assert np.array_equal(KT.minimizer_positions(h, w), ep), (k, w, q)


@pytest.mark.parametrize("k,s", [(15, 11), (35, 11), (28, 24), (48, 24), (31, 16)])
def test_closed_syncmer_equals_oracle(oracle, k, s):
    rng = random.Random(k * 37 + s)
    seqs = [KT.rand_seq(rng, rng.randint(2 * k - s - 1, 400)) for _ in range(150)] + ["A" * 120, "AC" * 70]
    for q in seqs:
        hs = oracle.nthash(q, s)[0]
        eh, ep, es, fl = oracle.syncmer(q, k, s, closed=True)
        assert np.array_equal(KT.syncmer_positions(hs, k, s, len(q)), ep), (k, s, q)


def _check_teeth(oracle, t, kind):
    """the read's true selection is the oracle's, and a key-only machine (either tie-break) selects differently"""
    q = t.seq
    if kind == "minimizer":
        h = oracle.nthash(q, t.k)[0]
        ep = oracle.minimizer(q, t.k, t.w, closed=True)[1]
        mp = oracle.minimizer(q, t.k, t.w)[1]
        assert np.array_equal(KT.minimizer_positions(h, t.w), ep) and np.array_equal(mp, ep)
        assert any(not np.array_equal(ep, KT.minimizer_positions(h, t.w, r)) for r in ("left", "right")), (t.w, t.d, t.a, t.side)
    else:
        hs = oracle.nthash(q, t.s)[0]
        ep = oracle.syncmer(q, t.k, t.s, closed=True)[1]
        mp = oracle.syncmer(q, t.k, t.s)[1]
        assert np.array_equal(KT.syncmer_positions(hs, t.k, t.s, len(q)), ep) and np.array_equal(mp, ep)
        assert any(not np.array_equal(ep, KT.syncmer_positions(hs, t.k, t.s, len(q), r)) for r in ("left", "right")), (t.w, t.d, t.a)


@pytest.mark.parametrize("name", sorted(KT.MIN_SETS))
def test_every_minimizer_tie_read_has_teeth(oracle, name):
    """k = 21: EVERY layout (d < W, start residue, orientation, placement) is built -- the guard makes the teeth -- and the last
    (ragged) block is met at every nk mod W"""
    for w in KT.MIN_SETS[name][0]:
        reads, lost = KT.min_set_reads(oracle, name, w)
        assert lost == 0 and len(reads) == 2 * w * (w - 1) * len(KT.MIN_SETS[name][2]), (name, w, lost, len(reads))
        ends = {(t.place, (len(t.seq) - KT.MIN_K + 1) % w) for t in reads}
        for place in KT.MIN_SETS[name][2]:
            if place == "last":   # the ragged last block at every nk mod W
                assert {e for p, e in ends if p == place} == set(range(w)), (name, w)
        for t in reads:
            _check_teeth(oracle, t, "minimizer")


def test_every_other_k_tie_read_has_teeth(oracle):
    for k, ws in KT.MIN_OTHER_K:
        for w in ws:
            reads, _ = KT.min_set_reads(oracle, "short", w, k=k)
            assert not KT.missing_classes(reads, w), (k, w, KT.missing_classes(reads, w))
            for t in reads:
                _check_teeth(oracle, t, "minimizer")


def test_every_syncmer_tie_read_has_teeth(oracle):
    """syncmer reads have no guards: every (d, side) with d < W keeps reads; of the pairs W..2W-1 apart (they meet only where a 2W
    window's two halves are combined) some do, at every W"""
    for w in range(4, 25):
        by_s, _ = KT.syn_reads(oracle, w)
        reads = [t for v in by_s.values() for t in v]
        assert not KT.missing_classes(reads, w), (w, KT.missing_classes(reads, w))
        assert any(t.d >= w for t in reads), w
        for t in reads:
            _check_teeth(oracle, t, "syncmer")
