"""k_minimizer_pk's block loop at the edges of its word arithmetic and of its two loops.

PkMin::run (kernels_pk.hpp) carries twice the number of the base that enters and of the one that leaves at a block's slot 0 (bits 5..
index the packed word, bits 0..4 are the shift), runs block PAIRS without a per-lane window test while another block follows the pair
and every lane with a read fills both (i0 + 2 W < nk_min), and the rest -- at least one block -- in the ragged variants.  So what can
go wrong depends on (k, w) (where the entering and the leaving base fall in their words, k + w on both sides of 32), on nk mod W (the
last block holds 1, W - 1 or W windows; the steady loop ends one, two or three blocks before the read does), on how far the words
reach (150 bases, and 239 / 240 / 241 at the sixteenth packed word, where k_minimizer_pk<W, true> takes over and loads the rest), and
on whether a unit's lanes agree on any of it (fixed length, ragged from one window up, ragged above L / 2, lanes without a read).  Every read of every batch is compared
with the reference's state machine; every batch asserts the kernel that ran.
"""
import random

import numpy as np
import pytest

from bio_amd import _lib as L
from tests import key_ties as KT

pytestmark = pytest.mark.gpu

KW = [(21, 11), (22, 11), (20, 11), (19, 13), (16, 11), (15, 11), (11, 5), (31, 2), (27, 5), (28, 5)]
N_FIXED = 2 * 64 + 37    # three units, lanes 37..63 of the last one without a read
N_RAGGED = 2 * 64


def lengths(k, w):
    """k + w - 1 (one window); nk = 0, 1, W - 1 (mod W) a few blocks long; 150; the sixteenth packed word: 239, 240 and 241 bases"""
    nk0 = w * max(4, -(-60 // w))
    out = [k + w - 1] + [nk0 + r + k - 1 for r in (0, 1, w - 1)] + [150, 239, 240, 241]
    assert all((n - k + 1) % w == r for n, r in zip(out[1:4], (0, 1, w - 1)))
    return out


def plan_of(w, maxlen):
    return "k_minimizer_pk<%d,%s>" % (w, "true" if maxlen > 240 else "false")


def check_batch(engine, oracle, seqs, k, w, plan):
    b = engine.batch(seqs)
    res = engine.run(b, engine.params(L.MINIMIZER, k, w=w))
    name = res.plan()["kernel"]
    assert name.startswith(plan), (plan, name)
    for i, q in enumerate(seqs):
        st, h, p = res.read(i)
        where = (k, w, i, len(q))
        if len(q) < k + w - 1:
            assert (st & L.ST_CODE_MASK) == L.ST_SHORT and len(h) == 0, where
            continue
        mh, mp, ms, fl = oracle.minimizer(q, k, w)  # closed=False: the state machine
        assert (st & L.ST_CODE_MASK) == L.ST_OK, where
        assert bool(st & L.ST_FIRST_WINDOW_TIE) == bool(fl & oracle.FLAG_FIRST_WINDOW_TIE), where
        assert np.array_equal(h, mh), where
        assert np.array_equal(p & L.POS_MASK, mp) and np.array_equal(p >> 31, ms), where
    res.close()
    b.close()


@pytest.fixture
def pk_only(monkeypatch):
    """the packed machine for every batch (the planner would hand short and dense batches to its siblings)"""
    for v in ("BSK_RING", "BSK_TILE_MIN", "BSK_TILE_POS", "BSK_TILE_DENSE", "BSK_NO_PK"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("BSK_NO_RING", "1")
    monkeypatch.setenv("BSK_NO_DENSE", "1")


@pytest.mark.parametrize("k,w", KW)
def test_fixed_length(engine, oracle, pk_only, k, w):
    """every lane of a unit ends in the same block; the last unit's lanes 37..63 have no read; a homopolymer in every batch"""
    rng = random.Random(KT.hash_seed("fixed", k, w))
    for n in lengths(k, w):
        seqs = [KT.rand_seq(rng, n) for _ in range(N_FIXED)]
        seqs[70] = "A" * n
        check_batch(engine, oracle, seqs, k, w, plan_of(w, n))


@pytest.mark.parametrize("k,w", KW)
def test_ragged_within_a_unit(engine, oracle, pk_only, k, w):
    """Two units (small batches are not length-binned: a unit is 64 consecutive reads).  The first draws its lengths from one window up
    to L and holds a one-window read: nk_min = W, no steady pair runs, every block after the first is ragged.  The second draws from
    about L / 2 up to L: the steady pairs end where its shortest read does and several ragged blocks follow them."""
    rng = random.Random(KT.hash_seed("ragged", k, w))
    for n in lengths(k, w):
        half = max(k + w - 1, (n + k) // 2)
        lens = [rng.randint(k + w - 1, n) for _ in range(64)] + [rng.randint(half, n) for _ in range(64)]
        lens[3], lens[64 + 5] = n, n   # the longest read decides the kernel
        lens[17] = k + w - 1           # one window
        lens[64 + 40] = half           # the second unit's shortest read
        seqs = [KT.rand_seq(rng, m) for m in lens]
        seqs[29] = "C" * lens[29]
        check_batch(engine, oracle, seqs, k, w, plan_of(w, n))


def key_equal_pair_at_slot0(oracle, t):
    """the read's crafted pair: equal 27-bit keys, different hashes, less than W apart, the left one at slot 0 of its block"""
    h = oracle.nthash(t.seq, t.k)[0]
    a, b = int(h[t.a]), int(h[t.a + t.d])
    return t.a % t.w == 0 and t.d < t.w and a != b and a >> KT.KEY_SHIFT == b >> KT.KEY_SHIFT


def test_tie_at_block_slot_0(engine, oracle, pk_only):
    """Reads the packed machine has to hand to the exact one: a homopolymer, and crafted key ties (tests/golden/key_ties.json) whose left
    element sits at slot 0 of a block -- the suffix pass no longer compares slot 0 with slot 1 (S[0] is never read; the pair meets as
    prefix minimum against new element instead).  Every distance d < W in both orientations, in the first, an interior and the last
    block, among random reads, must come back exact.  That a read went through the list is not observable from outside (the library
    reports no count of listed reads); what is asserted is that every planted pair is a key tie of different hashes at slot 0, and
    the result: a machine that missed the tie would keep the wrong element in one of the two orientations."""
    k, w = KT.MIN_K, 11
    reads = [t for t in KT.build_minimizer_reads(oracle, k, w, lambda e: 150, KT.hash_seed("slot0", k, w))[0] if t.a % w == 0]
    assert {(t.d, t.side, t.place) for t in reads} == {(d, s, pl) for d in range(1, w) for s in ("left", "right")
                                                      for pl in ("first", "interior", "last")}
    assert all(key_equal_pair_at_slot0(oracle, t) for t in reads)
    rng = random.Random(11)
    seqs = []
    for t in reads:
        seqs += [t.seq, KT.rand_seq(rng, 150), KT.rand_seq(rng, 150)]
    seqs[1] = "A" * 150
    assert len(seqs) <= 3 * 64
    seqs += [KT.rand_seq(rng, 150) for _ in range(3 * 64 - len(seqs))]
    check_batch(engine, oracle, seqs, k, w, plan_of(w, 150))
