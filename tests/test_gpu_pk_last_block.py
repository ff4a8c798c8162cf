"""The last block of k_minimizer_pk's window machine and the last trip of its copy-out.

PkMin::run ends in the ragged variants of PkMin::steps.  The block that holds the last window of the wave's longest lane hashes
live = min(W, nk_max - i0) steps only -- the steps behind them belong to no window of any lane: they only stage the previous block's
slots -- and PkMin::drain stages that block's first `live` slots.  pk_copyout's last trip runs ceil((T - t0) / 64) rows.  So what can
go wrong depends on the number of live steps (1 .. W), on what the last block follows (block 0, a ragged block, a steady pair), on
whether the lanes of a unit agree on where they end, on what lies behind a read (dead steps used to hash it and to feed it to the tie
checks), and on T mod 512.  Fixed-length batches run both forms of the kernel (BSK_PK_NO_UNIFORM) and are compared word for word;
every read of every batch is compared with the reference's state machine; every batch asserts the kernel that ran.
"""
import random

import numpy as np
import pytest

from bio_amd import _lib as L
from tests import key_ties as KT
from tests import test_gpu_pk_uniform as U

pytestmark = pytest.mark.gpu

K = U.K
COUNTS = (65, 8 * 64 + 1)
EXTRA = (76, 100, 101, 125, 150, 151, 240)
# L = k + w - 1 + j, j = 0 .. 2w: nk = w + j -- block 0 alone (j = 0), a last block of 1 .. w windows right behind block 0 (j = 1 .. w),
# and of 1 .. w windows behind a ragged block (j = w + 1 .. 2w); the EXTRA lengths end behind steady pairs
LIVE_CASES = [(w, K + w - 1 + j) for w in (2, 5, 11, 13) for j in range(2 * w + 1)] + [(w, ln) for w in (2, 5, 11, 13) for ln in EXTRA]


def live_of(length, w, k=K):
    """windows in the block that holds a read's last window"""
    nk = length - k + 1
    return nk - ((nk - 1) // w) * w


def test_live_case_table():
    for w in (2, 5, 11, 13):
        first = {live_of(ln, x) for x, ln in LIVE_CASES if x == w and w < ln - K + 1 <= 2 * w}
        second = {live_of(ln, x) for x, ln in LIVE_CASES if x == w and 2 * w < ln - K + 1 <= 3 * w}
        assert first == second == set(range(1, w + 1)), w
    assert {live_of(ln, 11) for ln in EXTRA} == {1, 3, 4, 6, 9, 10, 11}


@pytest.mark.parametrize("w,length", LIVE_CASES)
def test_every_live_count(engine, oracle, monkeypatch, capfd, w, length):
    p = engine.params(L.MINIMIZER, K, w=w)
    for n in COUNTS:
        data, offs = U.rand_reads(length * 7919 + w * 101 + n, n, length)
        res = U.both_forms(engine, monkeypatch, capfd, lambda: engine.batch_from_arrays(data, offs), p, "k_minimizer_pk<%d,false>" % w)
        U.check_reads(res, oracle, U.seqs_of(data, offs, range(n)), w)
        res.close()


@pytest.mark.parametrize("length", range(241, 253))
def test_long_kernel_every_residue(engine, oracle, monkeypatch, capfd, length):
    """k_minimizer_pk<11, true>: nk = 221 .. 232, every residue mod 11"""
    w, n = 11, 65
    p = engine.params(L.MINIMIZER, K, w=w)
    data, offs = U.rand_reads(length * 31 + 5, n, length)
    res = U.both_forms(engine, monkeypatch, capfd, lambda: engine.batch_from_arrays(data, offs), p, "k_minimizer_pk<%d,true>" % w, uniform=False)
    U.check_reads(res, oracle, U.seqs_of(data, offs, range(n)), w)
    res.close()


def ragged_unit(rng, w, top_lane, k=K):
    """64 reads, the longest (nk = 9 w + 3: three live steps in the last block) in lane top_lane; around it lanes that end in the
    same block with one and two windows, one and two blocks earlier, on a block's last slot, and lanes without a read"""
    nk_top = 9 * w + 3
    special = [9 * w + 1, 9 * w + 2,            # the same block: one and two windows
               9 * w, 8 * w,                    # an exact multiple of W: their last block is full
               8 * w + 1, 9 * w - 1,            # one block earlier
               7 * w + 1, 8 * w - 1,            # two blocks earlier
               w, w + 1, 0, -5]                 # block 0 alone, one window behind it, SHORT reads (one base short, and shorter)
    nks = [rng.choice(special) for _ in range(64)]
    free = [i for i in range(64) if i != top_lane]
    rng.shuffle(free)
    for i, nk in zip(free, special):
        nks[i] = nk
    nks[top_lane] = nk_top
    lens = [nk + k - 1 if nk > 0 else k + w - 2 + nk for nk in nks]
    return [KT.rand_seq(rng, n) for n in lens]


@pytest.mark.parametrize("w", (5, 11, 13))
@pytest.mark.parametrize("top_lane", (0, 31, 32, 63))
def test_ragged_unit_general_form(engine, oracle, monkeypatch, w, top_lane):
    """one ragged unit (and the same unit again as a second one, behind 64 plain reads): the longest lane alone decides the live
    steps, every other lane keeps its own window mask"""
    for v, x in U.BASE_ENV.items():
        monkeypatch.setenv(v, x)
    monkeypatch.delenv("BSK_PK_NO_UNIFORM", raising=False)
    rng = random.Random(KT.hash_seed("last-block-ragged", w, top_lane))
    unit = ragged_unit(rng, w, top_lane)
    seqs = unit + [KT.rand_seq(rng, 9 * w + 3 + K - 1) for _ in range(64)] + unit
    b = engine.batch(seqs)
    res = engine.run(b, engine.params(L.MINIMIZER, K, w=w))
    assert res.plan()["kernel"].startswith("k_minimizer_pk<%d,false>" % w), res.plan()
    U.check_reads(res, oracle, dict(enumerate(seqs)), w)
    res.close()
    b.close()


# (length, live steps at w = 11): 144 bases are nine whole words -- the next read begins right behind the last base, so the eight
# dead steps of the last block would hash its first bases; 150 and 100: ten and four padding bases (code 0 = A) lie between
SEAM_LENGTHS = ((144, 3), (160, 8), (150, 9), (100, 3))


@pytest.mark.parametrize("length,live", SEAM_LENGTHS)
def test_dead_steps_across_the_seam(engine, oracle, monkeypatch, capfd, length, live):
    """Fixed-length reads are packed back to back.  Reads that end in 40 A's or in random bases, in front of reads that begin with
    40 A's or with random bases: a dead step would hash a homopolymer across that seam.  Every read equals the oracle's, whatever
    its neighbour is; so do reads with a crafted key tie (tests/golden/key_ties.json) whose right element is the last k-mer of the
    read (the last live step) or the last k-mer of the block before the last one."""
    w, n = 11, 3 * 64 + 7
    assert live_of(length, w) == live
    nk = length - K + 1
    rng = random.Random(KT.hash_seed("seam", length))
    seqs = [KT.rand_seq(rng, length) for _ in range(n)]
    tail, head = "A" * 40, "A" * 40
    for r in range(0, n - 1, 4):  # (A-tail, A-head), (random tail, A-head), (A-tail, random head) in turn; every fourth pair plain
        kind = (r // 4) % 4
        if kind in (0, 2):
            seqs[r] = seqs[r][:-40] + tail
        if kind in (0, 1):
            seqs[r + 1] = head + seqs[r + 1][40:]
    ties = 0
    last_block = ((nk - 1) // w) * w
    at = 2
    for target in (nk - 1, last_block - 1):
        for d in range(1, w):
            for side in ("left", "right"):
                e = KT.fixture("minimizer", K, d, side)
                assert e is not None, (d, side)
                a = target - d
                core = e["core"]
                seq = KT.rand_seq(rng, a) + core + KT.rand_seq(rng, length - a - len(core))
                assert len(seq) == length
                h = oracle.nthash(seq, K)[0]
                x, y = int(h[a]), int(h[a + d])
                assert x != y and x >> KT.KEY_SHIFT == y >> KT.KEY_SHIFT, (target, d, side)
                seqs[at] = seq  # (reads 2, 3 mod 4: between the seam pairs; its successor keeps its head)
                at += 3 if at % 4 == 3 else 1
                ties += 1
    assert ties == 4 * (w - 1) and at < n
    data = np.frombuffer("".join(seqs).encode(), np.uint8).copy()
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(length)
    p = engine.params(L.MINIMIZER, K, w=w)
    res = U.both_forms(engine, monkeypatch, capfd, lambda: engine.batch_from_arrays(data, offs), p, "k_minimizer_pk<%d,false>" % w)
    U.check_reads(res, oracle, dict(enumerate(seqs)), w)
    res.close()


# ---- copy-out tails ---------------------------------------------------------------------------------------------------------------
# TAIL_UNITS: (reads, seed) of one partial unit of 150-base reads each, chosen with the oracle so that the units' tuple totals T cover
# every class below; the test computes T and the classes itself and fails on a missing one
TAIL_LEN, TAIL_W = 150, 11
ROWS_PER_TRIP = 8
ALL_CLASSES = {"rows%d" % r for r in range(1, ROWS_PER_TRIP + 1)} | {"whole-trips", "below-64", "1-mod-64", "63-mod-64", "two-trips-or-more"}


def unit_total(oracle, seqs, w, k=K):
    """the tuples a unit of <= 64 reads hands to the copy-out, or None where the oracle cannot tell: a read with two equal 27-bit keys
    in one window may go to the list pass, and so do both reads of a staging column (lanes l, l + 32) with 58 tuples or more"""
    counts = []
    for q in seqs:
        h = np.asarray(oracle.nthash(q, k)[0], np.uint64) >> np.uint64(KT.KEY_SHIFT)
        for d in range(1, w):
            if np.any(h[d:] == h[:-d]):
                return None
        counts.append(len(oracle.minimizer(q, k, w)[0]))
    if max(counts) > 46:  # (a lane that nears the end of its column on its own is parked: PkMin::guard)
        return None
    for lane in range(32, len(counts)):
        if counts[lane] + counts[lane - 32] >= 58:
            return None
    return sum(counts)


def classes_of(t):
    out = set()
    rest = t % (64 * ROWS_PER_TRIP)
    if rest == 0:
        out.add("whole-trips")
    else:
        out.add("rows%d" % (-(-rest // 64)))
    if t < 64:
        out.add("below-64")
    if t % 64 == 1:
        out.add("1-mod-64")
    if t % 64 == 63:
        out.add("63-mod-64")
    if t > 2 * 64 * ROWS_PER_TRIP:
        out.add("two-trips-or-more")
    return out


def tail_unit(n, seed, length=TAIL_LEN):
    return U.rand_reads(seed, n, length)


TAIL_UNITS = (
    (1, 1), (4, 1), (7, 1), (10, 1), (13, 1), (16, 1), (19, 1), (21, 1),  # T = 21, 78, 140, 203, 263, 334, 405, 450: 1 .. 8 rows
    (20, 2),                                                               # T = 447 = 63 (mod 64)
    (46, 4), (46, 8),                                                      # T = 1025 = 1 (mod 64), T = 1024: whole trips only
    (33, 1), (50, 1), (64, 1),                                             # T = 714, 1094, 1405: full trips in front of 4, 2, 6 rows
)
LONG_UNIT = (32, 240, 0x7A12)  # lanes 0 .. 31 alone in their columns: 240-base reads, about 39 tuples each, T = 1258


def test_copyout_tails(engine, oracle, monkeypatch, capfd):
    p = engine.params(L.MINIMIZER, K, w=TAIL_W)
    seen = set()
    units = [(n, TAIL_LEN, seed) for n, seed in TAIL_UNITS] + [LONG_UNIT]
    for n, length, seed in units:
        data, offs = tail_unit(n, seed, length)
        seqs = U.seqs_of(data, offs, range(n))
        t = unit_total(oracle, [seqs[i] for i in range(n)], TAIL_W)
        assert t is not None, (n, length, seed)
        seen |= classes_of(t)
        res = U.both_forms(engine, monkeypatch, capfd, lambda: engine.batch_from_arrays(data, offs), p, "k_minimizer_pk<%d,false>" % TAIL_W)
        assert res.digest()["n_tuples"] == t, (n, length, seed)
        U.check_reads(res, oracle, seqs, TAIL_W)
        res.close()
    assert seen == ALL_CLASSES, sorted(ALL_CLASSES - seen)
