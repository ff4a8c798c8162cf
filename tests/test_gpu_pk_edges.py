"""k_minimizer_pk at the edges of its work distribution: ticket ends, batch ends, listed reads and full staging columns next to them.

A wavefront takes tickets of tk units (64 reads each) and requests the next ticket two units before its current one ends, so the
next ticket's first unit enters the same one-unit-ahead pipeline of descriptors and words as any other unit.  tk is 8 when every
wavefront of the grid gets a whole ticket, ceil(units / grid) below that (launch.hip), so unit counts around 1, tk and grid * tk give
tickets of one, two, three and eight units, tickets that end with the batch and waves that get no further ticket.  Every read is
compared with the reference's state machine (small batches) or the whole batch with the oracle's digest plus the reads of every
unit at a ticket edge (large ones).  Staged positions are 2 * position + strand in LDS: every read's strand bits are checked too.
"""
import os
import random

import numpy as np
import pytest

from bio_amd import _lib as L

pytestmark = pytest.mark.gpu

K, W = 21, 11
SEED = 0x5EED00E5


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def check_reads(res, oracle, seqs, idx):
    for i in idx:
        st, h, p = res.read(i)
        q = seqs[i]
        if len(q) < K + W - 1:
            assert (st & L.ST_CODE_MASK) == L.ST_SHORT and len(h) == 0, (i, len(q))
            continue
        mh, mp, ms, fl = oracle.minimizer(q, K, W)  # closed=False: the state machine
        assert (st & L.ST_CODE_MASK) == L.ST_OK, (i, len(q))
        assert bool(st & L.ST_FIRST_WINDOW_TIE) == bool(fl & oracle.FLAG_FIRST_WINDOW_TIE), i
        assert np.array_equal(h, mh), (i, len(q))
        assert np.array_equal(p & L.POS_MASK, mp) and np.array_equal(p >> 31, ms), (i, len(q))


@pytest.fixture(scope="module")
def grid(engine):
    b = engine.synth(L.ALPHA_DNA, 64 * 4096, 150, SEED)  # (more units than the grid has wavefronts: the full grid)
    res = engine.run(b, engine.params(L.MINIMIZER, K, w=W))
    pl = res.plan()
    assert pl["kernel"].startswith("k_minimizer_pk<11,false>"), pl
    g = int(pl["grid"])
    res.close()
    b.close()
    return g


def ticket_units(nunits, g):
    return 8 if nunits >= 8 * g else max(1, -(-nunits // g))


@pytest.mark.parametrize("nu", [1, 2, 3, 7, 8, 9])
@pytest.mark.parametrize("ragged", [0, 37])
def test_small_unit_counts(engine, oracle, grid, nu, ragged):
    """unit counts 1 .. tk + 1 (one ticket of one unit per wave): every read against the state machine"""
    rng = random.Random(nu * 101 + ragged)
    n = 64 * nu - ragged if 64 * nu > ragged else 64 * nu
    seqs = [rand_seq(rng, 150) for _ in range(n)]
    seqs[n - 1] = "A" * 150  # a listed read (key ties) in the batch's last unit
    b = engine.batch(seqs)
    res = engine.run(b, engine.params(L.MINIMIZER, K, w=W))
    assert res.plan()["kernel"].startswith("k_minimizer_pk<"), res.plan()
    check_reads(res, oracle, seqs, range(n))
    res.close()
    b.close()


def high_count_reads(oracle, rng, m, at_least):
    """random 150-bp reads that select at least `at_least` tuples each (two in one column fill it: PkLds::PR = 58 rows)"""
    out = []
    while len(out) < m:
        q = rand_seq(rng, 150)
        if len(oracle.minimizer(q, K, W, closed=True)[0]) >= at_least:
            out.append(q)
    return out


@pytest.mark.parametrize("mult,delta", [(1, 1), (2, -1), (2, 1), (3, -1), (3, 0), (3, 1), (8, -1), (8, 0), (8, 1)])
def test_grid_times_tk(engine, oracle, grid, mult, delta):
    """unit counts around grid x tk for tk = 2, 3, 8 (tk = 8 from 8 x grid units on): the whole batch against the oracle's digest,
    and every read of every unit at a ticket edge -- with a listed read in each ticket's last unit and a full staging column in each
    ticket's second-to-last and first unit"""
    nunits = mult * grid + delta
    tk = ticket_units(nunits, grid)
    assert tk == {1: 2, 2: 2 if delta < 0 else 3, 3: 3 if delta <= 0 else 4, 8: 8}[mult]
    n = 64 * nunits
    b0 = engine.synth(L.ALPHA_DNA, n, 150, SEED + mult * 7 + delta)
    data, offs = b0.fetch_ascii(0, n)
    b0.close()
    data = data.copy()
    rng = random.Random(mult * 1000 + delta)
    hot = high_count_reads(oracle, rng, 2, 29)
    edge_units = set()
    nticket = -(-nunits // tk)
    for t in range(nticket):
        u0, ul = t * tk, min(nunits, (t + 1) * tk) - 1
        if t % 97 and t != nticket - 1 and t > 2:
            continue  # every 97th ticket and the batch's first and last ones carry the planted reads (the digest covers the rest)
        for u in {u0, ul, max(u0, ul - 1)}:
            edge_units.add(u)
        r = ul * 64 + 63  # listed read: the last lane of the ticket's last unit
        data[int(offs[r]):int(offs[r + 1])] = ord("A")
        for u in {u0, max(u0, ul - 1)}:  # a full column: lanes 5 and 37 of the ticket's first and second-to-last unit
            for lane, q in zip((5, 37), hot):
                r = u * 64 + lane
                data[int(offs[r]):int(offs[r + 1])] = np.frombuffer(q.encode(), np.uint8)
    b = engine.batch_from_arrays(data, offs)
    res = engine.run(b, engine.params(L.MINIMIZER, K, w=W))
    assert res.plan()["kernel"].startswith("k_minimizer_pk<11,false>"), res.plan()
    assert res.plan()["grid"] == grid
    d = res.digest()
    nt, ck = oracle.batch_run(4, data, offs, K, W, threads=min(16, os.cpu_count() or 1))
    assert (d["n_tuples"], d["checksum"]) == (nt, ck), (nunits, tk)
    idx = [u * 64 + j for u in sorted(edge_units) for j in range(64)]
    seqs = {i: bytes(data[int(offs[i]):int(offs[i + 1])]).decode() for i in idx}
    check_reads(res, oracle, seqs, idx)
    res.close()
    b.close()


def unit_with_total(oracle, rng, total):
    """64 reads whose tuples add up to `total`: short reads (none), then reads searched on the host for an exact count each"""
    seqs, left = [], total
    for i in range(64):
        slots = 64 - i
        want = -(-left // slots)
        if want == 0:
            seqs.append(rand_seq(rng, 20))
            continue
        while True:
            ln = max(K + W - 1, min(400, K + W - 1 + 6 * (want - 1) + rng.randint(-6, 6)))
            q = rand_seq(rng, ln)
            if len(oracle.minimizer(q, K, W, closed=True)[0]) == want:
                break
        seqs.append(q)
        left -= want
    assert left == 0
    return seqs


@pytest.mark.parametrize("total", [0, 1, 63, 64, 127, 128, 511, 512, 513])
def test_unit_totals(engine, oracle, total):
    """one unit's tuple total T at the copy-out's trip edges (64 lanes x 8 rows per trip) between two ordinary units"""
    rng = random.Random(total + 17)
    seqs = [rand_seq(rng, 150) for _ in range(64)] + unit_with_total(oracle, rng, total) + [rand_seq(rng, 150) for _ in range(64)]
    b = engine.batch(seqs)
    res = engine.run(b, engine.params(L.MINIMIZER, K, w=W))
    assert res.plan()["kernel"].startswith("k_minimizer_pk<"), res.plan()
    check_reads(res, oracle, seqs, range(len(seqs)))
    assert sum(len(res.read(i)[1]) for i in range(64, 128)) == total
    res.close()
    b.close()
