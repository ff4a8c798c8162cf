"""k_minimizer_pk's fixed-length form (k_minimizer_pk<W, false, true>) against the oracle and against its general form.

A batch whose reads all have one length L <= 240 and start at word r * ceil(L / 16) takes the fixed-length form: no descriptor
loads, length and window counts as launch constants, ceil(L / 16) / 4 + 1 16-byte loads per read.  The plan string does not name
the form; under BSK_TIMING=1 the launch says which one it took, and BSK_PK_NO_UNIFORM=1 forces the general one.  A launch of whole
eight-unit tickets hands out its last round as tickets of three units (BSK_PK_TAIL, BSK_PK_SMALL); the same BSK_TIMING line names
the first small ticket and the small tickets' units, so a run with these set shows that they took effect.  Every case runs both forms on
the same reads and compares them word for word (offsets, status bytes, hashes, positions with their strand bit, digest), and the
reads -- all of them, or a seeded sample of a large batch -- with the reference's state machine.
"""
import json
import os
import random
import re

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S

pytestmark = pytest.mark.gpu

K = 21
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "key_ties.json")
# (the unit-row and per-read-slab kernels would take some of these shapes: every case here is k_minimizer_pk's)
BASE_ENV = {"BSK_NO_RING": "1", "BSK_NO_DENSE": "1", "BSK_TIMING": "1"}
CODE = np.full(256, 0, np.uint8)
for _i, _c in enumerate("ACGT"):
    CODE[ord(_c)] = _i


def rand_reads(seed, n, length):
    rng = np.random.default_rng(seed)
    data = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n * length)].copy()
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(length)
    return data, offs


def seqs_of(data, offs, idx):
    return {i: bytes(data[int(offs[i]):int(offs[i + 1])]).decode() for i in idx}


def pack(data, n, length):
    """2-bit words of n reads of one length, read r at word r * wpr (16 bases per word, the first base in the lowest bits)"""
    wpr = (length + 15) // 16
    codes = np.zeros((n, wpr * 16), np.uint64)
    codes[:, :length] = CODE[data].reshape(n, length)
    words = (codes.reshape(n, wpr, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=2).astype(np.uint32)
    return words, wpr


def check_reads(res, oracle, seqs, w, k=K):
    for i, q in seqs.items():
        st, h, p = res.read(i)
        if len(q) < k + w - 1:
            assert (st & L.ST_CODE_MASK) == L.ST_SHORT and len(h) == 0, (i, len(q))
            continue
        mh, mp, ms, fl = oracle.minimizer(q, k, w)  # closed=False: the state machine
        assert (st & L.ST_CODE_MASK) == L.ST_OK, (i, len(q))
        assert bool(st & L.ST_FIRST_WINDOW_TIE) == bool(fl & oracle.FLAG_FIRST_WINDOW_TIE), i
        assert np.array_equal(h, mh), (i, len(q))
        assert np.array_equal(p & L.POS_MASK, mp) and np.array_equal(p >> 31, ms), (i, len(q))


def forms(err):
    return set(re.findall(r"k_minimizer_pk: (\S+) form", err))


def run_form(engine, monkeypatch, capfd, make_batch, p, general, want_form, want_plan):
    """one run with the switch set or not -> the open result (the caller closes it); the launch must have said `want_form`"""
    for v, x in BASE_ENV.items():
        monkeypatch.setenv(v, x)
    if general:
        monkeypatch.setenv("BSK_PK_NO_UNIFORM", "1")
    else:
        monkeypatch.delenv("BSK_PK_NO_UNIFORM", raising=False)
    b = make_batch()
    capfd.readouterr()
    res = engine.run(b, p)
    said = forms(capfd.readouterr().err)
    b.close()
    assert res.plan()["kernel"].startswith(want_plan), res.plan()
    assert said == {want_form}, (said, want_form)
    return res


def fetched(res):
    """a result's arrays and digest on the host, for same_results (a large reference is fetched once)"""
    return res.fetch(), res.digest()


def same_results(a, b):
    """a: a result; b: a result or fetched(result)"""
    fa, da = fetched(a)
    fb, db = b if isinstance(b, tuple) else fetched(b)
    for x, y, what in zip(fa, fb, ("offsets", "status", "hash", "pos")):
        assert np.array_equal(x, y), what
    assert da == db


def both_forms(engine, monkeypatch, capfd, make_batch, p, want_plan, uniform=True):
    """-> the result of the run WITHOUT the switch, after comparing it with the run with the switch set"""
    gen = run_form(engine, monkeypatch, capfd, make_batch, p, True, "general", want_plan)
    res = run_form(engine, monkeypatch, capfd, make_batch, p, False, "fixed-length" if uniform else "general", want_plan)
    same_results(res, gen)
    gen.close()
    return res


COUNTS = (1, 63, 64, 65, 8 * 64 - 1, 8 * 64 + 1)  # a partial last unit, tickets of fewer than three units
# 30: every read SHORT (w = 11); 31: nk = W, block 0 + drain; 32: nk = W + 1; 42, 53: nk a multiple of W; 43: nk = 2 W + 1;
# 240: the last length the registers hold; 241: the general LONG kernel
LENGTHS = [(ln, 11) for ln in (30, 31, 32, 42, 43, 53, 150, 240, 241)] + [(ln, w) for w in (2, 13) for ln in (30, 31, 32, 42)]


@pytest.mark.parametrize("length,w", LENGTHS)
def test_lengths_and_counts(engine, oracle, monkeypatch, capfd, length, w):
    p = engine.params(L.MINIMIZER, K, w=w)
    long_reads = length > 240
    for n in COUNTS:
        data, offs = rand_reads(length * 1000 + w * 37 + n, n, length)
        res = both_forms(engine, monkeypatch, capfd, lambda: engine.batch_from_arrays(data, offs), p,
                         "k_minimizer_pk<%d,%s>" % (w, "true" if long_reads else "false"), uniform=not long_reads)
        check_reads(res, oracle, seqs_of(data, offs, range(n)), w)
        res.close()


def tickets(err):
    """(tk, tk_t0, tk_small) of every k_minimizer_pk launch that the BSK_TIMING lines name"""
    return [tuple(int(x) for x in m) for m in re.findall(r"k_minimizer_pk: \S+ form, tk (\d+), tk_t0 (\d+), tk_small (\d+)", err)]


def run_tail(engine, monkeypatch, capfd, b, n, p, tail, small, general=False):
    """one run of batch b with BSK_PK_TAIL / BSK_PK_SMALL set (None: the defaults, one round of three units) -> the open result;
    the launch must have said the ticket numbers that launch.hip's rule gives for its grid"""
    for v, x in ((("BSK_PK_TAIL", tail), ("BSK_PK_SMALL", small))):
        if x is None:
            monkeypatch.delenv(v, raising=False)
        else:
            monkeypatch.setenv(v, str(x))
    if general:
        monkeypatch.setenv("BSK_PK_NO_UNIFORM", "1")
    else:
        monkeypatch.delenv("BSK_PK_NO_UNIFORM", raising=False)
    capfd.readouterr()
    res = engine.run(b, p)
    err = capfd.readouterr().err
    assert forms(err) == {"general" if general else "fixed-length"}, err
    nunits = (n + 63) // 64
    grid = res.plan()["grid"]
    assert nunits >= grid * 8  # whole tickets
    t, s = (1 if tail is None else tail), (3 if small is None else small)
    want = (0, (nunits - min(t * grid * 8, nunits)) // 8, s) if t else (0, 0, 0)
    assert tickets(err) == [want], (err, want)
    return res


N_BIG = 2048 * 8 * 64 + 37  # 16 385 units of 150-base reads, the last one of 37 reads
# the launch's last tickets: none smaller, the default (one round of the grid as tickets of three units), two rounds of four units
TAILS = ((0, 3), (None, None), (2, 4))


def test_full_tickets_and_tail(engine, oracle, monkeypatch, capfd):
    """2048 x 8 x 64 + 37 reads on the whole grid: every wavefront gets a whole ticket and no more than about one, so the last
    round IS the launch (tk_t0 = 0 on a grid of 2 048 wavefronts) and every ticket has eight, three or four units, by the setting.
    Both forms, each setting, a partial last unit; the handover from eight-unit tickets to small ones is test_ticket_handover's."""
    n, length, w = N_BIG, 150, 11
    p = engine.params(L.MINIMIZER, K, w=w)
    for v, x in BASE_ENV.items():
        monkeypatch.setenv(v, x)
    b = engine.synth(L.ALPHA_DNA, n, length, 0xF1CED)
    ref = run_tail(engine, monkeypatch, capfd, b, n, p, 0, 3, general=True)
    assert ref.plan()["kernel"].startswith("k_minimizer_pk<11,false>"), ref.plan()
    want = fetched(ref)
    ref.close()
    for tail, small in TAILS[1:]:
        other = run_tail(engine, monkeypatch, capfd, b, n, p, tail, small)
        same_results(other, want)
        other.close()
    res = run_tail(engine, monkeypatch, capfd, b, n, p, 0, 3)
    same_results(res, want)
    check_sample(b, res, oracle, n, w)


def test_ticket_handover(engine, oracle, monkeypatch, capfd):
    """The same batch on two wavefronts per CU (BSK_WAVES_PER_CU=2): 16 385 units are several rounds of such a grid, so tickets
    below tk_t0 > 0 have eight units and the ones from there on three or four -- the waves walk from the one kind into the other
    (ticket_unit / ticket_end on both sides of u0s, the next ticket taken ahead across the border), as the headline launch does.
    Fixed-length form with every setting, and the general form with the default one, against the general form without small tickets,
    word for word; a seeded sample against the oracle."""
    n, length, w = N_BIG, 150, 11
    p = engine.params(L.MINIMIZER, K, w=w)
    for v, x in BASE_ENV.items():
        monkeypatch.setenv(v, x)
    monkeypatch.setenv("BSK_WAVES_PER_CU", "2")
    b = engine.synth(L.ALPHA_DNA, n, length, 0xF1CED)
    ref = run_tail(engine, monkeypatch, capfd, b, n, p, 0, 3, general=True)
    assert ref.plan()["kernel"].startswith("k_minimizer_pk<11,false>"), ref.plan()
    nunits, grid = (n + 63) // 64, ref.plan()["grid"]
    assert 2 * grid * 8 < nunits, grid  # eight-unit tickets in front of two rounds of small ones: tk_t0 > 0 with every setting below
    want = fetched(ref)
    ref.close()
    res = None
    for general, (tail, small) in ((True, TAILS[1]), (False, TAILS[0]), (False, TAILS[2]), (False, TAILS[1])):
        if res is not None:
            res.close()
        res = run_tail(engine, monkeypatch, capfd, b, n, p, tail, small, general=general)
        same_results(res, want)
    check_sample(b, res, oracle, n, w)


def check_sample(b, res, oracle, n, w):
    """a seeded sample of reads against the reference's state machine; closes the batch and the result"""
    rng = random.Random(150)
    sample = {0, 63, 64, n - 38, n - 37, n - 1}  # (the batch's ends, then seeded reads up to 256)
    while len(sample) < 256:
        sample.add(rng.randrange(n))
    sample = sorted(sample)
    for i in sample:
        data, offs = b.fetch_ascii(i, 1)
        q = bytes(data[int(offs[0]):int(offs[1])]).decode()
        _, st, h, pos = res.fetch(i, 1)
        mh, mp, ms, fl = oracle.minimizer(q, K, w)
        assert (int(st[0]) & L.ST_CODE_MASK) == L.ST_OK, i
        assert bool(int(st[0]) & L.ST_FIRST_WINDOW_TIE) == bool(fl & oracle.FLAG_FIRST_WINDOW_TIE), i
        assert np.array_equal(h, mh) and np.array_equal(pos & L.POS_MASK, mp) and np.array_equal(pos >> 31, ms), i
    b.close()
    res.close()


@pytest.mark.parametrize("layout", ["stride", "shuffled", "gap"])
def test_from_packed_offsets(engine, oracle, monkeypatch, capfd, layout):
    """fixed-length reads given as packed words: only reads at r * wpr take the fixed-length form, and the results do not depend on it"""
    n, length, w = 8 * 64 + 1, 150, 11
    p = engine.params(L.MINIMIZER, K, w=w)
    data, offs = rand_reads(4242, n, length)
    words, wpr = pack(data, n, length)
    place = np.arange(n, dtype=np.uint64)  # read r sits in row place[r] of the word array
    if layout == "shuffled":
        place = np.random.default_rng(7).permutation(n).astype(np.uint64)
    rows = np.zeros((n, wpr), np.uint32)
    rows[place.astype(np.int64)] = words
    flat = rows.reshape(-1)
    first = place * np.uint64(wpr)
    if layout == "gap":  # three words of padding in front of read 100: every read from there on starts off the stride
        flat = np.concatenate([flat[:100 * wpr], np.zeros(3, np.uint32), flat[100 * wpr:]])
        first[100:] += np.uint64(3)
    desc = (first << np.uint64(24)) | np.uint64(length)
    res = both_forms(engine, monkeypatch, capfd, lambda: engine.batch_from_packed(flat, desc), p, "k_minimizer_pk<11,false>", uniform=layout == "stride")
    ref = run_form(engine, monkeypatch, capfd, lambda: engine.batch_from_arrays(data, offs), p, False, "fixed-length", "k_minimizer_pk<11,false>")
    same_results(res, ref)
    ref.close()
    check_reads(res, oracle, seqs_of(data, offs, range(n)), w)
    res.close()


def test_listed_tied_flagged_reads(engine, oracle, monkeypatch, capfd):
    """poly-A reads (key ties and a full column: the list pass), a crafted pair of equal 27-bit keys, and -- in a second batch -- a read
    with an N, whose side launch keeps the whole batch on the general form"""
    n, length, w = 3 * 64 + 5, 150, 11
    p = engine.params(L.MINIMIZER, K, w=w)
    data, offs = rand_reads(99, n, length)
    data = data.copy()
    ties = [e for e in json.load(open(GOLDEN))["minimizer"] if e["k"] == K and e["d"] < w]
    left = next(e for e in ties if e["smaller"] == "left")
    right = next(e for e in ties if e["smaller"] == "right")
    for r, e in ((7, left), (70, right), (n - 2, left)):  # (the last one in the batch's partial last unit)
        core = np.frombuffer(e["core"].encode(), np.uint8)
        data[int(offs[r]) + 40:int(offs[r]) + 40 + len(core)] = core
    for r in (5, 37, 64 + 63, n - 1, n - 4):  # lanes 5 and 37 share a staging column
        data[int(offs[r]):int(offs[r + 1])] = ord("A")
    res = both_forms(engine, monkeypatch, capfd, lambda: engine.batch_from_arrays(data, offs), p, "k_minimizer_pk<11,false>")
    check_reads(res, oracle, seqs_of(data, offs, range(n)), w)
    res.close()
    data[int(offs[66]) + 75] = ord("N")
    data[int(offs[n - 3]) + 3] = ord("N")
    res = both_forms(engine, monkeypatch, capfd, lambda: engine.batch_from_arrays(data, offs), p, "k_minimizer_pk<11,false>", uniform=False)
    assert "ASCII side launch" in res.plan()["kernel"]
    whole = res.fetch()
    clean = [i for i in range(n) if i not in (66, n - 3)]
    check_reads(res, oracle, seqs_of(data, offs, clean), w)
    for i in (66, n - 3):
        assert whole[1][i] & L.ST_HAS_NON_ACGT, i
    res.close()


def test_pipeline_chunks(engine, oracle, monkeypatch, capfd):
    """three chunks of fixed-length reads through the streaming path, with and without the switch: the whole batch's digest, the
    oracle's; every chunk's launch (the pipeline's workers read the switches when they start) must have taken the form asked for"""
    n, length, w = 2 * 4096 + 1000, 150, 11
    p = engine.params(L.MINIMIZER, K, w=w)
    data, offs = rand_reads(31337, n, length)
    nt, ck = oracle.batch_run(4, data, offs, K, w, threads=min(16, os.cpu_count() or 1))
    for v, x in BASE_ENV.items():
        monkeypatch.setenv(v, x)
    for general in (True, False):
        if general:
            monkeypatch.setenv("BSK_PK_NO_UNIFORM", "1")
        else:
            monkeypatch.delenv("BSK_PK_NO_UNIFORM", raising=False)
        capfd.readouterr()
        st = S.Engine.pipeline_memory(data, offs, p, n_streams=2, chunk_records=4096, fetch=True)
        said = re.findall(r"k_minimizer_pk: (\S+) form", capfd.readouterr().err)
        assert (st["records"], st["chunks"], st["tuples"], st["checksum"]) == (n, 3, nt, ck), general
        assert len(said) >= 3 and set(said) == {"general" if general else "fixed-length"}, (said, general)  # (a launch per chunk)
        b = engine.batch_from_arrays(data, offs)
        res = engine.run(b, p)
        said = forms(capfd.readouterr().err)
        d = res.digest()
        res.close()
        b.close()
        assert said == {"general" if general else "fixed-length"}, (said, general)
        assert (d["n_tuples"], d["checksum"]) == (nt, ck), general
