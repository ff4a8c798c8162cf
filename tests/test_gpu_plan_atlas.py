"""Every row of the plan atlas (tests/plan_atlas.py) on the device: the row's switches are set, the batch runs, the plan must name the row's
kernel -- exactly, with the suffixes the row expects and none of the others; a mismatch is a failure with the plan printed, never a
skip -- and then EVERY read is compared: minimizers and syncmers against the line-by-line restatement of the reference's state machines
(hashes, positions, strand bits, status code, the first-window-tie and non-ACGT flags), the other kinds against the oracle's values and
status, and `res.digest()` against the sum over the reads.  Rows with a `digest_env` (the ASCII side launches, whose kernel the plan
string cannot name) run a second time with those switches: same digest.
"""
import numpy as np
import pytest

from bio_amd import _lib as L
from tests import plan_atlas as A

pytestmark = pytest.mark.gpu

KINDS = {"minimizer": L.MINIMIZER, "syncmer": L.SYNCMER, "nthash": L.NTHASH, "kmer": L.KMER, "simhash": L.SIMHASH, "prot_hash": L.PROT_HASH,
         "prot_minimizer": L.PROT_MINIMIZER}
MASK64 = (1 << 64) - 1


def assert_plan(row, plan):
    name = plan["kernel"]
    want = row.name + "".join(s for s in A.SUFFIXES if s in row.suffixes)
    if row.name.endswith(","):  # template arguments the table cannot know follow
        head = name.split(">")[0] + ">"
        assert head.startswith(row.name) and name[len(head):] == want[len(row.name):], (row.id, row.env, plan, want)
    else:
        assert name == want, (row.id, row.env, plan, want)


def expected(O, row, q):
    """-> (status code, flag bits or None, values, positions or None, strands or None) of read q"""
    p = row.p
    k, circ = p["k"], bool(p.get("circular"))
    try:
        if row.kind == "minimizer":
            h, pos, strand, fl = O.minimizer(q, k, p["w"], circ)  # closed=False: the state machine
            return L.ST_OK, fl, h, pos, strand
        if row.kind == "syncmer":
            h, pos, strand, fl = O.syncmer(q, k, p["s"], circ)
            return L.ST_OK, fl, h, pos, strand
        if row.kind == "prot_minimizer":
            if row.alphabet == "protein":
                h, pos, fl = O.protein_minimizer(q, k, p["w"])
            else:
                h, pos, fl = O.protein_minimizer_nt(q, k, p["w"], p.get("codon_table", 1), p.get("frame", 1))
            return L.ST_OK, fl & O.FLAG_FIRST_WINDOW_TIE, h, pos, None
        if row.kind == "nthash":
            return L.ST_OK, None, O.nthash(q, k, p.get("canonical", True), circ)[0], None, None
        if row.kind == "kmer":
            return L.ST_OK, None, O.kmer_codes(q, k, p.get("canonical", True), circ), None, None
        if row.kind == "simhash":
            return L.ST_OK, None, O.simhash(q, k, p["m"], p["scale"], p.get("canonical", True), circ), None, None
        if row.alphabet == "protein":
            return L.ST_OK, None, O.protein_hashes(q, k), None, None
        return L.ST_OK, None, O.protein_hashes_nt(q, k, p.get("codon_table", 1), p.get("frame", 1)), None, None
    except O.OracleError as e:
        assert e.name == "ErrShortSeq", (row.id, e.name, len(q))
        return L.ST_SHORT, None, np.zeros(0, np.uint64), None, None


@pytest.mark.parametrize("rid", [r.id for r in A.ROWS])
def test_row(engine, oracle, monkeypatch, rid):
    row = A.BY_ID[rid]
    for name, v in row.env.items():
        monkeypatch.setenv(name, v)
    seqs = row.reads()
    b = engine.batch(seqs, L.ALPHA_PROTEIN if row.alphabet == "protein" else L.ALPHA_DNA)
    prm = engine.params(KINDS[row.kind], **row.p)
    res = engine.run(b, prm)
    assert_plan(row, res.plan())
    n_tuples = checksum = n_short = n_tie = 0
    positional = row.kind in ("minimizer", "syncmer", "prot_minimizer")
    for i, q in enumerate(seqs):
        st, h, p = res.read(i)
        code, fl, eh, ep, es = expected(oracle, row, q)
        assert (st & L.ST_CODE_MASK) == code, (rid, i, len(q), st)
        assert np.array_equal(h, eh), (rid, i, len(q), len(h), len(eh))
        if positional:
            assert np.array_equal(p & L.POS_MASK, ep if ep is not None else np.zeros(0, np.uint32)), (rid, i, len(q))
            if es is not None:
                assert np.array_equal(p >> 31, es), (rid, i, len(q))
            if fl is not None and row.kind != "prot_minimizer":
                assert (st & 0xF0) == fl, (rid, i, len(q), st, fl)
            elif fl is not None:
                assert bool(st & L.ST_FIRST_WINDOW_TIE) == bool(fl), (rid, i, len(q), st, fl)
            weights = 2 * (p & L.POS_MASK).astype(np.uint64) + np.uint64(1)
        else:
            weights = 2 * np.arange(len(h), dtype=np.uint64) + np.uint64(1)
        n_tuples += len(h)
        n_short += code == L.ST_SHORT
        n_tie += bool(st & L.ST_FIRST_WINDOW_TIE)
        checksum = (checksum + int((h * weights).sum(dtype=np.uint64))) & MASK64
    d = res.digest()
    assert d["n_tuples"] == n_tuples and d["checksum"] == checksum and d["short"] == n_short and d["first_window_tie"] == n_tie, (rid, d, n_tuples, checksum, n_short, n_tie)
    assert n_tuples > 0, rid
    res.close()
    if row.digest_env:
        for name, v in row.digest_env.items():
            monkeypatch.setenv(name, v)
        res2 = engine.run(b, prm)
        assert res2.plan()["kernel"].endswith(A.SIDE), (rid, res2.plan())  # (still a mixed plan: only the side launch's kernel differs)
        assert res2.digest() == d, (rid, d, res2.digest())
        res2.close()
    b.close()
