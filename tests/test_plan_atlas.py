"""The plan atlas (tests/plan_atlas.py) stays complete and keeps its teeth -- no GPU.

Completeness: the instantiations the default build compiles are read off the headers -- the X-lists (`#define BSK_*_WS(X)`, `BSK_PH_KS`,
`BSK_PROT_K` / `BSK_PROT_KW`), the closed ranges of the `*_supported` functions, and the kernels launch.hip instantiates itself -- and
must equal the atlas rows' `covers` plus `UNREACHABLE`: nothing missing, nothing extra.  The lists of the EXPERIMENTS=1 build
(BSK_SEG_WS, BSK_SYNSEL_WS, k_minimizer_wpr, the compact stream kernels) are left out by name: tests/test_gpu_experiments.py has them.

Teeth, with the oracle alone: the plain reads of every row yield tuples, the crafted reads are where Row.reads says, the boundary
lengths are present and the longest read is the row's limit, every SimHash row holds a read whose counters reach nh, and the reads the
packed kernels must leave to the exact machine (an equal-hash pair inside a window) are in every minimizer and syncmer row.
"""
import os
import re

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from tests import plan_atlas as A

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bio_amd", "csrc")
EXPERIMENT_LISTS = {"BSK_SEG_WS", "BSK_SYNSEL_WS"}  # make EXPERIMENTS=1 only


def _read(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read().replace("\\\n", " ")


def _defines():
    """{macro: [body, ...]} of every `#define BSK_*(X...) ...` in the kernel headers (a list: two translation units may each define one)"""
    out = {}
    for fn in sorted(os.listdir(CSRC)):
        if fn.startswith("kernels_") and fn.endswith(".hpp"):
            for m in re.finditer(r"^#define (BSK_\w+)\(X(?:, *WW)?\) +(.*)$", _read(fn), re.M):
                out.setdefault(m.group(1), []).append(m.group(2).split("//")[0])
    return out


def _xlist(defs, name, which=0):
    """the integers of an X-list, nested lists (BSK_SYNPKL_WS = BSK_SYNPK_WS + ...) expanded"""
    vals = []
    for tok in re.finditer(r"(BSK_\w+)\(X\)|X\((?:WW, *)?(\d+)\)", defs[name][which]):
        vals += _xlist(defs, tok.group(1)) if tok.group(1) else [int(tok.group(2))]
    return vals


def _closed_range(fn_name):
    """(lo, hi) of `bool fn(int x) { return x >= lo && x <= hi; }`"""
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith(".hpp"):
            m = re.search(r"bool %s\(int (\w)\) \{ return \1 >= (\d+) && \1 <= (\d+); \}" % fn_name, _read(fn))
            if m:
                return int(m.group(2)), int(m.group(3))
    raise AssertionError("no closed range found for " + fn_name)


def compiled_set():
    defs = _defines()
    known = {"BSK_PK_WS", "BSK_RING_WS", "BSK_PKD_WS", "BSK_DENSE_WS", "BSK_FAST_WS", "BSK_MINPFT_WS", "BSK_SYNPK_WS", "BSK_SYNPKL_WS", "BSK_SYNPF_WS",
             "BSK_SYNPFL_WS", "BSK_SYN_WS", "BSK_SYN_WIDE_WS", "BSK_PH_KS", "BSK_PROT_K", "BSK_PROT_KW"}
    assert set(defs) - EXPERIMENT_LISTS == known, "a new X-list in the headers: teach tests/test_plan_atlas.py its instantiations (%s)" % sorted(set(defs) ^ known ^ EXPERIMENT_LISTS)
    ph = sorted(_xlist(defs, "BSK_PH_KS", 0) + _xlist(defs, "BSK_PH_KS", 1))
    assert len(defs["BSK_SYN_WS"]) == 2  # k_syncmer.hip's k_syncmer_fast<W> and k_syncmer_ascii.hip's k_syncmer_fast<W,false,true>
    s = set()
    for w in _xlist(defs, "BSK_PK_WS"):
        s |= {"k_minimizer_pk<%d,false>" % w, "k_minimizer_pk<%d,true>" % w}
    for w in _xlist(defs, "BSK_RING_WS"):
        s |= {"k_minimizer_ring<%d,false>" % w, "k_minimizer_ring<%d,true>" % w}
    s |= {"k_minimizer_pkd<%d>" % w for w in _xlist(defs, "BSK_PKD_WS")}
    for w in _xlist(defs, "BSK_DENSE_WS"):
        s |= {"k_minimizer_dense<%d>" % w, "k_minimizer_dense<%d,false,true>" % w}
    s |= {"k_minimizer_fast<%d>" % w for w in _xlist(defs, "BSK_FAST_WS")}
    s |= {"k_minimizer_pft<%d>" % w for w in _xlist(defs, "BSK_MINPFT_WS")}
    s |= {"k_syncmer_pk<%d>" % w for w in _xlist(defs, "BSK_SYNPK_WS")}
    s |= {"k_syncmer_pkl<%d>" % w for w in _xlist(defs, "BSK_SYNPKL_WS")}
    s |= {"k_syncmer_pf<%d>" % w for w in _xlist(defs, "BSK_SYNPF_WS")}
    s |= {"k_syncmer_pfl<%d>" % w for w in _xlist(defs, "BSK_SYNPFL_WS")}
    s |= {"k_syncmer_fast<%d>" % w for w in _xlist(defs, "BSK_SYN_WS", 0) + _xlist(defs, "BSK_SYN_WIDE_WS")}
    s |= {"k_syncmer_fast<%d,false,true>" % w for w in _xlist(defs, "BSK_SYN_WS", 1)}
    for k in ph:
        s |= {"k_prot_hash_fast<%d,false>" % k, "k_prot_hash_fast<%d,true>" % k}
    prot_ks = sorted(_xlist(defs, "BSK_PROT_K", 0) + _xlist(defs, "BSK_PROT_K", 1))
    prot_ws = [int(x) for x in re.findall(r"BSK_PROT_K\(X, *(\d+)\)", defs["BSK_PROT_KW"][0])]
    for w in prot_ws:
        for k in prot_ks:
            s |= {"k_prot_minimizer_fast<%d,%d,false>" % (w, k), "k_prot_minimizer_fast<%d,%d,true>" % (w, k)}
    # the kernels launch.hip instantiates itself, outside its #ifdef BSK_EXPERIMENTS blocks
    src = re.sub(r"#ifdef BSK_EXPERIMENTS.*?#(?:else|endif)", "", _read("launch.hip"), flags=re.S)
    words = {"BSK_SIM_SHORT_WORDS": None, "BSK_SIM_MID_WORDS": None, "BSK_NT_FAST_WORDS": None}
    for name in words:
        hdr = _read("kernels_fast.hpp") + _read("kernels_simhash.hpp")
        words[name] = int(re.search(r"#define %s (\d+)" % name, hdr).group(1))
    for m in re.finditer(r"hipLaunchKernelGGL\(\(?(k_(?:minimizer_generic|nthash_fast|nthash_stream|syncmer|kmer|simhash_fast|simhash|prot_hash|prot_minimizer)\b(?:<[^>]*>)?)", src):
        name = m.group(1).replace(" ", "")
        for macro, v in words.items():
            name = name.replace(macro, str(v))
        if re.fullmatch(r"k_simhash_fast<\d>", name):
            name = name[:-1] + ",%d>" % words["BSK_NT_FAST_WORDS"]
        s.add(name)
    return s


def test_atlas_rows_and_unreachable_are_exactly_the_compiled_set():
    want, have = compiled_set(), A.covered() | set(A.UNREACHABLE)
    assert not (A.covered() & set(A.UNREACHABLE)), sorted(A.covered() & set(A.UNREACHABLE))
    missing, extra = sorted(want - have), sorted(have - want)
    assert not missing, "compiled instantiations without an atlas row: %s" % missing
    assert not extra, "atlas rows for instantiations the build does not compile: %s" % extra
    assert len(want) > 400
    for name, reason in A.UNREACHABLE.items():
        assert reason and "\n" not in reason, name


def test_supported_ranges_say_what_the_lists_say():
    """the planner asks `*_supported`, the launch switches over the X-list: a W in one and not in the other is planned and never launched"""
    defs = _defines()
    for fn, lst in (("pk_minimizer_supported", "BSK_PK_WS"), ("ring_minimizer_supported", "BSK_RING_WS"), ("pkd_minimizer_supported", "BSK_PKD_WS"),
                    ("dense_minimizer_supported", "BSK_DENSE_WS"), ("fast_syncmer_wide_supported", "BSK_SYN_WIDE_WS")):
        lo, hi = _closed_range(fn)
        assert list(range(lo, hi + 1)) == sorted(_xlist(defs, lst)), (fn, lo, hi, lst, _xlist(defs, lst))
    lo, hi = _closed_range("fast_prot_hash_supported")
    assert sorted(_xlist(defs, "BSK_PH_KS", 0) + _xlist(defs, "BSK_PH_KS", 1)) == list(range(lo, hi + 1)), (lo, hi)


def test_limits_the_rows_are_sized_by_are_the_headers():
    pk = int(re.search(r"#define PKNW (\d+)", _read("kernels_pk.hpp")).group(1))
    assert "return 16u * (PKNW - 1);" in _read("kernels_pk.hpp") and A.PK_SHORT_BASES == 16 * (pk - 1)
    ring = _read("kernels_ring.hpp")
    waves = int(re.search(r"#define BSK_RING_WAVES (\d+)", ring).group(1))
    nq = 3 if waves >= 3 else 4
    assert "#define BSK_RING_NQ (BSK_RING_WAVES >= 3 ? 3 : 4)" in ring and "return 16u * (4 * BSK_RING_NQ - 1);" in ring and A.RING_SHORT_BASES == 16 * (4 * nq - 1)
    synpk, synpf = _read("kernels_syncmer_pk.hpp"), _read("kernels_syncmer_pf.hpp")
    rows_s, rows_l, nw_l = (int(re.search(r"#define %s (\d+)" % n, synpk).group(1)) for n in ("BSK_SYNPK_ROWS", "BSK_SYNPKL_ROWS", "BSK_SYNPKL_NW"))
    assert A.SYN_PAIR_ROWS == {False: rows_s, True: rows_l} and A.SYN_SHORT_BASES == 16 * (pk - 2) and A.SYN_LONG_BASES == 16 * (nw_l - 2)
    m = re.search(r"typedef SynPfLdsT<PKNW, (\d+), (\d+), true, \d+> SynPfLds;", synpf)
    ml = re.search(r"typedef SynPfLdsT<(\d+), (\d+), (\d+), false, \d+> SynPfLdsL;", synpf)
    assert A.SYN_PF_MASK_ROWS == {False: int(m.group(1)), True: int(ml.group(2))} and A.SYN_PF_TUPLES == {False: int(m.group(2)), True: int(ml.group(3))} and int(ml.group(1)) == nw_l
    table = _read("planner_table.hpp")
    assert A.SYN_TILE_MIN == int(re.search(r"syn_tile_min_bases = (\d+);", table).group(1))
    assert "slab_sel_num = 2.6;" in table and "slab_sel_pad = 16;" in table and "syn_sel_num = 1.5;" in table and "pf_list_fill = 0.86;" in table
    nt = int(re.search(r"#define BSK_NT_FAST_WORDS (\d+)", _read("kernels_fast.hpp")).group(1))
    sim = _read("kernels_simhash.hpp")
    short, mid = (int(re.search(r"#define %s (\d+)" % n, sim).group(1)) for n in ("BSK_SIM_SHORT_WORDS", "BSK_SIM_MID_WORDS"))
    assert A.STREAM_BASES == 16 * (nt - 2) and A.SIM_BASES == {short: 16 * (short - 2), mid: 16 * (mid - 2), nt: 16 * (nt - 2)}


def _oracle_call(O, row, q):
    """what the reference yields for read q of the row -> (values, positions or None); raises O.OracleError"""
    p = row.p
    k, circ = p["k"], bool(p.get("circular"))
    if row.kind == "minimizer":
        return O.minimizer(q, k, p["w"], circ)[:2]
    if row.kind == "syncmer":
        return O.syncmer(q, k, p["s"], circ)[:2]
    if row.kind == "nthash":
        return O.nthash(q, k, p.get("canonical", True), circ)[0], None
    if row.kind == "kmer":
        return O.kmer_codes(q, k, p.get("canonical", True), circ), None
    if row.kind == "simhash":
        return O.simhash(q, k, p["m"], p["scale"], p.get("canonical", True), circ), None
    if row.kind == "prot_hash":
        return (O.protein_hashes(q, k) if row.alphabet == "protein" else O.protein_hashes_nt(q, k, p.get("codon_table", 1), p.get("frame", 1))), None
    if row.alphabet == "protein":
        return O.protein_minimizer(q, k, p["w"])[:2]
    return O.protein_minimizer_nt(q, k, p["w"], p.get("codon_table", 1), p.get("frame", 1))[:2]


def _has_equal_pair_in_a_window(O, row, q):
    """two equal hashes inside one window of the machine: w k-mers (minimizers), 2 (k - s) s-mers (syncmers)"""
    p = row.p
    try:
        h = O.nthash(q, p["k"] if row.kind == "minimizer" else p["s"])[0]
    except O.OracleError:
        return False
    span = p["w"] if row.kind == "minimizer" else 2 * (p["k"] - p["s"])
    if span < 2 or len(h) < 2:
        return False
    span = min(span, len(h))
    win = np.sort(sliding_window_view(h, span), axis=1)
    return bool((win[:, 1:] == win[:, :-1]).any())


@pytest.mark.parametrize("family", sorted({r.id.split("<")[0] for r in A.ROWS}))
def test_rows_have_teeth(oracle, family):
    O = oracle
    for row in (r for r in A.ROWS if r.id.split("<")[0] == family):
        seqs = row.reads()
        assert seqs == row.reads(), row.id  # seeded: both modules build the same reads
        assert len(seqs) == row.n + len(row.extra) and len(seqs) <= 400, row.id
        longest = max(len(q) for q in seqs)
        assert longest == max(row.lens + row.limits), (row.id, longest)  # the longest read decides the plan
        assert [len(seqs[i]) for i in row.limit_indices()] == list(row.limits), row.id
        assert seqs[3] == "" and len(set(seqs[1])) == 1 and len(seqs[2]) == max(row.min_len() - 1, 0), row.id
        if not row.circular:
            with pytest.raises(O.OracleError) as e:
                _oracle_call(O, row, seqs[2])
            assert e.value.name == "ErrShortSeq", (row.id, e.value.name)
            _oracle_call(O, row, seqs[2] + "A")  # ... and one letter more is accepted
        plain = row.plain_indices()
        assert len(plain) >= 40, row.id
        with_tuples = 0
        for i in plain:
            q = seqs[i]
            assert set(q) <= set(A.AA if row.alphabet == "protein" else "ACGT"), (row.id, i)
            try:
                with_tuples += len(_oracle_call(O, row, q)[0]) > 0
            except O.OracleError:
                pass
        assert with_tuples * 2 >= len(plain), (row.id, with_tuples, len(plain))  # (a row whose shortest length class is below the constructor's limit still keeps half)
        if row.mixed:
            flagged = sum(any(c not in "ACGT" for c in q) for q in seqs[:row.n])
            assert row.n // 4 <= flagged <= row.n // 2, (row.id, flagged)
        if row.kind in ("minimizer", "syncmer") and (row.p.get("w", 2) >= 2):
            listed = sum(_has_equal_pair_in_a_window(O, row, q) for q in seqs)
            span = row.p["w"] if row.kind == "minimizer" else 2 * (row.p["k"] - row.p["s"])
            # the homopolymer, and (windows that span a whole repeat unit of up to six letters) low-complexity reads: the exact machine's
            assert listed >= (2 if span > 6 else 1), (row.id, listed)
            assert listed * 4 <= len(seqs), (row.id, listed)  # ... and no more than the list of reads takes
        if row.kind == "simhash":
            k, m = row.p["k"], row.p["m"]
            nh = k - m + 1
            top = 0
            for q in [seqs[1]] + list(row.extra):
                hm = O.nthash(q, m, row.p.get("canonical", True))[0]
                bits = ((hm[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.int64)
                counts = sliding_window_view(bits, nh, axis=0).sum(axis=2)  # counter of every bit over the nh m-mers of every k-mer
                top = max(top, int(counts.max()))
            assert top == nh, (row.id, top, nh)  # a counter with every plane set: the threshold compare's longest borrow chain


def test_fallback_rows_hold_a_read_that_outgrows_its_slab(oracle):
    rows = [r for r in A.ROWS if "fallback" in r.id]
    assert len(rows) >= 10
    for row in rows:
        seqs = row.reads()
        k, w = row.p["k"], row.p["w"]
        nwin = max(len(q) for q in seqs) - k - w + 2
        h = _oracle_call(oracle, row, seqs[1])[0]
        assert len(h) == nwin > A.slab_tuples(nwin, w) + 15, (row.id, len(h), nwin)  # (the slab is rounded up to whole lines of 16 tuples)
    # ... and the rows of the same kernels that must NOT fall back keep every read within its slab
    for row in (r for r in A.ROWS if r.lc_max):
        seqs = row.reads()
        p = row.p
        longest = max(len(q) for q in seqs)
        plen = longest // 3 if (row.kind == "prot_minimizer" and row.alphabet == "dna") else longest
        cap = A.slab_tuples(plen - p["k"] - p["w"] + 2, p["w"])
        for i in [1] + list(range(0, row.n, 10)):
            try:
                n = len(_oracle_call(oracle, row, seqs[i])[0])
            except oracle.OracleError:
                n = 0
            assert n <= cap, (row.id, i, n, cap)
