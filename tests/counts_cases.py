"""Counted sketch sets (include/biosketch.h "counted sketch sets", bio_amd/csrc/counts.hip, setops.hip): references and crafted inputs.

ref_counted is the header's rule in NumPy -- keep v <= MaxUint64 / scale, then np.unique(..., return_counts=True) -- over values that
come from the CPU ORACLE (tests/sets_cases.values_of), never from the engine.  The algebra's reference is NumPy on host arrays: np.unique
with np.add.at and a clamp at 2^32 - 1 for ADD, np.isin for KEEP / DROP.  Every builder returns its input with what it claims about it;
tests/test_counts_cases.py re-derives the claims.  Nothing here imports the engine."""
import os
import re

import numpy as np

from tests import sets_cases as SC
from tests import setops_cases as SO

U64, U32 = np.uint64, np.uint32
ADD, KEEP, DROP = 0, 1, 2
OPS = (ADD, KEEP, DROP)
SAT = 2**32 - 1
ROOT = SO.ROOT
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def read_chunk(path=os.path.join(ROOT, "bio_amd", "csrc", "counts.hip")):
    """CNT_CHUNK of counts.hip: the elements a workgroup of the run-length kernels owns"""
    d = {}
    for name, val in re.findall(r"^#define\s+(CNT_\w+)\s+\(?([\w *]+?)\)?\s*$", open(path).read(), re.M):
        if name == "CNT_NONE":
            continue
        prod = 1
        for f in val.split("*"):
            f = f.strip()
            prod *= d[f] if f in d else int(f, 0)
        d[name] = prod
    return d["CNT_CHUNK"]


# ---- the reference: construction ----
def ref_counted(values_per_read, scale, whole):
    """-> (offsets, values, counts): per read (or for all reads together) the values <= MaxUint64 / scale, each once, with how often it occurred"""
    mh = U64(SC.maxhash(scale))
    per = [np.asarray(v, U64) for v in values_per_read]
    per = [v[v <= mh] for v in per]
    if whole:
        per = [np.concatenate(per) if per else np.zeros(0, U64)]
    vs, cs = [], []
    for v in per:
        u, c = np.unique(v, return_counts=True)
        vs.append(u.astype(U64))
        cs.append(c.astype(U32))
    offs, vals = SC.collection(vs)
    return offs, vals, (np.concatenate(cs) if cs and offs[-1] else np.zeros(0, U32))


def ref_counted_rows(v2d, scale, whole):
    """ref_counted for reads of one count (v2d[i]: read i's values) without a Python loop over the reads"""
    v = np.sort(np.asarray(v2d, U64), axis=1)
    ok = v <= U64(SC.maxhash(scale))
    if whole:
        u, c = np.unique(v[ok], return_counts=True)
        return np.array([0, len(u)], U64), u.astype(U64), c.astype(U32)
    head = ok.copy()
    head[:, 1:] &= v[:, 1:] != v[:, :-1]
    offs = np.zeros(len(v) + 1, U64)
    offs[1:] = np.cumsum(head.sum(1))
    # a head's run ends at the next head, the first filtered value or the row's end
    n, m = v.shape
    stop = np.where(head | ~ok, np.arange(m)[None, :], m)
    nxt = np.minimum.accumulate(np.concatenate([stop[:, 1:], np.full((n, 1), m)], axis=1)[:, ::-1], axis=1)[:, ::-1]
    return offs, v[head], (nxt - np.arange(m)[None, :])[head].astype(U32)


# ---- the reference: algebra, filter, totals ----
def ranks(offs):
    """every value's rank inside its set"""
    offs = np.asarray(offs, np.int64)
    return np.arange(int(offs[-1])) - np.repeat(offs[:-1], np.diff(offs))


def counts_a(offs):
    return (1 + ranks(offs) % 7).astype(U32)


def counts_b(offs):
    return (1000 * (1 + ranks(offs) % 5)).astype(U32)


def ones(offs):
    return np.ones(int(offs[-1]), U32)


def ref_pair(a, ca, b, cb, op):
    if op == ADD:
        u, inv = np.unique(np.concatenate([a, b]), return_inverse=True)
        s = np.zeros(len(u), U64)
        np.add.at(s, inv, np.concatenate([ca, cb]).astype(U64))
        return u.astype(U64), np.minimum(s, U64(SAT)).astype(U32)
    m = np.isin(a, b)
    if op == DROP:
        m = ~m
    return a[m], ca[m]


def ref_op(a, b, op):
    """(offsets, values, counts) x (offsets, values, counts) -> the same; counts None: an uncounted operand (1 per value); an operand of one
    set is combined with every set of the other"""
    ca = ones(a[0]) if a[2] is None else a[2]
    cb = ones(b[0]) if b[2] is None else b[2]
    sa, sb = list(zip(SO.split(a[0], a[1]), SO.split(a[0], ca))), list(zip(SO.split(b[0], b[1]), SO.split(b[0], cb)))
    if len(sa) != len(sb):
        assert len(sa) == 1 or len(sb) == 1
        if len(sb) == 1:
            sb = sb * len(sa)
        else:
            sa = sa * len(sb)
    out = [ref_pair(x, cx, y, cy, op) for (x, cx), (y, cy) in zip(sa, sb)]
    offs, vals = SO.collection([v for v, _ in out])
    return offs, vals, (np.concatenate([c for _, c in out]).astype(U32) if out and offs[-1] else np.zeros(0, U32))


def pair_t(a_offs, b_offs):
    na, nb = np.diff(a_offs).astype(np.int64), np.diff(b_offs).astype(np.int64)
    if len(na) == len(nb):
        return na + nb
    return na + nb[0] if len(nb) == 1 else na[0] + nb


def path_counts(a_offs, b_offs, caps):
    t = pair_t(a_offs, b_offs)
    return [int((t <= caps["SO_GROUP_CAP"]).sum()), int(((t > caps["SO_GROUP_CAP"]) & (t <= caps["SO_WAVE_CAP"])).sum()), int((t > caps["SO_WAVE_CAP"]).sum())]


def ref_filter(s, lo, hi):
    offs, vals, c = s
    keep = (c >= lo) & (c <= hi)
    kept = np.concatenate([[0], np.cumsum(keep)])
    return kept[offs.astype(np.int64)].astype(U64), vals[keep], c[keep]


def ref_totals(s):
    offs, _, c = s
    cs = np.concatenate([[0], np.cumsum(c.astype(object))]) if c is not None else np.arange(int(offs[-1]) + 1, dtype=object)
    o = offs.astype(np.int64)
    return np.array([int(cs[o[i + 1]] - cs[o[i]]) for i in range(len(o) - 1)], U64)


# ---- builders: construction ----
def kmer_stream(oracle, n, k=21, seed=211):
    """n reads of k bases, read i = bases [i, i + k) of one random sequence: ONE oracle call gives every read's only value -> (reads, values)"""
    rng = np.random.default_rng(seed)
    s = _ACGT[rng.integers(0, 4, n + k - 1)]
    h = np.asarray(oracle.kmer_codes(s.tobytes().decode(), k, True, False), U64)
    assert len(h) == n
    text = s.tobytes().decode()
    return [text[i:i + k] for i in range(n)], h


RUN_LENGTHS = (1, 2047, 2048, 2049, 5000)


def run_layout(chunk):
    """run lengths in sorted order: for every L of RUN_LENGTHS a run that ENDS at a multiple of `chunk` and one that SPANS one (starts
    L // 2 + 1 before it; L = 1 cannot span: it starts at the border), singles in between -> (lengths, [(L, how, start)])"""
    lengths, facts, at = [], [], 0

    def pad_to(start):
        nonlocal at
        lengths.extend([1] * (start - at))
        at = start

    for L in RUN_LENGTHS:
        for how in ("ends", "spans"):
            off = L if how == "ends" else L // 2 + 1 if L > 1 else 0
            m = (at + off + chunk - 1) // chunk + 1
            start = m * chunk - off
            pad_to(start)
            facts.append((L, how, start))
            lengths.append(L)
            at += L
    pad_to(at + 3)
    return lengths, facts


def runs_case(oracle, chunk, seed=223):
    """one-value KMER reads whose whole-batch sorted order holds run_layout(chunk): the value of sorted rank j is read lengths[j] times,
    the copies scattered over the batch"""
    lengths, facts = run_layout(chunk)
    reads, h = kmer_stream(oracle, len(lengths), seed=seed)
    assert len(np.unique(h)) == len(h)
    order = np.argsort(h)
    idx = np.repeat(order, lengths)
    idx = np.random.default_rng(seed).permutation(idx)
    return dict(kind="kmer", pk=dict(k=21), reads=[reads[i] for i in idx], values=h[idx], lengths=np.array(lengths), facts=facts)


def neighbours_case(oracle, seed=227):
    """KMER k = 21 reads: 2, 3 and 130 copies of one read in a row, and a read followed by the one-value read of its LARGEST value, a
    one-value read of the next read's SMALLEST value in front of it.  facts: name -> first index"""
    rng = np.random.default_rng(seed)
    k = 21
    reads, facts = [], {}

    def vals(q):
        return np.asarray(SC.oracle_values(oracle, "kmer", dict(k=k), q), U64)

    for copies in (2, 3, 130):
        q = SC.rand_read(rng, int(rng.integers(40, 70)))
        facts["copies%d" % copies] = len(reads)
        reads += [q] * copies
        reads.append(SC.rand_read(rng, 50))
    x = SC.rand_read(rng, 60)
    v = vals(x)
    facts["max_then_single"] = len(reads)
    reads += [x, x[int(np.argmax(v)):int(np.argmax(v)) + k]]
    y = SC.rand_read(rng, 60)
    v = vals(y)
    facts["single_then_min"] = len(reads)
    reads += [y[int(np.argmin(v)):int(np.argmin(v)) + k], y]
    return dict(kind="kmer", pk=dict(k=k), reads=reads, facts=facts)


def empty_cases():
    return {"no reads": [], "too short": ["ACGT", "", "ACGTACGTAC"] * 5}


# ---- builders: algebra ----
def with_counts(s, which):
    """(offsets, values) -> (offsets, values, counts): which = "a" (1 + rank % 7), "b" (1000 (1 + rank % 5)) or None (uncounted)"""
    return s[0], s[1], None if which is None else counts_a(s[0]) if which == "a" else counts_b(s[0])


def saturation_pairs():
    """one value per pair -> (a, b, expected sums): (2^32-1) + 1 and 2^31 + 2^31 saturate, (2^32-2) + 1 is exact; a fourth pair whose values differ"""
    ca = np.array([SAT, 2**31, SAT - 1, SAT], U32)
    cb = np.array([1, 2**31, 1, SAT], U32)
    a = (np.arange(5, dtype=U64), np.array([7, 8, 9, 10], U64), ca)
    b = (np.arange(5, dtype=U64), np.array([7, 8, 9, 11], U64), cb)
    return a, b, [[SAT], [SAT], [SAT], [SAT, SAT]]


def filter_sets(chunk, seed=229):
    """sets for bsk_sets_filter_counts with bounds lo = 3, hi = 9: counts equal to both bounds, sets that lose everything at the first, a
    middle and the last position, an empty set, and one set that spans more than a scan chunk"""
    rng = np.random.default_rng(seed)
    lo, hi = 3, 9
    sizes = [5, 0, 40, 7, chunk + 77, 6, 9]
    sets, cs = [], []
    for i, n in enumerate(sizes):
        sets.append(np.sort(rng.choice(1 << 40, size=n, replace=False).astype(U64)))
        c = rng.integers(1, 13, size=n).astype(U32)
        if i in (0, 3, 6):
            c[:] = np.where(rng.integers(0, 2, size=n) == 0, lo - 1, hi + 1)  # nothing survives
        cs.append(c)
    cs[2][:4] = [lo, hi, lo - 1, hi + 1]
    offs, vals = SO.collection(sets)
    return (offs, vals, np.concatenate(cs).astype(U32)), lo, hi


# ---- end to end ----
def gather_case(seed=233):
    """three random 20 kb genomes, reads of 150 bases at coverage 3, 1 and 0, shuffled and cut into two batches"""
    rng = np.random.default_rng(seed)
    genomes = [bytes(_ACGT[rng.integers(0, 4, 20000)]) for _ in range(3)]
    reads = []
    for g, cov in zip(genomes, (3, 1, 0)):
        for _ in range(cov * len(g) // 150):
            at = int(rng.integers(0, len(g) - 150))
            reads.append(g[at:at + 150])
    reads = [reads[i] for i in rng.permutation(len(reads))]
    half = len(reads) // 2
    return dict(genomes=genomes, batches=[reads[:half], reads[half:]], pk=dict(k=21, w=11), scale=10)
