"""CPU: the sketch sets' host-side reference and crafted reads (tests/sets_cases.py) hold what they claim.

ref_sets is pinned against a brute-force loop over Python integers, ref_sets_rows against ref_sets, the restated constants against
sets.hip / sets_internal.hpp, and every builder's claim -- counts, network widths, ranks of duplicates, values that pass a scale,
threshold and sentinel codes -- is re-derived with the oracle alone, so the GPU tests that use them reach the edge they exist for."""
import os
import re

import numpy as np
import pytest

from tests import sets_cases as SC

U64 = np.uint64
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bio_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def test_constants_equal_the_sources():
    sets, scan = _read("sets.hip"), _read("sets_internal.hpp")
    assert SC.SMALL_CAP == int(re.search(r"#define SMALL_CAP (\d+)", sets).group(1))
    assert "max_count <= SMALL_CAP" in sets and "__ballot(c > 32)" in sets and "__ballot(c > 16)" in sets
    per, block = (int(re.search(r"#define %s (\d+)" % n, scan).group(1)) for n in ("SCAN_PER_THREAD", "SCAN_BLOCK"))
    assert "#define SCAN_CHUNK (SCAN_PER_THREAD * SCAN_BLOCK)" in scan and SC.SCAN_CHUNK == per * block
    assert SC.SCAN_TRIP == int(re.search(r"for \(u64 b0 = 0; b0 < nb; b0 \+= (\d+)\)", scan).group(1))
    assert SC.SCAN_TRIP == int(re.search(r"__launch_bounds__\((\d+)\) void k_scan_top", scan).group(1))


def _brute(values_per_read, scale, whole):
    mh = (2**64 - 1) // scale if scale > 1 else 2**64 - 1
    per = [sorted({int(x) for x in v if int(x) <= mh}) for v in values_per_read]
    if whole:
        per = [sorted(set().union(*per))] if per else [[]]
    offs, vals = [0], []
    for s in per:
        vals += s
        offs.append(len(vals))
    return np.array(offs, U64), np.array(vals, U64)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ref_sets_equals_brute_force(seed):
    rng = np.random.default_rng(seed)
    for scale in (0, 1, 2, 3, 7, 2**31 - 1):
        m = SC.maxhash(scale)
        pool = np.concatenate([np.array([0, 1, m - 1, m, min(m + 1, SC.FULL), SC.FULL], U64), rng.integers(0, 2**64, 20, dtype=U64)])
        reads = [pool[rng.integers(0, len(pool), rng.integers(0, 40))] for _ in range(30)] + [np.zeros(0, U64)]
        for whole in (False, True):
            got, want = SC.ref_sets(reads, scale, whole), _brute(reads, scale, whole)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (seed, scale, whole)
    assert SC.maxhash(0) == SC.maxhash(1) == 2**64 - 1 and SC.maxhash(3) == 0x5555555555555555
    o, v = SC.ref_sets([], 1, True)
    assert list(o) == [0, 0] and len(v) == 0


@pytest.mark.parametrize("seed", [1, 2])
def test_ref_sets_rows_equals_ref_sets(seed):
    rng = np.random.default_rng(seed)
    pool = np.concatenate([np.array([0, SC.FULL // 3, SC.FULL // 3 + 1, SC.FULL], U64), rng.integers(0, 2**64, 12, dtype=U64)])
    v2d = pool[rng.integers(0, len(pool), (200, 7))]
    present = rng.random(200) < 0.9
    reads = [v if p else np.zeros(0, U64) for v, p in zip(v2d, present)]
    for scale in (1, 2, 3):
        for whole in (False, True):
            got, want = SC.ref_sets_rows(v2d, scale, whole, present), SC.ref_sets(reads, scale, whole)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (scale, whole)
    got, want = SC.ref_sets_rows(v2d, 3, False), SC.ref_sets(list(v2d), 3, False)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_ladder_waves_hold_every_count_at_every_row():
    waves = np.array(SC.ladder_waves())
    for c in SC.LADDER:
        for p in range(4):
            assert (waves[:, p] == c).any(), (c, p)
    for width, lo, hi in ((32, 17, 32), (64, 33, 64)):  # one long row, three rows the 16-value network would do for
        for p in range(4):
            assert any(lo <= w[p] <= hi and sum(x > 16 for x in w) == 1 for w in waves), (width, p)
    assert any(sorted(w) == [0, 0, 0, 33] for w in waves.tolist())
    assert set(SC.wave_widths(waves.ravel())) == {16, 32, 64} and waves.max() == SC.SMALL_CAP
    assert list(SC.wave_widths([16, 0, 0, 0, 17, 0, 0, 0, 32, 1, 1, 1, 0, 0, 0, 33, 64])) == [16, 32, 32, 64, 64]


@pytest.mark.parametrize("k", [21, 4])
@pytest.mark.parametrize("tail", [0, 1, 2, 3])
@pytest.mark.parametrize("extra65", [False, True])
def test_ladder_case_claims(oracle, k, tail, extra65):
    case = SC.ladder_case(oracle, k, tail, extra65)
    vals = SC.values_of(oracle, case)
    counts = np.array([len(v) for v in vals])
    assert np.array_equal(counts, case["counts"]) and len(counts) % 4 == (tail + extra65) % 4
    assert counts.max() == (65 if extra65 else 64) and (counts == 65).sum() == int(extra65)
    assert np.array_equal(case["widths"], SC.wave_widths(counts))
    if not extra65:
        assert np.array_equal(counts[:4 * len(SC.ladder_waves())].reshape(-1, 4), SC.ladder_waves())
        assert tail == 0 or counts[-tail:].max() > 16  # a loaded last wave
    distinct = np.array([len(np.unique(v)) for v in vals])
    assert np.array_equal(distinct, case["distinct"])
    if k == 21:
        assert np.array_equal(distinct, counts)  # no duplicates: the sets are the sorted reads
    else:
        assert (distinct < counts)[counts >= 31].mean() > 0.9 and (distinct < counts)[counts >= 63].all()  # full of them


def test_dup_boundary_case_claims(oracle):
    case = SC.dup_boundary_case(oracle)
    vals = SC.values_of(oracle, case)
    seen = set()
    for v, f in zip(vals, case["facts"]):
        v = np.sort(v)
        assert len(v) == f["count"] <= SC.SMALL_CAP
        if f["how"] == "at":
            assert f["count"] > f["b"] and v[f["b"] - 1] == v[f["b"]], f
        elif f["how"] == "after":
            assert v[f["b"] - 1] != v[f["b"]] == v[f["b"] + 1], f
        else:
            assert len(np.unique(v)) == f["distinct"], f
        seen.add((f["how"], f.get("b", f["count"])))
    assert seen == {(h, b) for h in ("at", "after") for b in (16, 32, 48)} | {(h, c) for h in ("poly", "period2") for c in (17, 33, 49, 64)}


def test_filter_case_claims(oracle):
    cases = SC.filter_case(oracle)
    assert [(e["c"], e["b"]) for e in cases] == SC.FILTER_PAIRS
    assert {b for _, b in SC.FILTER_PAIRS} == {0, 1, 15, 16, 17, 32, 48, 64} and (48, 48) in SC.FILTER_PAIRS and (64, 64) in SC.FILTER_PAIRS
    for e in cases:
        v = np.sort(SC.oracle_values(oracle, "nthash", dict(k=SC.FILTER_K), e["read"]))
        assert len(v) == e["c"] and 2 <= e["scale"] <= 64
        assert int((v <= U64(SC.maxhash(e["scale"]))).sum()) == e["b"], e
        assert e["straddle"] == bool(SC.straddles(v, e["b"]))
        if e["straddle"]:
            m = U64(SC.maxhash(e["scale"]))
            assert v[e["b"] - 2] == v[e["b"] - 1] <= m < v[e["b"]] == v[e["b"] + 1]
    assert sum(e["straddle"] for e in cases) >= 1


def test_threshold_case_claims(oracle):
    cases = SC.threshold_case(oracle)
    assert len(cases) == 3 and {3, 2**31 - 1} <= {e["scale"] for e in cases}
    for e in cases:
        m = e["m"]
        assert m == (2**64 - 1) // e["scale"]
        for q, x in zip(e["short"], (m - 1, m, m + 1)):
            assert len(q) == 32 and [int(c) for c in oracle.kmer_codes(q, 32, True, False)] == [x]
        lv = oracle.kmer_codes(e["long"], 32, True, False)
        assert len(e["long"]) == 96 and len(lv) == 65 > SC.SMALL_CAP and {m - 1, m, m + 1} <= {int(c) for c in lv}
        o, v = SC.ref_sets([lv], e["scale"], False)
        assert m - 1 in v and m in v and m + 1 not in v


def test_sentinel_case_claims(oracle):
    case = SC.sentinel_case()
    vals = SC.values_of(oracle, case)
    assert max(len(v) for v in vals) <= SC.SMALL_CAP
    for v, full in zip(vals, case["holds_full"]):
        assert bool((v == U64(SC.FULL)).any()) == full and (not full or (v == 0).any())
    assert [int(x) for x in vals[0]] == [SC.FULL, 0] and (vals[1] == U64(SC.FULL)).sum() == 9 and len(vals[3]) > 32
    for scale in (0, 1):
        o, v = SC.ref_sets(vals, scale, False)
        assert [int(x) for x in v[:2]] == [0, SC.FULL] and (v == U64(SC.FULL)).sum() == sum(case["holds_full"])
    o, v = SC.ref_sets(vals, 2, False)
    assert not (v == U64(SC.FULL)).any() and (v == 0).sum() == sum(case["holds_full"])


@pytest.mark.parametrize("name", list(SC.LAYOUTS))
def test_layout_case_claims(oracle, name):
    case = SC.layout_case(oracle, name)
    lens, _, _ = SC.LAYOUTS[name]
    counts = np.array([len(v) for v in SC.values_of(oracle, case)])
    n = len(counts)
    assert n % 64 == 29 and counts.max() <= SC.SMALL_CAP and counts.max() > 16
    assert (counts == 0).sum() >= 4 and counts[64] == counts[65] == counts[127] == 0
    k, w = case["pk"]["k"], case["pk"]["w"]
    for i in case["tailed"]:
        assert case["reads"][i].endswith("A" * (k + w + 4)) and counts[i] > 0  # windows of one repeated k-mer: a key tie
    full = [len(q) for i, q in enumerate(case["reads"]) if counts[i] and not (name == "pk" and i in (199, 263))]
    assert min(full) >= min(lens) and max(full) == max(lens)  # one length class; the longest read decides the plan
    if name == "pk":
        assert counts[199] == 50 and len(np.unique(SC.values_of(oracle, dict(case, reads=case["reads"][199:200]))[0])) == 1


def test_scan_cases_cross_the_trips(oracle):
    trip = SC.SCAN_TRIP * SC.SCAN_CHUNK
    a = SC.scan_reads_case(oracle, n=3 * SC.SCAN_CHUNK + 5)  # (the builder at a small n: the same code, three blocks)
    assert a["step"] == 4 and not a["present"][[0, 1, SC.SCAN_CHUNK - 1, SC.SCAN_CHUNK]].any() and a["present"].sum() == a["n"] - 4
    for i in range(0, a["n"], 97):
        want = oracle.nthash(SC.scan_read(a, i), 21, True)[0] if a["present"][i] else []
        assert np.array_equal(want, a["v2d"][i] if a["present"][i] else []), i
    reads = [v if p else np.zeros(0, U64) for v, p in zip(a["v2d"], a["present"])]
    for scale in (1, 3):
        got, want = SC.ref_sets_rows(a["v2d"], scale, False, a["present"]), SC.ref_sets(reads, scale, False)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    n = 2 * trip + SC.SCAN_CHUNK + 1  # the default: three trips of the counts scan
    assert (n + SC.SCAN_CHUNK - 1) // SC.SCAN_CHUNK == 2 * SC.SCAN_TRIP + 2
    b = SC.scan_values_case()
    assert b["count"] == 130 > SC.SMALL_CAP and b["n"] * b["count"] > trip  # the KeepOf scan's second trip
    v = SC.scan_values_v2d(oracle, dict(b, n=50))
    assert v.shape == (50, 130)
