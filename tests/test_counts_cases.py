"""CPU: every claim a builder of tests/counts_cases.py makes, re-derived -- the chunk size read from counts.hip, where the crafted runs lie
against the chunk borders, what neighbouring reads share, the references against a plain Python count, the saturation sums."""
import collections
import os
import re

import numpy as np
import pytest

from tests import counts_cases as CC
from tests import sets_cases as SC
from tests import setops_cases as SO

U64, U32 = np.uint64, np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_is_read_from_the_source():
    src = open(os.path.join(ROOT, "bio_amd", "csrc", "counts.hip")).read()
    per, block = (int(re.search(r"^#define %s (\d+)" % n, src, re.M).group(1)) for n in ("CNT_PER_THREAD", "CNT_BLOCK"))
    assert CC.read_chunk() == per * block and re.search(r"__launch_bounds__\(CNT_BLOCK\) void k_cnt_runs", src)
    for k in ("k_cnt_first", "k_cnt_suffix", "k_cnt_runs", "k_fc_flags", "k_fc_scatter", "k_ct_totals"):
        assert re.search(r"__global__[^;{]*\b%s\(" % k, src), k


def plain_count(values_per_read, scale, whole):
    mh = SC.maxhash(scale)
    per = [[int(x) for x in v if int(x) <= mh] for v in values_per_read]
    if whole:
        per = [[x for v in per for x in v]]
    offs, vals, cnt = [0], [], []
    for v in per:
        c = collections.Counter(v)
        for x in sorted(c):
            vals.append(x)
            cnt.append(c[x])
        offs.append(len(vals))
    return np.array(offs, U64), np.array(vals, U64), np.array(cnt, U32)


@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("scale", [0, 1, 3])
def test_references_against_a_plain_count(scale, whole):
    rng = np.random.default_rng(3)
    reads = [rng.integers(0, 40, size=int(rng.integers(0, 60)), dtype=U64) * U64((2**64 - 1) // 40) for _ in range(30)] + [np.zeros(0, U64)]
    reads.append(np.array([2**64 - 1] * 3 + [0] * 2, U64))
    want = plain_count(reads, scale, whole)
    for g, w in zip(CC.ref_counted(reads, scale, whole), want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    v2d = rng.integers(0, 12, size=(50, 9), dtype=U64) * U64((2**64 - 1) // 12)
    for g, w in zip(CC.ref_counted_rows(v2d, scale, whole), plain_count(list(v2d), scale, whole)):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def test_run_layout_reaches_the_borders():
    chunk = CC.read_chunk()
    lengths, facts = CC.run_layout(chunk)
    start = np.concatenate([[0], np.cumsum(lengths)])
    assert sorted({L for L, _, _ in facts}) == sorted(CC.RUN_LENGTHS) and len(facts) == 2 * len(CC.RUN_LENGTHS)
    for L, how, at in facts:
        j = int(np.searchsorted(start, at))
        assert start[j] == at and lengths[j] == L
        if how == "ends":
            assert (at + L) % chunk == 0
        elif L > 1:
            assert at // chunk < (at + L - 1) // chunk and at % chunk != 0  # starts in one chunk, ends in a later one
        else:
            assert at % chunk == 0
    assert any(L > chunk and (at + L - 1) // chunk - at // chunk >= 2 for L, how, at in facts)  # a run over a whole chunk in the middle


def test_runs_case_holds_the_layout(oracle):
    chunk = CC.read_chunk()
    case = CC.runs_case(oracle, chunk)
    vals = SC.values_of(oracle, dict(case, reads=case["reads"][:50] + case["reads"][-50:]))
    assert [int(v[0]) for v in vals] == [int(x) for x in np.concatenate([case["values"][:50], case["values"][-50:]])] and all(len(v) == 1 for v in vals)
    u, c = np.unique(case["values"], return_counts=True)
    assert np.array_equal(c, case["lengths"]) and len(case["reads"]) == int(case["lengths"].sum())


def test_neighbours_case(oracle):
    case = CC.neighbours_case(oracle)
    vals = SC.values_of(oracle, case)
    f = case["facts"]
    for copies in (2, 3, 130):
        i = f["copies%d" % copies]
        assert len(set(case["reads"][i:i + copies])) == 1 and case["reads"][i + copies] != case["reads"][i]
    i = f["max_then_single"]
    assert len(vals[i + 1]) == 1 and vals[i + 1][0] == vals[i].max()
    i = f["single_then_min"]
    assert len(vals[i]) == 1 and vals[i][0] == vals[i + 1].min()


def test_attached_counts_name_both_ranks():
    offs = np.array([0, 3, 3, 40], U64)
    r = CC.ranks(offs)
    assert list(r[:4]) == [0, 1, 2, 0] and r[-1] == 36
    ca, cb = CC.counts_a(offs), CC.counts_b(offs)
    assert ca.min() == 1 and ca.max() == 7 and cb.min() == 1000 and cb.max() == 5000 and ca.dtype == cb.dtype == U32
    sums = {int(x) + int(y) for x in range(1, 8) for y in range(1000, 5001, 1000)}
    assert len(sums) == 35  # a sum determines (ca, cb)


def test_ref_op_on_a_hand_made_pair():
    a = (np.array([0, 3], U64), np.array([1, 5, 9], U64), np.array([2, 3, 4], U32))
    b = (np.array([0, 2], U64), np.array([5, 7], U64), np.array([10, 20], U32))
    assert [list(map(int, x)) for x in CC.ref_op(a, b, CC.ADD)] == [[0, 4], [1, 5, 7, 9], [2, 13, 20, 4]]
    assert [list(map(int, x)) for x in CC.ref_op(a, b, CC.KEEP)] == [[0, 1], [5], [3]]
    assert [list(map(int, x)) for x in CC.ref_op(a, b, CC.DROP)] == [[0, 2], [1, 9], [2, 4]]
    assert [list(map(int, x)) for x in CC.ref_op(a, (b[0], b[1], None), CC.ADD)] == [[0, 4], [1, 5, 7, 9], [2, 4, 1, 4]]
    two = (np.array([0, 2, 3], U64), np.array([5, 7, 1], U64), None)
    assert [list(map(int, x)) for x in CC.ref_op(a, two, CC.KEEP)] == [[0, 1, 2], [5, 1], [3, 2]]  # a broadcast
    assert list(CC.path_counts(a[0], two[0], dict(SO_GROUP_CAP=4, SO_WAVE_CAP=5))) == [1, 1, 0]
    assert [int(x) for x in CC.ref_totals(a)] == [9] and [int(x) for x in CC.ref_totals(two)] == [2, 1]
    assert [list(map(int, x)) for x in CC.ref_filter(a, 3, 3)] == [[0, 1], [5], [3]]


def test_saturation_pairs():
    a, b, sums = CC.saturation_pairs()
    assert sums == [[2**32 - 1]] * 3 + [[2**32 - 1, 2**32 - 1]]
    exact = [int(x) + int(y) for x, y in zip(a[2], b[2])]
    assert exact[0] == 2**32 and exact[1] == 2**32 and exact[2] == 2**32 - 1


def test_filter_sets():
    s, lo, hi = CC.filter_sets(SC.SCAN_CHUNK)
    sizes = np.diff(s[0].astype(np.int64))
    assert sizes[1] == 0 and sizes[4] > SC.SCAN_CHUNK and s[2].min() >= 1
    for v in SO.split(s[0], s[1]):
        assert np.all(np.diff(v.astype(np.int64)) > 0)


def test_gather_case():
    g = CC.gather_case()
    n = [len(b) for b in g["batches"]]
    assert sum(n) == 3 * 20000 // 150 + 20000 // 150 and abs(n[0] - n[1]) <= 1 and all(len(r) == 150 for b in g["batches"] for r in b)
    assert sum(r in g["genomes"][2] for b in g["batches"] for r in b) == 0 and sum(r in g["genomes"][0] for r in g["batches"][0]) > 100
