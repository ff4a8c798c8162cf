"""CPU: the containment search's host-side reference, mixer and crafted cases (tests/search_cases.py) hold what they claim.

ref_search is pinned against a brute-force loop over Python sets, unmix64 against mix64, and every crafted case -- recomputed from
its own sets -- has the posting sums, large queries and bucket occupancy it claims, so the GPU tests that use them reach the branch
they exist for."""
import numpy as np
import pytest

from tests import search_cases as SC

U64 = np.uint64


def test_unmix64_inverts_mix64():
    x = np.concatenate([np.array([0, 1, 2**63, 2**64 - 1], U64), np.random.default_rng(3).integers(0, 2**64, 100_000, dtype=U64)])
    assert np.array_equal(SC.unmix64(SC.mix64(x)), x)
    assert np.array_equal(SC.mix64(SC.unmix64(x)), x)
    assert int(SC.mix64(0)) == 0 and int(SC.mix64(SC.unmix64(2**64 - 1))) == 2**64 - 1
    # splitmix64's published finalizer on 1, step by step in Python integers
    z, m = 1, (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    assert int(SC.mix64(1)) == z ^ (z >> 31)


def _brute(tsets, qsets, ms, qc, tc):
    offs, tgt, sh = [0], [], []
    for q in qsets:
        for j, t in enumerate(tsets):
            s = len(q & t)
            if s >= max(ms, 1) and float(s) >= qc * float(len(q)) and float(s) >= tc * float(len(t)):
                tgt.append(j)
                sh.append(s)
        offs.append(len(tgt))
    return np.array(offs, U64), np.array(tgt, np.uint32), np.array(sh, np.uint32)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ref_search_equals_brute_force(seed):
    rng = np.random.default_rng(seed)
    pool = np.concatenate([np.array([0, 2**64 - 1], U64), rng.integers(0, 2**64, 60, dtype=U64)])
    tsets = [set(pool[rng.integers(0, len(pool), rng.integers(0, 30))].tolist()) for _ in range(25)]
    qsets = [set(pool[rng.integers(0, len(pool), rng.integers(0, 30))].tolist()) for _ in range(40)]
    tg, qs = SC.collection([sorted(s) for s in tsets]), SC.collection([sorted(s) for s in qsets])
    for ms, qc, tc in [(1, 0.0, 0.0), (0, 0.0, 0.0), (3, 0.0, 0.0), (1, 0.1, 0.0), (1, 1 / 3, 0.0), (1, 0.5, 0.0), (1, 1.0, 0.0),
                       (1, 0.0, 0.1), (1, 0.0, 0.3), (1, 0.0, 1.0), (7, 0.0, 0.0), (30, 0.25, 0.25), (2, 0.2, 0.2)]:
        want = _brute(tsets, qsets, ms, qc, tc)
        got = SC.ref_search(*tg, *qs, ms, qc, tc)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), (seed, ms, qc, tc)
    assert np.array_equal(SC.posting_sums(*tg, *qs), [sum(sum(v in t for t in tsets) for v in q) for q in qsets])


def test_ref_top_on_a_hand_made_case():
    """query 0: shared 2 5 5 1 -> the two 5s by ascending target, then the 2; query 1: no hits; query 2: one hit"""
    o, t, s = SC.ref_top(np.array([0, 4, 4, 5], U64), np.array([1, 3, 7, 9, 2], np.uint32), np.array([2, 5, 5, 1, 4], np.uint32), 3)
    assert o.tolist() == [0, 3, 3, 4] and t.tolist() == [3, 7, 1, 2] and s.tolist() == [5, 5, 2, 4] and t.dtype == s.dtype == np.uint32


def test_s2_matrix_equals_ref_search():
    offs, vals = SC.s2_case(n_sets=60, size=500, pool=20_000)
    m = SC.s2_matrix(offs, vals)
    o, t, s = SC.ref_search(offs, vals, offs, vals)
    q = np.repeat(np.arange(60), np.diff(o).astype(np.int64))
    want = np.zeros((60, 60), np.int64)
    want[q, t.astype(np.int64)] = s
    assert np.array_equal(m, want) and np.array_equal(np.diag(m), np.diff(offs).astype(np.int64)) and (m > 0).sum() > 60


def _check_claims(case):
    tg, qs, cl = case
    sums = SC.posting_sums(*tg, *qs)
    assert np.array_equal(sums, cl["sums"])
    assert np.array_equal(cl["large"], sums > SC.SR_CAP) and cl["n_large"] == int((sums > SC.SR_CAP).sum())
    assert len(tg[1]) == int(tg[0][-1]) and len(qs[1]) == int(qs[0][-1])
    for o, v in (tg, qs):
        d = np.diff(v.astype(np.float64))  # (ascending inside every set: the upload rejects anything else)
        inside = np.ones(len(v), bool)
        inside[o[:-1][np.diff(o) > 0].astype(np.int64)] = False
        assert (v[1:][inside[1:]] > v[:-1][inside[1:]]).all() if len(v) > 1 else True, d
    return tg, qs, cl, sums


def test_posting_edge_case_claims():
    tg, qs, cl, sums = _check_claims(SC.posting_edge_case())
    for n in SC.SUM_EDGES:
        assert (sums == n).sum() >= 4, n
    run, best = 0, 0
    for s in sums:
        run = run + 1 if s == SC.SR_CAP else 0
        best = max(best, run)
    assert best >= 32 and (sums == SC.SR_CAP).sum() >= 80
    tsz = np.diff(tg[0]).astype(np.int64)
    assert (tsz[:3] == 0).all() and (tsz[-4:] == 0).all() and (tsz[3:-4] > 0).all()  # leading and trailing runs of empty targets


@pytest.mark.parametrize("n_targets", [1, 2, 3])
def test_clamp_case_claims(n_targets):
    tg, qs, cl, sums = _check_claims(SC.clamp_case(n_targets))
    assert len(tg[0]) - 1 == n_targets and cl["n_large"] >= 2 and ((sums > 10 * n_targets) & ~cl["large"]).sum() >= 2
    assert SC.SR_CAP in sums or n_targets == 3


def test_list_length_case_claims():
    tg, qs, cl, sums = _check_claims(SC.list_length_case())
    assert cl["large"][:-1].all()
    sv = np.sort(tg[1])
    for i, n in enumerate(SC.LIST_LENGTHS):
        for j, at in enumerate(SC.LIST_PLACES):
            q = i * len(SC.LIST_PLACES) + j
            v = qs[1][int(qs[0][q]):int(qs[0][q + 1])]
            cnt = np.searchsorted(sv, v, "right") - np.searchsorted(sv, v, "left")
            assert len(v) == 140 and cnt[at] == n and (np.delete(cnt, at) <= 40).all(), (n, at)


@pytest.mark.parametrize("n_large,last_only", [(n, False) for n in (1, 2, 3, 4, 5, 255, 256, 257)] + [(1, True)])
def test_nl_case_claims(n_large, last_only):
    tg, qs, cl, sums = _check_claims(SC.nl_case(n_large, last_only))
    large = cl["large"]
    assert cl["n_large"] == n_large and large[-1] == (n_large > 1 or last_only) and large[0] != last_only and (~large).sum() > n_large
    if n_large > 2:
        assert large[1] and qs[0][2] - qs[0][1] == 1  # the query that min_shared = 2 rejects: one value, 2 100 targets
        nh = np.diff(SC.ref_search(*tg, *qs, 2)[0])
        assert nh[1] == 0 and (nh[large] > 0).sum() == n_large - 1  # and every other large query keeps hits
    if n_large > 3:
        assert 2 < np.flatnonzero(large)[2] < len(large) - 1


def test_edge_large_case_claims():
    tg, qs, cl, sums = _check_claims(SC.edge_large_case())
    assert cl["large"].all() and cl["n_large"] == 290
    assert sorted(set(np.diff(qs[0]).tolist())) == [10, 30, 60, 90, 100]


def test_boundary_case_claims():
    tg, qs, cl, sums = _check_claims(SC.boundary_case(21000, 21000))
    assert cl["n_large"] == 21000 and len(sums) == 42000
    assert sums.min() >= 2036 and sums.max() <= 2071 and ((sums >= 2040) & (sums <= 2060)).mean() > 0.8
    assert (sums == SC.SR_CAP).any() and (sums == SC.SR_CAP + 1).any() and int(sums.sum()) < 10**8
    assert 0.3 < cl["large"][-5000:].mean() < 0.7  # both paths beyond the first grid pass


@pytest.mark.parametrize("name", SC.LAYOUTS)
def test_directory_layout_claims(name):
    vals, cl = SC.layout(name)
    d = SC.directory(vals)
    assert d["n_distinct"] == cl["n_distinct"] == len(np.unique(vals))
    assert 2 ** d["bits"] <= d["n_distinct"] < 2 ** (d["bits"] + 1) and d["counts"].sum() == d["n_distinct"]
    assert np.array_equal(np.sort(SC.mix64(np.unique(vals))), d["keys"])
    if "keys" in cl:
        assert cl["keys"] <= set(int(k) for k in d["keys"])
        b = SC.bucket(d["keys"], d["bits"])
        assert b[0] == 0 and b[-1] == 2 ** d["bits"] - 1
    if "occupied" in cl:
        assert d["bits"] == cl["bits"] and {j: int(c) for j, c in enumerate(d["counts"]) if c} == cl["occupied"]
        assert d["max_bucket"] == d["counts"][-1] > d["counts"][0]  # the fullest bucket is the last
    if "min_bucket_at" in cl:
        (j, n), = cl["min_bucket_at"].items()
        assert d["bits"] == cl["bits"] and d["counts"][j] >= n >= 500 and d["max_bucket"] == d["counts"][j]
    probes = SC.probe_keys(d)
    present = np.isin(probes, d["keys"])
    assert present.any() and (~present).any() if d["n_distinct"] > 1 else present.any()


def test_probe_keys_reach_the_long_bucket_and_empty_neighbours():
    d = SC.directory(SC.layout("long bucket")[0])
    p = SC.probe_keys(d)
    inb = d["keys"][SC.bucket(d["keys"], 12) == 1234]
    assert {int(inb[0]), int(inb[len(inb) // 2]), int(inb[-1]), int(inb[0]) - 1, int(inb[-1]) + 1} <= set(int(x) for x in p)
    d = SC.directory(SC.layout("first and last bucket")[0])
    b = set(SC.bucket(SC.probe_keys(d), 10).tolist())
    assert {0, 1, 1022, 1023} <= b
