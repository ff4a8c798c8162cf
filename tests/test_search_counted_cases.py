"""CPU: tests/search_counted_cases.py checked against itself -- the caps it restates are those of search.hip, the dict-walk model agrees
with a pair-by-pair brute force on random and crafted collections, every wrong model named in BUGS is told from the right one, and each
crafted case has the posting sums, rows and paths it claims.  Nothing here runs the library, so this module passes without the feature's
device code; tests/test_gpu_search_counted.py holds the device to the model."""
import numpy as np
import pytest

from tests import search_cases as SC
from tests import search_counted_cases as W


def _random_case(seed, nt=9, nq=7, pool=40):
    rng = np.random.default_rng(seed)
    tg = SC.collection([rng.choice(pool, int(rng.integers(0, 14)), replace=False) for _ in range(nt)])
    qs = SC.collection([rng.choice(pool, int(rng.integers(0, 14)), replace=False) for _ in range(nq)])
    return tg, qs


def _same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b)) and len(a) == len(b) == 5


def test_the_caps_are_those_of_the_source():
    caps = W.read_caps()
    assert caps["SW_ROW"] == W.SW_ROW and caps["SW_CHUNK"] == W.SW_CHUNK and caps["SR_CAP"] == W.SR_CAP == SC.SR_CAP
    assert W.SW_ROW <= W.SR_CAP and W.SW_ROW % 32 == 0  # a small-path row has at most SR_CAP hits; a word of saturation bits per 32 hits


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("counted", [(True, True), (True, False), (False, True), (False, False)])
def test_model_against_brute_force(seed, counted):
    tg, qs = _random_case(seed)
    kind = "mixed" if seed % 2 else "small"
    tc, qc = W.with_counts(tg, qs, 100 + seed, kind)
    tc, qc = (tc if counted[0] else None), (qc if counted[1] else None)
    for thr in ((1, 0.0, 0.0), (2, 0.0, 0.0), (1, 0.3, 0.0), (1, 0.0, 0.4), (3, 0.2, 0.2)):
        got, want = W.ref_search_counted(tg, tc, qs, qc, *thr), W.brute(tg, tc, qs, qc, *thr)
        assert _same(got, want), thr
        assert all(np.array_equal(x, y) for x, y in zip(got[:3], SC.ref_search(*tg, *qs, *thr)))  # the rows are the unweighted search's
        if tc is None and qc is None:
            assert np.array_equal(got[3], got[2].astype(np.uint64)) and np.array_equal(got[4], got[2].astype(np.uint64))  # dot == min_sum == shared


@pytest.mark.parametrize("bug", W.BUGS)
def test_wrong_models_are_caught(bug):
    """each wrong model differs from the right one on a case made for it (and on the saturation case where that is the point)"""
    if bug == "wrap":
        tg, tc, qs, qc, _, _ = W.saturation_case(False)
        thr = (1, 0.0, 0.0)
    elif bug == "uncounted is 0":
        tg, qs = _random_case(3)
        tc, qc = W.with_counts(tg, qs, 5, "small")[0], None
        thr = (1, 0.0, 0.0)
    else:
        tg, qs = _random_case(4)
        tc, qc = W.with_counts(tg, qs, 6, "small")
        thr = (2, 0.0, 0.0) if bug == "unlisted pairs" else (1, 0.0, 0.0)  # a threshold that drops pairs, so that there are unlisted ones
    right, wrong = W.brute(tg, tc, qs, qc, *thr), W.brute(tg, tc, qs, qc, *thr, bug=bug)
    model = W.ref_search_counted(tg, tc, qs, qc, *thr)
    assert _same(model, right) and not _same(model, wrong)
    assert all(np.array_equal(x, y) for x, y in zip(right[:3], wrong[:3]))  # the rows agree: only the weights tell them apart
    if bug == "unlisted pairs":
        assert len(W.brute(tg, tc, qs, qc, 1, 0.0, 0.0)[1]) > len(right[1]) > 0  # min_shared = 2 did drop pairs, and kept some


def test_saturation_case_has_its_numbers():
    for large in (False, True):
        tg, tc, qs, qc, cl, want = W.saturation_case(large)
        assert np.array_equal(SC.posting_sums(*tg, *qs), cl["sums"]) and bool(cl["large"][0]) == large
        o, t, s, d, m = W.ref_search_counted(tg, tc, qs, qc)
        assert t[:5].tolist() == [0, 1, 2, 3, 4] and s[:5].tolist() == [2, 2, 3, 2, 4] and len(t) == (2105 if large else 5)
        assert [int(x) for x in d[:5]] == want["dot"] and [int(x) for x in m[:5]] == want["min_sum"]
        M = W.M32
        assert M * M + 2 * M == W.MAX and want["dot"][1] < W.MAX and 2 * M > 1 << 32  # exactly 2^64 - 1 without a wrap; one below it; a min_sum above 2^32
        assert M * M + 2 * M + 1 == 1 << 64 and 2 * M * M > 1 << 64 and 2 * M * M + 3 * M >= 2 << 64 - 1  # beyond: by one, and by a whole wrap
        if large:
            assert d[5:].tolist() == [3] * 2100 and m[5:].tolist() == [1] * 2100
        in_row, chunks = W.paths(cl["sums"], qs[0], o)
        assert (in_row.tolist(), chunks.tolist()) == (([False], [1]) if large else ([True], [0]))


def test_row_edge_case_straddles_the_lds_row():
    tg, qs, cl, extra = W.row_edge_case()
    assert np.array_equal(SC.posting_sums(*tg, *qs), cl["sums"]) and cl["n_large"] == 0  # every query on the search's small path
    o, t, s = SC.ref_search(*tg, *qs)
    assert np.diff(o).tolist() == extra["hits"] == [W.SW_ROW - 1, W.SW_ROW, W.SW_ROW + 1, 200] and set(s.tolist()) == {1, 2, 3}
    in_row, chunks = W.paths(cl["sums"], qs[0], o)
    assert in_row.tolist() == [True, True, False, True] and chunks.tolist() == [0, 0, -(-(W.SW_ROW + 3) // W.SW_CHUNK), 0]
    assert max(len(v[0]) for v in W.postings(*tg).values()) == 200  # a posting list beyond 64 on the small path
    # thresholds change the rows, and with them the path: with min_shared = 2 the third query's row fits
    o2 = SC.ref_search(*tg, *qs, 2)[0]
    assert W.paths(cl["sums"], qs[0], o2)[0].tolist() == [True, True, True, False] and np.diff(o2)[3] == 0


def test_chunk_edge_case_straddles_the_chunk():
    tg, qs, cl, extra = W.chunk_edge_case()
    assert np.array_equal(SC.posting_sums(*tg, *qs), cl["sums"])
    n = np.diff(qs[0]).astype(int)
    assert n[0::2].tolist() == list(W.CHUNK_EDGES) and cl["large"][0::2].all() and not cl["large"][1::2].any()
    o = SC.ref_search(*tg, *qs)[0]
    in_row, chunks = W.paths(cl["sums"], qs[0], o)
    assert chunks[0::2].tolist() == [1, 1, 2, 2, 3] and not in_row[0::2].any() and not chunks[1::2].any()
    assert W.plan_tail(cl["sums"], qs[0], o) == "; weights: k_sw_row %d queries (<= 512 hits), k_sw_chunk 9 chunks of 256 values" % int(in_row.sum())


def test_seeded_counts_reach_both_ends():
    c = W.seeded_counts(4000, 1, "mixed")
    assert c.dtype == np.uint32 and c.min() == 1 and c.max() == W.M32 and 200 < (c == W.M32).sum() < 600
    assert W.seeded_counts(10, 1, "small").max() <= 9 and (W.seeded_counts(10, 1, "max") == W.M32).all()
    assert np.array_equal(W.seeded_counts(50, 7), W.seeded_counts(50, 7))  # seeded
