"""CPU: the NumPy model of the window sets and the folded hits (tests/window_cases.py) against a second formulation -- per tuple and per
window by the definition, a dict per row for the fold -- and proof that the cases tell the contract from its likely misreadings."""
import numpy as np
import pytest

from tests import window_cases as WC

U64, U32 = np.uint64, np.uint32


def _tuples(rng, lengths, implicit=False, dup=False):
    """random tuples of sequences with these tuple counts: ascending positions with a random strand bit (or implicit), 64-bit hashes"""
    offs, hs, ps = [0], [], []
    for c in lengths:
        p = np.sort(rng.choice(max(3 * c, 1), size=c, replace=False)).astype(U32) if c else np.zeros(0, U32)
        ps.append(p | (rng.integers(0, 2, c).astype(U32) << U32(31)))
        h = rng.integers(0, 2**64, c, dtype=U64)
        if dup and c > 3:
            h[rng.integers(0, c, c // 2)] = h[0]  # repeated values: counts above 1
        hs.append(h)
        offs.append(offs[-1] + c)
    return np.array(offs, U64), np.concatenate(hs), (None if implicit else np.concatenate(ps))


def _window_cases():
    rng = np.random.default_rng(20261020)
    cases = []
    for implicit in (False, True):
        t = _tuples(rng, [0, 1, 2, 9, 40, 0, 17], implicit, dup=True)
        for kw in (dict(window=1), dict(window=7), dict(window=7, step=1), dict(window=7, step=3), dict(window=7, step=6), dict(window=64), dict(window=2**31 - 1),
                   dict(count=1), dict(count=3), dict(count=10), dict(count=100000), dict(window=5, scale=3), dict(count=4, scale=2)):
            cases.append((t, kw))
    # crafted edges: the last position exactly at W, at W - 1 and at W + 1; a sequence whose only tuple sits at position 0; the strand bit on the last tuple
    for last in (6, 7, 8, 14):
        pos = np.array([0, 3, last], U32) | np.array([0, 0, 0x80000000], U32)
        t = (np.array([0, 3, 4], U64), np.array([5, 5, 9, 1], U64), np.concatenate([pos, np.array([0], U32)]))
        cases += [(t, dict(window=7)), (t, dict(window=7, step=3)), (t, dict(count=2)), (t, dict(count=3))]
    return cases


def _fold_cases():
    rng = np.random.default_rng(7)
    cases = []
    go = np.array([0, 0, 3, 3, 10, 11, 20, 20], U64)  # empty groups at the start, in the middle and at the end
    for nq in (0, 1, 30):
        offs, tg = [0], []
        for _ in range(nq):
            t = np.sort(rng.choice(20, size=rng.integers(0, 12), replace=False))
            tg.append(t)
            offs.append(offs[-1] + len(t))
        tg = np.concatenate(tg).astype(U32) if tg else np.zeros(0, U32)
        sh = rng.integers(1, 1000, len(tg)).astype(U32)
        for kw in (dict(), dict(min_members=0), dict(min_members=2), dict(frac=(1, 1)), dict(frac=(8, 10)), dict(frac=(1, 3)), dict(min_members=2, frac=(1, 3))):
            cases.append(((np.array(offs, U64), tg, sh, go), kw))
    # saturation: 0xFFFFFFFF + 1; the fraction met exactly: 8 of 10 and 1 of 3
    cases.append(((np.array([0, 2], U64), np.array([0, 1], U32), np.array([0xFFFFFFFF, 1], U32), np.array([0, 2], U64)), dict()))
    exact = (np.array([0, 9], U64), np.array([0, 1, 2, 3, 4, 5, 6, 7, 10], U32), np.ones(9, U32), np.array([0, 10, 13], U64))
    cases += [(exact, dict(frac=(8, 10))), (exact, dict(frac=(1, 3))), (exact, dict(frac=(9, 10))), (exact, dict(frac=(2, 3)))]
    return cases


@pytest.mark.parametrize("i", range(len(_window_cases())))
def test_windows_model_equals_the_definition(i):
    (offs, h, p), kw = _window_cases()[i]
    got, want = WC.windows_model(offs, h, p, **kw), WC.windows_brute(offs, h, p, **kw)
    assert WC.same(got, want), kw
    seq_off, set_off, vals, cnts = got
    assert seq_off[-1] == len(set_off) - 1 and set_off[-1] == len(vals) == len(cnts)
    if kw.get("count"):
        assert (np.diff(seq_off.astype(np.int64)) <= kw["count"]).all()  # count mode: at most `count` windows
    # the union of a sequence's windows is the sequence's own set, for any step
    so, sv = WC.sets_per_sequence(offs, h, kw.get("scale", 1))
    for s in range(len(offs) - 1):
        a, b = int(set_off[seq_off[s]]), int(set_off[seq_off[s + 1]])
        assert np.array_equal(np.unique(vals[a:b]), sv[int(so[s]):int(so[s + 1])])


@pytest.mark.parametrize("i", range(len(_fold_cases())))
def test_fold_model_equals_a_dict_per_row(i):
    args, kw = _fold_cases()[i]
    assert WC.same(WC.fold_model(*args, **kw), WC.fold_brute(*args, **kw)), kw


@pytest.mark.parametrize("wrong", WC.WINDOW_MISREADINGS)
def test_the_window_cases_catch_the_misreading(wrong):
    caught = [kw for (t, kw) in _window_cases() if not WC.same(WC.windows_model(*t, **kw), WC.windows_brute(*t, wrong=wrong, **kw))]
    assert caught, wrong


@pytest.mark.parametrize("wrong", WC.FOLD_MISREADINGS)
def test_the_fold_cases_catch_the_misreading(wrong):
    cases = _fold_cases()
    if wrong == "hits_not_targets":
        # a target listed twice in a row is outside what the entry accepts (it refuses such rows); the model still counts it once
        cases = cases + [((np.array([0, 3], U64), np.array([1, 1, 2], U32), np.array([4, 5, 6], U32), np.array([0, 3], U64)), dict())]
    caught = [kw for (a, kw) in cases if not WC.same(WC.fold_model(*a, **kw), WC.fold_brute(*a, wrong=wrong, **kw))]
    assert caught, wrong


def test_top1_model():
    o, t, s = WC.top1_model(np.array([0, 3, 3, 5]), np.array([2, 5, 9, 1, 4], U32), np.array([7, 9, 9, 3, 3], U32))
    assert list(o) == [0, 1, 1, 2] and list(t) == [5, 1] and list(s) == [9, 3]
