"""CPU: the model of tests/select_cases.py against a brute force in fractions.Fraction, and the misreadings of the contract it must tell
from the contract: each of them changes the outcome of at least one crafted case."""
import functools
from fractions import Fraction

import numpy as np
import pytest

from tests import select_cases as SC

U64, U32 = np.uint64, np.uint32
TOP64 = SC.TOP64


def random_record(rng, nq=12, n_targets=40):
    o, t = [0], []
    for _ in range(nq):
        t.append(np.sort(rng.choice(n_targets, size=int(rng.integers(0, 14)), replace=False)))
        o.append(o[-1] + len(t[-1]))
    t = np.concatenate(t).astype(U32)
    s = rng.integers(1, 5, len(t)).astype(U32)
    ms = s.astype(U64) * rng.integers(1, 4, len(t)).astype(U64)
    rec = SC.record(o, t, s, s * rng.integers(1, 4, len(t)).astype(U32), ms * rng.integers(1, 5, len(t)).astype(U64), ms, rng.integers(1, 4, len(t)))
    return rec, rng.integers(40, 60, nq).astype(U64), rng.integers(40, 60, n_targets).astype(U64)


def brute_value(measure, rec, q, i, qn, tn):
    """the measure as a Fraction, written from the formulas and not from the table"""
    s, Q, T = int(rec["s"][i]), int(qn[q]), int(tn[int(rec["t"][i])])
    dot, ms = int(rec["dot"][i]), int(rec["msum"][i])
    return {"shared": Fraction(s), "members": Fraction(int(rec["members"][i])), "dot": Fraction(dot), "min_sum": Fraction(ms), "query_cov": Fraction(s, Q),
            "target_cov": Fraction(s, T), "jaccard": Fraction(s, int(rec["total"][i])), "cosine": Fraction(dot * dot, Q * T), "weighted_jaccard": Fraction(ms, Q + T - ms),
            "bray_curtis_similarity": 1 - Fraction(Q + T - 2 * ms, Q + T), "weighted_containment": Fraction(dot, Q)}[measure]


@pytest.mark.parametrize("measure", SC.MEASURES)
def test_the_model_is_the_brute_force(measure):
    rng = np.random.default_rng(len(measure))
    for _ in range(6):
        rec, qn, tn = random_record(rng)
        o = rec["o"]
        val = [brute_value(measure, rec, q, i, qn, tn) for q in range(len(o) - 1) for i in range(int(o[q]), int(o[q + 1]))]
        assert [Fraction(N, D) for N, D in SC.all_nd(measure, rec, qn, tn)] == val
        for bound in (Fraction(0), Fraction(1, 3), Fraction(1, 2), Fraction(7, 10), Fraction(1), Fraction(5, 2), val[len(val) // 2] if val else Fraction(1)):
            if measure == "cosine":  # the bound is on the cosine: val is its square
                keep = [i for i, v in enumerate(val) if v >= bound * bound]
            else:
                keep = [i for i, v in enumerate(val) if v >= bound]
            got = SC.filter_model(rec, measure, bound.numerator, bound.denominator, qn, tn)
            assert np.array_equal(got["t"], rec["t"][keep]) and all(np.array_equal(got[p], rec[p][keep]) for p in SC.PAYLOADS)
            assert np.array_equal(got["o"], [sum(1 for i in keep if i < int(x)) for x in o])
        for n in (1, 3, 20):
            idx = []
            for q in range(len(o) - 1):
                row = sorted(range(int(o[q]), int(o[q + 1])), key=lambda i: (-val[i], int(rec["t"][i])))
                idx += row[:n]
            got = SC.top_by_model(rec, measure, n, qn, tn)
            assert np.array_equal(got["t"], rec["t"][idx]) and all(np.array_equal(got[p], rec[p][idx]) for p in SC.PAYLOADS + ("s",))
            assert list(np.diff(got["o"])) == [min(n, int(c)) for c in np.diff(o)]


def test_jaccard_without_totals_and_the_refusals():
    rec = SC.record([0, 2], [0, 1], [3, 4])
    assert SC.all_nd("jaccard", rec, [10], [5, 6]) == [(3, 12), (4, 12)]
    with pytest.raises(SC.BadHits):
        SC.all_nd("jaccard", rec, [1], [1, 1])  # Q + T - shared < 0
    with pytest.raises(SC.BadHits):
        SC.all_nd("target_cov", rec, [1], [1])  # target 1 >= n_tnorm
    with pytest.raises(SC.BadHits):
        SC.all_nd("query_cov", rec, [0], [1, 1])  # D == 0
    num, den = SC.step_above(1, 2)
    assert Fraction(num, den) - Fraction(1, 2) == Fraction(1, den) and den > 1 << 62  # one step of the largest denominator that fits
    assert SC.step_above(TOP64 - 1, 3) == (TOP64, 3)


# ---- the misreadings: a variant of the model with one rule bent, and the crafted cases that tell it apart ----
def variant(nd=SC.nd, kept=SC.kept, before=SC.before, carry=lambda rec, idx: {p: (None if rec[p] is None else rec[p][idx]) for p in SC.PAYLOADS}):
    def run(rec, measure, op, arg, qn=None, tn=None):
        o = rec["o"]
        fr = [nd(measure, rec, q, i, qn, tn) for q in range(len(o) - 1) for i in range(int(o[q]), int(o[q + 1]))]
        idx, offs = [], [0]
        for q in range(len(o) - 1):
            row = list(range(int(o[q]), int(o[q + 1])))
            if op == "filter":
                idx += [i for i in row if kept(measure, fr[i][0], fr[i][1], *arg)]
            else:
                key = functools.cmp_to_key(lambda i, j: -1 if before((fr[i][0], fr[i][1], int(rec["t"][i]), int(rec["s"][i])), (fr[j][0], fr[j][1], int(rec["t"][j]), int(rec["s"][j]))) else 1)
                idx += sorted(row, key=key)[:arg]
            offs.append(len(idx))
        idx = np.asarray(idx, np.int64)
        return dict(o=np.asarray(offs, U64), t=rec["t"][idx], s=rec["s"][idx], **carry(rec, idx))
    return run


def wrap64(measure, rec, q, i, qn, tn):
    N, D = SC.nd(measure, rec, q, i, qn, tn)
    return N, (D % (1 << 64)) or 1


def ignore_total(measure, rec, q, i, qn, tn):
    return SC.nd(measure, dict(rec, total=None) if measure == "jaccard" and qn is not None else rec, q, i, qn, tn)


MISREADINGS = {
    "float arithmetic": variant(kept=lambda m, N, D, num, den: (float(N) / float(D)) ** (0.5 if m == "cosine" else 1) >= float(num) / float(den),
                                before=lambda a, b: float(a[0]) / float(a[1]) > float(b[0]) / float(b[1]) or (float(a[0]) / float(a[1]) == float(b[0]) / float(b[1]) and a[2] < b[2])),
    "the cosine bound not squared": variant(kept=lambda m, N, D, num, den: N * den >= num * D),
    "ties by descending target": variant(before=lambda a, b: a[0] * b[1] > b[0] * a[1] or (a[0] * b[1] == b[0] * a[1] and a[2] > b[2])),
    "ties by shared": variant(before=lambda a, b: a[0] * b[1] > b[0] * a[1] or (a[0] * b[1] == b[0] * a[1] and (a[3] > b[3] or (a[3] == b[3] and a[2] < b[2])))),
    "D wrapped at 64 bits": variant(nd=wrap64),
    "a payload left behind": variant(carry=lambda rec, idx: {p: (None if rec[p] is None or p == "members" else rec[p][idx]) for p in SC.PAYLOADS}),
    "a payload gathered with the wrong index": variant(carry=lambda rec, idx: {p: (None if rec[p] is None else rec[p][np.sort(idx)] if p == "dot" else rec[p][idx]) for p in SC.PAYLOADS}),
    "> for >=": variant(kept=lambda m, N, D, num, den: (N * den * den > num * num * D) if m == "cosine" else (N * den > num * D)),
    "jaccard ignoring total": variant(nd=ignore_total),
}


def crafted():
    """(record, measure, op, arg, qnorm, tnorm)"""
    ties = SC.record([0, 4], [1, 2, 3, 4], [2, 3, 1, 2], [4, 6, 2, 5], [6, 12, 3, 9], [2, 3, 1, 2], [1, 2, 3, 1])  # 2/4 = 3/6 = 1/2, shared differs
    wide = SC.record([0, 3], [0, 1, 2], [3, 3, 5])
    tn = np.array([TOP64 - 1, TOP64 - 2, 1 << 63], U64)
    cases = [(ties, "jaccard", "top_by", 2, None, None), (ties, "jaccard", "top_by", 4, None, None), (ties, "jaccard", "filter", (1, 2), None, None),
             (ties, "jaccard", "filter", (1, 2), [9], [0, 9, 9, 9, 9]), (ties, "cosine", "filter", (3, 5), [10], [0, 10, 10, 10, 10]),  # cosine 6 / 10
             (ties, "dot", "top_by", 3, None, None), (ties, "members", "filter", (2, 1), None, None), (ties, "min_sum", "top_by", 4, None, None),
             (wide, "target_cov", "top_by", 3, None, tn), (wide, "target_cov", "filter", (3, TOP64 - 2), None, tn),
             (wide, "jaccard", "top_by", 3, [TOP64], tn), (wide, "jaccard", "filter", (1, 1 << 63), [TOP64], tn)]
    return cases


def test_the_model_agrees_with_its_unbent_variant():
    run = variant()
    for rec, measure, op, arg, qn, tn in crafted():
        want = SC.filter_model(rec, measure, arg[0], arg[1], qn, tn) if op == "filter" else SC.top_by_model(rec, measure, arg, qn, tn)
        assert not SC.same(run(rec, measure, op, arg, qn, tn), want), (measure, op, arg)


@pytest.mark.parametrize("what", sorted(MISREADINGS))
def test_every_misreading_is_caught(what):
    run, caught = MISREADINGS[what], []
    for rec, measure, op, arg, qn, tn in crafted():
        want = SC.filter_model(rec, measure, arg[0], arg[1], qn, tn) if op == "filter" else SC.top_by_model(rec, measure, arg, qn, tn)
        if SC.same(run(rec, measure, op, arg, qn, tn), want):
            caught.append((measure, op, arg))
    assert caught, what


def test_the_crafted_shapes():
    rec = SC.shape_record()
    lens = [int(x) for x in np.diff(rec["o"])]
    assert set(SC.ROW_LENGTHS) <= set(lens) and lens.count(1025) == 2 and 3000 < len(rec["t"]) < 10000
    o = rec["o"]
    for q in range(len(lens)):
        assert np.all(np.diff(rec["t"][int(o[q]):int(o[q + 1])].astype(np.int64)) > 0)  # strictly ascending: bsk_hits_from_host takes it
    row = slice(int(o[5]), int(o[6]))
    assert len(set(zip(rec["s"][row].tolist(), rec["total"][row].tolist()))) == 1 and lens[5] == 64  # a whole row tied
    fr = [Fraction(int(s), int(t)) for s, t in zip(rec["s"], rec["total"])]
    assert any(fr[i] == fr[j] and rec["s"][i] != rec["s"][j] for i in range(20, 60) for j in range(20, 60))  # equal fractions of different N and D
    (qo, qv, qc), (to, tv, tc) = SC.weighted_sets()
    assert len(qv) == len(qc) == int(qo[-1]) and len(tv) == len(tc) == int(to[-1]) and qc.min() >= 1 and tc.min() >= 1
    for j, L_j in enumerate(list(SC.ROW_LENGTHS) + [1025, 40]):
        v = qv[int(qo[j]):int(qo[j + 1])]
        assert np.all(np.diff(v.astype(np.int64)) > 0) and len(np.unique(v // U64(2))) == L_j and (L_j == 0 or int(v.max()) // 2 == L_j - 1)
    q, t = SC.wide_sets()
    assert all(len(x[1]) == len(x[2]) == int(x[0][-1]) for x in (q, t))
