"""CPU: the NumPy model of the hits by target (tests/transpose_cases.py) against a brute-force double loop, its involution on ascending
rows, and the wrong models its cases must tell from the right one."""
import numpy as np
import pytest

from tests import select_cases as SC
from tests import transpose_cases as TC

U64, U32 = np.uint64, np.uint32


def small_cases():
    rng = np.random.default_rng(1)
    out = []
    for k in range(40):
        payloads = (("total",), (), ("total", "dot"), ("dot",), ("members",))[k % 5]
        out.append((TC.random_record(rng, int(rng.integers(0, 9)), int(rng.integers(1, 12)), 6, payloads, ascending=k % 3 != 2, repeats=k % 4 == 3), int(rng.integers(12, 16))))
    return out


def test_model_against_the_double_loop():
    for rec, nt in small_cases():
        assert not SC.same(TC.transpose_model(rec, nt), TC.transpose_brute(rec, nt))
        assert not TC.same_table(TC.tally_model(rec, nt), TC.tally_brute(rec, nt))
    for rec, nt in ((TC.unique_record(), 3), (TC.key_width_record(3), 3), (TC.key_width_record(1), 1)):
        assert not SC.same(TC.transpose_model(rec, nt), TC.transpose_brute(rec, nt))
        assert not TC.same_table(TC.tally_model(rec, nt), TC.tally_brute(rec, nt))
    assert [list(x) for x in TC.tally_model(TC.unique_record(), 3)] == [[2, 1, 4], [1, 0, 2], [8, 4, 16]]


def test_model_is_an_involution_on_ascending_rows():
    rng = np.random.default_rng(2)
    for k in range(20):
        rec = TC.random_record(rng, int(rng.integers(0, 30)), 25, 9, (("total", "dot"), ("members",), ())[k % 3])
        nq = len(rec["o"]) - 1
        for nt in (25, 26, 40):
            back = TC.transpose_model(TC.transpose_model(rec, nt), nq)
            assert not SC.same(back, rec)
    rec, nt = TC.row_length_record()
    assert not SC.same(TC.transpose_model(TC.transpose_model(rec, nt), 3001), rec)


def test_the_builders_build_what_they_say():
    rec, nt = TC.row_length_record()
    lens = np.diff(TC.transpose_model(rec, nt)["o"]).astype(int)
    assert nt == 200 and [int(lens[10 * k]) for k in range(15)] == list(TC.TARGET_ROW_LENGTHS) and lens.sum() == sum(TC.TARGET_ROW_LENGTHS)
    assert not lens[141:].any() and len(rec["o"]) == 3002 and rec["total"] is not None and TC.row_length_record(False)[0]["total"] is None
    for nt in TC.KEY_WIDTH_TARGETS:
        rec = TC.key_width_record(nt)
        assert int(rec["t"].max()) == nt - 1 and 0 in np.diff(rec["o"]).tolist()
    for nt in (TC.TALLY_LDS_TARGETS, TC.TALLY_LDS_TARGETS + 1):
        even, one = TC.spread_record(nt), TC.spread_record(nt, one_target=nt - 1)
        assert set(np.bincount(even["t"].astype(int), minlength=nt).tolist()) == {3} and set(one["t"].tolist()) == {nt - 1}
        assert {1, 2} == set(np.diff(even["o"]).astype(int).tolist()) and int(TC.tally_model(one, nt)[2][nt - 1]) > 1 << 32
        o, t = even["o"], even["t"].astype(np.int64)
        assert all(np.all(np.diff(t[int(a):int(b)]) >= 0) for a, b in zip(o[:-1], o[1:]))
    a, b = TC.symmetric_sets()
    assert len(a[0]) - 1 == 40 and len(b[0]) - 1 == 42
    with pytest.raises(SC.BadHits):
        TC.transpose_model(TC.unique_record(), 2)
    with pytest.raises(SC.BadHits):
        TC.tally_model(TC.unique_record(), 2)


def test_concat_is_the_rows_one_after_another():
    rng = np.random.default_rng(3)
    recs = [TC.random_record(rng, n, 10, 5) for n in (4, 0, 7)]
    both = TC.concat(recs)
    assert len(both["o"]) - 1 == 11 and int(both["o"][-1]) == sum(len(r["t"]) for r in recs) and both["total"] is not None
    table = None
    for r in recs:
        table = TC.tally_model(r, 10, into=table)
    assert not TC.same_table(table, TC.tally_model(both, 10))


def test_wrong_models_are_caught():
    """every wrong model differs from the right one on at least one of the cases the GPU tests run"""
    rng = np.random.default_rng(4)
    twice = TC.random_record(rng, 12, 5, 6, ("total",), repeats=True)  # rows that name a target twice: the order inside a target's row shows
    assert any(np.any(np.diff(np.sort(twice["t"][int(a):int(b)].astype(int))) == 0) for a, b in zip(twice["o"][:-1], twice["o"][1:]))
    shape, nt = TC.row_length_record()
    cases = [(twice, 5), (shape, nt), (TC.key_width_record(257), 257), (TC.unique_record(), 3)]
    for wrong in (TC.wrong_unstable, TC.wrong_payload_stays, TC.wrong_drops_trailing, TC.wrong_total_stays):
        assert any(SC.same(wrong(rec, n), TC.transpose_model(rec, n)) for rec, n in cases), wrong.__name__
    # the trailing rows show only where the last targets are unhit
    assert SC.same(TC.wrong_unstable(twice, 5), TC.transpose_model(twice, 5))
    assert SC.same(TC.wrong_drops_trailing(shape, nt), TC.transpose_model(shape, nt))
    assert any(TC.same_table(TC.wrong_unique_per_hit(rec, n), TC.tally_model(rec, n)) for rec, n in cases)
    first = TC.tally_model(shape, nt)
    assert TC.same_table(TC.wrong_add_overwrites(TC.unique_record(), nt, into=first), TC.tally_model(TC.unique_record(), nt, into=first))
    assert not TC.same_table(first, TC.tally_model(shape, nt))  # adding leaves its operand alone
