"""GPU: bsk_hits_transpose and bsk_hits_tally against the NumPy model of tests/transpose_cases.py, against each other and against the
library itself (the neighbours and the search of b against a are the transposes of those of a against b): every row length on the
target side, every key width, every payload combination, both tally paths, BSK_TALLY_ADD, the result slot, the empties, the grid caps.
Every entry call is made twice into fresh objects and the two results compared byte for byte.  Everything is exact equality."""
import ctypes as C
import re

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import select_cases as SC
from tests import transpose_cases as TC
from tests.test_gpu_grid_caps import GRID_CAPS, grid_stats, switches
from tests.test_gpu_hits_select import NAMES, Zoo, rec_of

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
TP_PLAN = re.compile(r"bsk_hits_transpose: k_tp_keys \+ sort \+ k_tp_offsets \+ k_tp_place, targets=(\d+) hits=(\d+) key_bits=(\d+)")
TL_PLAN = re.compile(r"bsk_hits_tally( add)?: k_tl_check \+ (k_tl_add<lds>|k_tl_add<global>|nothing) .*targets=(\d+) hits=(\d+)")


def upload(engine, rec):
    return engine.hits_from_arrays(rec["o"], rec["t"], rec["s"], rec["total"])


def bits(x):
    return int(x).bit_length()


def transposed(h, nt):
    """h.transpose(nt) twice into fresh objects, byte-identical -> the record, after the plan said what it must"""
    a, b = h.transpose(nt), h.transpose(nt)
    ra, rb = rec_of(a), rec_of(b)
    assert not SC.same(ra, rb) and all(ra[k] is None or ra[k].tobytes() == rb[k].tobytes() for k in ra)
    inf, p = h.info(), a.plan()
    m = TP_PLAN.fullmatch(p["plan"])
    H = inf["n_hits"]
    assert m and (int(m.group(1)), int(m.group(2))) == (nt, H) and p["n_large_queries"] == 0, p
    assert int(m.group(3)) == (max(1, bits(H - 1)) + bits(max(nt, 1) - 1) if H else 0), p
    assert a.info() == dict(n_queries=nt, n_hits=H)
    a.close(), b.close()
    return ra


def tallied(h, nt, path=None):
    a, b = h.tally(nt), h.tally(nt)
    ta, tb = a.fetch(), b.fetch()
    assert not TC.same_table(ta, tb) and all(x.tobytes() == y.tobytes() for x, y in zip(ta, tb))
    inf = h.info()
    m = TL_PLAN.fullmatch(a.plan())
    assert m and (int(m.group(3)), int(m.group(4))) == (nt, inf["n_hits"]) and not m.group(1), a.plan()
    if inf["n_hits"]:
        assert m.group(2) == ("k_tl_add<lds>" if nt <= TC.TALLY_LDS_TARGETS else "k_tl_add<global>"), a.plan()
    assert a.info() == dict(n_targets=nt, queries=inf["n_queries"], hits=inf["n_hits"], calls=1)
    assert all(np.array_equal(x, y) for x, y in zip((a.rows, a.unique, a.shared), ta))
    a.close(), b.close()
    return ta


def segment_sums(o, s):
    cs = np.concatenate([[0], np.cumsum(s.astype(U64))]).astype(U64)
    return cs[o[1:].astype(np.int64)] - cs[o[:-1].astype(np.int64)]


@pytest.fixture(scope="module")
def zoo(engine):
    return Zoo(engine)


@pytest.fixture(scope="module")
def pair(engine):
    """two counted collections with crafted overlaps, 40 and 42 sets"""
    a, b = TC.symmetric_sets()
    return engine.sets_from_arrays_counted(*a), engine.sets_from_arrays_counted(*b)


# ---- the row lengths on the target side, the key widths ----
@pytest.mark.parametrize("with_total", [True, False])
def test_row_lengths_on_the_target_side(engine, with_total):
    rec, nt = TC.row_length_record(with_total)
    h = upload(engine, rec)
    got, want = transposed(h, nt), TC.transpose_model(rec, nt)
    assert not SC.same(got, want) and (got["total"] is not None) == with_total
    assert [int(x) for x in np.diff(got["o"])[::10][:15]] == list(TC.TARGET_ROW_LENGTHS) and not np.diff(got["o"])[150:].any()
    table = tallied(h, nt)
    assert not TC.same_table(table, TC.tally_model(rec, nt))
    # the two entries against each other
    assert np.array_equal(table[0], np.diff(got["o"])) and np.array_equal(table[2], segment_sums(got["o"], got["s"]))
    back = h.transpose(nt).transpose(3001)
    assert not SC.same(rec_of(back), rec)
    h.close()


@pytest.mark.parametrize("nt", TC.KEY_WIDTH_TARGETS)
def test_key_widths(engine, nt):
    rec = TC.key_width_record(nt)
    h = upload(engine, rec)
    got = transposed(h, nt)
    assert not SC.same(got, TC.transpose_model(rec, nt)) and int(got["o"][nt]) == len(rec["t"]) and int(got["o"][nt - 1]) < len(rec["t"])
    assert not TC.same_table(tallied(h, nt), TC.tally_model(rec, nt))
    assert not SC.same(rec_of(h.transpose(nt).transpose(5)), rec)
    h.close()


# ---- every payload combination ----
ZOO_TARGETS = {"none": 4200, "totals": 4200, "totals+weights": 2100, "weights": 2100, "weights, plain index": 2100, "members": 2100}


@pytest.mark.parametrize("name", NAMES)
def test_every_payload_combination(zoo, name):
    h, rec, _, _ = zoo.items[name]
    nt, nq = ZOO_TARGETS[name], len(rec["o"]) - 1
    got = transposed(h, nt)
    assert not SC.same(got, TC.transpose_model(rec, nt))  # (same() tells a payload carried by one side only)
    t = h.transpose(nt)
    assert (t.has_totals(), t.has_weights(), t.has_members()) == (rec["total"] is not None, rec["dot"] is not None, rec["members"] is not None)
    back = t.transpose(nq)
    assert not SC.same(rec_of(back), rec)  # ascending rows: twice is the input, bit for bit
    top = h.top_by(5, "shared")  # rows that are not ascending: legal input
    trec = rec_of(top)
    if rec["dot"] is None:  # (the weighted sets' rows happen to rank in target order)
        assert any(np.any(np.diff(trec["t"][int(a):int(b)].astype(np.int64)) < 0) for a, b in zip(trec["o"][:-1], trec["o"][1:]))
    assert not SC.same(transposed(top, nt), TC.transpose_model(trec, nt))
    assert not TC.same_table(tallied(top, nt), TC.tally_model(trec, nt))
    for x in (t, back, top):
        x.close()


# ---- symmetry against the library itself ----
def test_neighbors_of_b_against_a_are_the_transpose(pair):
    a, b = pair
    for kw in (dict(), dict(min_jaccard=(1, 8)), dict(min_jaccard=(1, 6), min_shared=3)):
        ab, ba = a.neighbors_counted(b, **kw), b.neighbors_counted(a, **kw)
        want = rec_of(ba)
        assert want["total"] is not None and want["dot"] is not None and 0 < len(want["t"]) < 40 * 42
        got = transposed(ab, len(b.offsets()) - 1)
        assert not SC.same(got, want), kw
        assert not SC.same(rec_of(ba.transpose(40)), rec_of(ab)), kw
        ab.close(), ba.close()


def test_search_of_b_against_a_is_the_transpose(pair):
    a, b = pair
    ia, ib = a.index_counted(), b.index_counted()
    kept = []
    for x, y in ((0.0, 0.0), (0.25, 0.125), (0.375, 0.0625), (0.125, 0.3125)):  # dyadic: the covers' double expression is exact on both sides
        ab = ib.search_counted(a, min_query_cov=x, min_target_cov=y)
        ba = ia.search_counted(b, min_query_cov=y, min_target_cov=x)
        want = rec_of(ba)
        assert want["dot"] is not None and want["total"] is None
        assert not SC.same(transposed(ab, 42), want), (x, y)
        kept.append(len(want["t"]))
        ab.close(), ba.close()
    assert kept[0] > max(kept[1:]) and any(kept[1:])  # the thresholds bite, and not everywhere
    ia.close(), ib.close()


# ---- chains ----
def test_best_query_per_target_and_folded_members(engine):
    rec, nt = TC.row_length_record()
    h = upload(engine, rec)
    t = h.transpose(nt)
    best = t.top_by(1, "shared")
    assert not SC.same(rec_of(best), SC.top_by_model(TC.transpose_model(rec, nt), "shared", 1))
    go = np.arange(0, nt + 1, 20, dtype=U64)  # groups of 20 targets: two of the hit targets each
    folded = h.fold(go)
    frec = rec_of(folded)
    assert frec["members"] is not None and int(frec["members"].max()) == 2
    ft = transposed(folded, len(go) - 1)
    assert not SC.same(ft, TC.transpose_model(frec, len(go) - 1)) and ft["members"] is not None
    assert not TC.same_table(folded.top_by(1, "members").tally().fetch(), TC.tally_model(SC.top_by_model(frec, "members", 1), len(go) - 1))
    # rectangular hits: the clusters contract refuses a target >= n_queries
    with pytest.raises(S.DeviceError, match="bad argument"):
        t.cluster()
    for x in (h, t, best, folded):
        x.close()


def test_clusters_of_a_transposed_square_graph(pair):
    a, _ = pair
    h = a.neighbors(a, min_jaccard=(1, 8))
    t = h.transpose()
    assert not SC.same(rec_of(t), rec_of(h))  # a symmetric relation is its own transpose
    got, want = t.cluster(), h.cluster()
    assert np.array_equal(got.label, want.label) and np.array_equal(got.rep, want.rep) and 1 < got.info()["n_clusters"] < 40
    for x in (h, t, got, want):
        x.close()


def test_python_formulas_on_the_transposed_object(pair):
    a, b = pair
    h = a.neighbors_counted(b)
    t = h.transpose()
    assert t.info()["n_queries"] == 42 and np.array_equal(t.query_sizes, h.target_sizes) and np.array_equal(t.target_sizes, h.query_sizes)
    perm = np.argsort(h.target, kind="stable")
    for f in ("jaccard", "cosine", "weighted_jaccard", "bray_curtis", "angular_similarity"):
        assert np.array_equal(getattr(t, f)(), getattr(h, f)()[perm]), f
    assert np.array_equal(t.containment(), h.shared[perm].astype(np.float64) / h.target_sizes[h.target[perm].astype(np.int64)].astype(np.float64))
    trec = rec_of(t)
    assert not SC.same(rec_of(t.filter("cosine", (1, 2))), SC.filter_model(trec, "cosine", 1, 2, b.sumsq(), a.sumsq()))  # the default norms, swapped
    assert not SC.same(rec_of(t.top_by(2, "jaccard")), SC.top_by_model(trec, "jaccard", 2))
    assert not SC.same(rec_of(t.filter("query_cov", (1, 2))), SC.filter_model(trec, "query_cov", 1, 2, np.diff(b.offsets()), None))
    with pytest.raises(ValueError, match="one-sided"):
        t.weighted_containment()
    # the one-sided formula: defined on the hits of a plain index, refused on their transpose, back again on the transpose of that
    plain = b.index()
    hp = plain.search_counted(a)
    wc = hp.weighted_containment()
    tp = hp.transpose()
    with pytest.raises(ValueError, match="one-sided"):
        tp.weighted_containment()
    with pytest.raises(ValueError):
        tp.filter("weighted_containment", (1, 2))
    assert np.array_equal(tp.cosine(), hp.cosine()[np.argsort(hp.target, kind="stable")])
    assert np.array_equal(tp.transpose().weighted_containment(), wc)
    for x in (h, t, hp, tp, plain):
        x.close()


# ---- the tally's paths ----
@pytest.mark.parametrize("nt", [TC.TALLY_LDS_TARGETS, TC.TALLY_LDS_TARGETS + 1])
def test_tally_at_the_lds_bound(engine, nt):
    for rec in (TC.spread_record(nt), TC.spread_record(nt, one_target=nt - 1), TC.spread_record(nt, one_target=0)):
        h = upload(engine, rec)
        got, want = tallied(h, nt), TC.tally_model(rec, nt)
        assert not TC.same_table(got, want) and int(got[2].max()) > 1 << 32  # a sum beyond 32 bits, exact
        assert not SC.same(transposed(h, nt), TC.transpose_model(rec, nt))
        h.close()


def test_unique_on_rows_of_no_one_and_two_hits(engine):
    rec = TC.unique_record()
    h = upload(engine, rec)
    got = tallied(h, 3)
    assert [list(map(int, x)) for x in got] == [[2, 1, 4], [1, 0, 2], [8, 4, 16]]
    assert not TC.same_table(tallied(h, 5000), TC.tally_model(rec, 5000))  # the same through global memory
    h.close()


def test_tally_add(engine):
    rng = np.random.default_rng(41)
    for nt in (300, 3000):  # both paths
        recs = [TC.random_record(rng, n, nt, 12) for n in (200, 1, 333)]
        hs = [upload(engine, r) for r in recs]
        table = hs[0].tally(nt, add=True)  # a NULL slot under ADD is a fresh table
        for h in hs[1:]:
            assert h.tally(nt, into=table, add=True) is table
        want = TC.tally_model(TC.concat(recs), nt)
        assert not TC.same_table(table.fetch(), want)
        assert table.info() == dict(n_targets=nt, queries=534, hits=sum(len(r["t"]) for r in recs), calls=3) and " add" in table.plan()
        both = upload(engine, TC.concat(recs))
        assert not TC.same_table(tallied(both, nt), want)
        # refused: another n_targets, a target >= n_targets -- the table is bit-identical, its figures too
        before, held, info = table.fetch(), table.h.value, table.info()
        with pytest.raises(S.DeviceError, match="another n_targets"):
            hs[0].tally(nt + 1, into=table, add=True)
        high = upload(engine, SC.record([0, 2], [0, nt], [1, 1]))
        with pytest.raises(S.DeviceError, match="a target >= n_targets"):
            high.tally(nt, into=table, add=True)
        assert table.h.value == held and table.info() == info and all(x.tobytes() == y.tobytes() for x, y in zip(table.fetch(), before))
        # ... and without ADD the re-used object is overwritten
        assert hs[1].tally(nt, into=table) is table and not TC.same_table(table.fetch(), TC.tally_model(recs[1], nt)) and table.info()["calls"] == 1
        # a fetch of a range, and beyond the table
        r, u, s = table.fetch(nt - 7, 7)
        assert all(np.array_equal(x, y[nt - 7:]) for x, y in zip((r, u, s), TC.tally_model(recs[1], nt)))
        with pytest.raises(S.DeviceError, match="range outside the table"):
            table.fetch(nt - 7, 8)
        ptrs = table.device()
        assert all(ptrs) and ptrs[1] - ptrs[0] == 8 * nt and ptrs[2] - ptrs[1] == 8 * nt
        for x in hs + [table, both, high]:
            x.close()


# ---- the result slot ----
def test_reuse_into_objects_of_every_history(engine, pair):
    a, b = pair
    small = SC.record([0, 2, 3], [1, 4, 4], [7, 8, 9])
    big, nt = TC.row_length_record()
    weighted = a.neighbors_counted(b)
    wrec = rec_of(weighted)

    def slots():
        folded = upload(engine, TC.row_length_record(False)[0]).fold(np.arange(0, 201, 20, dtype=U64))
        return dict(none=upload(engine, small), totals=upload(engine, big), weights=a.neighbors_counted(a), members=folded)

    for name, slot in slots().items():  # a small input without payloads into every history
        res = upload(engine, small).transpose(5, reuse=slot)
        assert res is slot and not SC.same(rec_of(res), TC.transpose_model(small, 5)), name
        assert not (res.has_totals() or res.has_weights() or res.has_members()), name
        slot.close()
    for name, slot in slots().items():  # totals and weights into every history
        res = weighted.transpose(42, reuse=slot)
        assert res is slot and not SC.same(rec_of(res), TC.transpose_model(wrec, 42)), name
        assert res.has_totals() and res.has_weights() and not res.has_members(), name
        slot.close()
    for name, slot in slots().items():  # the larger input with totals
        res = upload(engine, big).transpose(nt, reuse=slot)
        assert res is slot and not SC.same(rec_of(res), TC.transpose_model(big, nt)), name
        slot.close()
    weighted.close()


def test_every_argument_error_keeps_the_slot(engine):
    lib = engine.lib
    rec, nt = TC.row_length_record()
    h = upload(engine, rec)
    res, table = h.transpose(nt), h.tally(nt)
    before, tbefore = rec_of(res), table.fetch()
    slot, tslot = C.c_void_p(res.h.value), C.c_void_p(table.h.value)
    other = S.Engine(0)
    foreign = other.hits_from_arrays(np.array([0, 1], U64), np.array([0], U32), np.array([1], U32))
    ftable = foreign.tally(3)
    fslot, ftslot = C.c_void_p(foreign.h.value), C.c_void_p(ftable.h.value)
    bad = [("null hits", engine.ctx, None, nt, slot, tslot), ("null ctx", None, h.h, nt, slot, tslot), ("foreign hits", engine.ctx, foreign.h, nt, slot, tslot),
           ("foreign context", other.ctx, h.h, nt, slot, tslot), ("foreign slot", engine.ctx, h.h, nt, fslot, ftslot),
           ("target >= n_targets", engine.ctx, h.h, 140, slot, tslot), ("no targets", engine.ctx, h.h, 0, slot, tslot)]
    for what, ctx, hh, n, sl, tsl in bad:
        held, theld = sl.value, tsl.value
        assert lib.bsk_hits_transpose(ctx, hh, n, C.byref(sl)) == L.ERR_ARG and sl.value == held, what
        for flags in (0, L.TALLY_ADD):
            assert lib.bsk_hits_tally(ctx, hh, n, flags, C.byref(tsl)) == L.ERR_ARG and tsl.value == theld, what
    assert lib.bsk_hits_transpose(engine.ctx, res.h, 3001, C.byref(slot)) == L.ERR_ARG and slot.value == res.h.value  # *out == h
    assert b"holds h itself" in lib.bsk_last_error(engine.ctx)
    assert lib.bsk_hits_transpose(engine.ctx, h.h, 1 << 32, C.byref(slot)) == L.ERR_UNSUPPORTED and slot.value == res.h.value
    assert lib.bsk_hits_tally(engine.ctx, h.h, 1 << 32, 0, C.byref(tslot)) == L.ERR_UNSUPPORTED and tslot.value == table.h.value
    for flags in (2, 3, 0x80000000):
        assert lib.bsk_hits_tally(engine.ctx, h.h, nt, flags, C.byref(tslot)) == L.ERR_ARG and tslot.value == table.h.value
    assert lib.bsk_hits_tally(engine.ctx, h.h, nt + 1, L.TALLY_ADD, C.byref(tslot)) == L.ERR_ARG and tslot.value == table.h.value
    assert lib.bsk_hits_transpose(engine.ctx, h.h, nt, None) == L.ERR_ARG and lib.bsk_hits_tally(engine.ctx, h.h, nt, 0, None) == L.ERR_ARG
    assert lib.bsk_tally_fetch(other.ctx, table.h, 0, 1, None, None, None) == L.ERR_ARG
    # readable and unchanged
    assert not SC.same(rec_of(res), before) and all(x.tobytes() == y.tobytes() for x, y in zip(table.fetch(), tbefore)) and table.info()["calls"] == 1
    # ... and the same calls with nothing wrong go through, into those slots
    assert lib.bsk_hits_transpose(engine.ctx, h.h, nt + 9, C.byref(slot)) == L.OK and slot.value == res.h.value and res.info()["n_queries"] == nt + 9
    assert lib.bsk_hits_tally(engine.ctx, h.h, nt, L.TALLY_ADD, C.byref(tslot)) == L.OK and tslot.value == table.h.value and table.info()["calls"] == 2
    with pytest.raises(S.DeviceError, match="bad argument: bsk_hits_transpose: the result slot holds h itself"):
        res.transpose(3001, reuse=res)
    for x in (h, res, table, foreign, ftable, other):
        x.close()


# ---- the empties ----
def test_empties(engine):
    for o in (np.zeros(1, U64), np.zeros(5, U64)):  # no queries; queries without hits
        for total in (None, np.zeros(0, U32)):
            h = engine.hits_from_arrays(o, np.zeros(0, U32), np.zeros(0, U32), total)
            for nt in (0, 4):
                got = transposed(h, nt)
                assert np.array_equal(got["o"], np.zeros(nt + 1, U64)) and len(got["t"]) == 0 and (got["total"] is not None) == (total is not None)
                table = tallied(h, nt)
                assert all(len(x) == nt and not x.any() for x in table)
            h.close()
    # hits, but targets nobody hit before, between and after them
    rec = SC.record([0, 1, 1, 2], [3, 3], [5, 6])
    h = upload(engine, rec)
    assert not SC.same(transposed(h, 9), TC.transpose_model(rec, 9)) and list(map(int, tallied(h, 9)[1])) == [0, 0, 0, 2, 0, 0, 0, 0, 0]
    h.close()


# ---- under a grid cap ----
def caps_cases():
    rec, nt = TC.row_length_record()
    return [("row lengths", rec, nt), ("lds, spread", TC.spread_record(TC.TALLY_LDS_TARGETS, per_target=20), TC.TALLY_LDS_TARGETS),
            ("global, spread", TC.spread_record(TC.TALLY_LDS_TARGETS + 1, per_target=20), TC.TALLY_LDS_TARGETS + 1),
            ("lds, one target", TC.spread_record(TC.TALLY_LDS_TARGETS, per_target=20, one_target=5), TC.TALLY_LDS_TARGETS)]


@pytest.mark.parametrize("case", range(4))
def test_under_a_grid_cap_the_record_is_the_same(engine, case):
    what, rec, nt = caps_cases()[case]
    h = upload(engine, rec)
    want, twant = TC.transpose_model(rec, nt), TC.tally_model(rec, nt)
    for cap in (None,) + GRID_CAPS:
        with switches(engine, dict(BSK_GRID_CAP=None if cap is None else str(cap))):
            s0, c0 = grid_stats(engine)
            t = h.transpose(nt)
            s1, c1 = grid_stats(engine)
            table = h.tally(nt)
            s2, c2 = grid_stats(engine)
        assert s1 - s0 == 3 and s2 - s1 == 2, (what, cap)  # keys, offsets, place; check, add
        if cap is None:
            assert c1 - c0 == 0 and c2 - c1 == 0, (what, cap)
        else:
            assert c1 - c0 >= 2 and c2 - c1 >= 1 + (cap == 1 and case != 0), (what, cap, c1 - c0, c2 - c1)  # the grids were cut
        assert not SC.same(rec_of(t), want) and not TC.same_table(table.fetch(), twant), (what, cap)
        t.close(), table.close()
    h.close()
