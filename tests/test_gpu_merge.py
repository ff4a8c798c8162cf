"""GPU: bsk_hits_merge against the NumPy model of tests/merge_cases.py and against the library itself (the hits against a database split
by target, or by value, merged, are the hits against the whole): every merged row length on both paths, the part counts, every payload
combination, duplicates and saturation, the result slot, contexts, the empties, the grid caps.  Every call is made twice into fresh
objects and the two results compared byte for byte.  Everything is exact equality."""
import ctypes as C
import re

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import merge_cases as MC
from tests import search_counted_cases as W
from tests import select_cases as SC
from tests import transpose_cases as TC
from tests.test_gpu_grid_caps import GRID_CAPS, grid_stats, switches
from tests.test_gpu_hits_select import NAMES, Zoo, rec_of
from tests.test_gpu_index_attach import free_bytes, n_devices

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
MG_PLAN = re.compile(r"bsk_hits_merge: (k_mg_check \+ k_mg_starts \+ k_mg_place(?: \+ segmented sort \+ k_mg_heads \+ k_mg_runs \+ k_mg_offsets)?), "
                     r"path=(concat|sort) parts=(\d+) hits=(\d+) combined=(\d+)")


def upload(engine, rec):
    return engine.hits_from_arrays(rec["o"], rec["t"], rec["s"], rec["total"])


def figures(h):
    p = h.plan()
    m = MG_PLAN.fullmatch(p["plan"])
    assert m and p["n_large_queries"] == 0 and ("sort" in m.group(1)) == (m.group(2) == "sort"), p
    return dict(path=m.group(2), parts=int(m.group(3)), hits=int(m.group(4)), combined=int(m.group(5)))


def identical(ra, rb):
    return not SC.same(ra, rb) and all(ra[k] is None or ra[k].tobytes() == rb[k].tobytes() for k in ra)


def merged(engine, parts, bases, add=False):
    """engine.merge_hits twice into fresh objects, byte-identical -> (the record, the plan's figures)"""
    a, b = engine.merge_hits(parts, bases, add), engine.merge_hits(parts, bases, add)
    ra, rb = rec_of(a), rec_of(b)
    assert identical(ra, rb)
    fig = figures(a)
    assert a.info() == dict(n_queries=len(ra["o"]) - 1, n_hits=len(ra["t"])) and fig["hits"] - fig["combined"] == len(ra["t"])
    a.close(), b.close()
    return ra, fig


def raw_merge(engine, handles, bases=None, flags=0, slot=None, ctx="own"):
    """the C entry itself -> (return code, the slot)"""
    arr = (C.c_void_p * max(len(handles), 1))(*handles)
    b = None if bases is None else (C.c_uint64 * max(len(bases), 1))(*bases)
    slot = C.c_void_p() if slot is None else slot
    return engine.lib.bsk_hits_merge(engine.ctx if ctx == "own" else ctx, arr, b, len(handles), flags, C.byref(slot)), slot


def wrapped(engine, slot, nq):
    h = S.Hits(engine)
    h._bind(slot, np.zeros(nq, U64), np.zeros(0, U64))
    return h


def upload_unsorted(engine, rec):
    """hits whose rows are not ascending, or name a target twice: nothing the library produces has such rows and bsk_hits_from_host
    refuses them, so the targets of an uploaded object are overwritten where they are"""
    lens = np.diff(rec["o"]).astype(np.int64)
    place = np.concatenate([np.arange(c) for c in lens] + [np.zeros(0, np.int64)]).astype(U32)
    h = upload(engine, dict(rec, t=place))
    t = np.ascontiguousarray(rec["t"], U32)
    po, pt, ps = h.device()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    engine.sync()
    assert hip.hipMemcpy(pt, t.ctypes.data, t.nbytes, 1) == 0  # hipMemcpyHostToDevice, inside the array of len(t) targets
    assert np.array_equal(h.fetch()[1], t)
    return h


def flags_of(h):
    return tuple(p for p, has in (("total", h.has_totals()), ("dot", h.has_weights()), ("msum", h.has_weights()), ("members", h.has_members())) if has)


@pytest.fixture(scope="module")
def zoo(engine):
    return Zoo(engine)


# ---- 1. the merged row lengths, on both paths ----
@pytest.mark.parametrize("interleaved", [False, True])
def test_row_lengths(engine, interleaved):
    parts, bases = MC.row_length_parts(interleaved)
    hs = [upload(engine, r) for r in parts]
    got, fig = merged(engine, hs, bases)
    want, wfig = MC.merge_model(parts, bases)
    assert fig == wfig and fig["path"] == ("sort" if interleaved else "concat") and fig["combined"] == 0
    assert not SC.same(got, want) and np.diff(got["o"]).astype(int).tolist()[:16] == list(MC.MERGED_ROW_LENGTHS)
    got, fig = merged(engine, hs, bases, add=True)  # ADD with nothing to add is the same result
    assert not SC.same(got, want) and fig == wfig
    for h in hs:
        h.close()


# ---- 2. the part counts ----
@pytest.mark.parametrize("n", [1, 2, 3, 8, MC.MAX_PARTS])
def test_part_counts(engine, n):
    parts, bases = MC.many_parts(n)
    if n == 1:
        bases = (77,)  # one part with a base: a relabelling
    hs = [upload(engine, r) for r in parts]
    got, fig = merged(engine, hs, bases)
    want, wfig = MC.merge_model(parts, bases)
    assert not SC.same(got, want) and fig == wfig and fig["parts"] == n and fig["path"] == "concat"
    if n == 1:
        assert np.array_equal(got["t"], parts[0]["t"] + U32(77)) and np.array_equal(got["o"], parts[0]["o"])
    got, fig = merged(engine, hs, bases[::-1])  # the bases in reverse: the shifted ranges decrease with p
    want, wfig = MC.merge_model(parts, bases[::-1])
    assert not SC.same(got, want) and fig == wfig and fig["path"] == ("sort" if n > 1 else "concat")
    for h in hs:
        h.close()


def test_no_parts_and_too_many_are_refused(engine):
    h = upload(engine, SC.record([0, 1], [3], [4]))
    for parts in ([], [h] * (MC.MAX_PARTS + 1)):
        with pytest.raises(S.DeviceError, match="bad argument: bsk_hits_merge: n_parts is 0 or beyond"):
            engine.merge_hits(parts, list(range(len(parts))))
    got, _ = merged(engine, [h] * MC.MAX_PARTS, list(range(MC.MAX_PARTS)))  # one object 64 times, behind itself
    assert got["t"].tolist() == list(range(3, 3 + MC.MAX_PARTS)) and got["s"].tolist() == [4] * MC.MAX_PARTS
    h.close()


# ---- 3. every payload combination, each path once per combination ----
@pytest.mark.parametrize("name", NAMES)
def test_every_payload_combination_with_itself(engine, zoo, name):
    h, rec, _, _ = zoo.items[name]
    nt = int(rec["t"].max()) + 1
    seen = set()
    for bases, add, path in MC.self_merge_plans(nt):
        got, fig = merged(engine, [h, h], bases, add)
        want, wfig = MC.merge_model([rec, rec], bases, add)
        assert not SC.same(got, want) and fig == wfig and fig["path"] == path, (name, path, SC.same(got, want))
        assert tuple(p for p in SC.PAYLOADS if got[p] is not None) == tuple(p for p in SC.PAYLOADS if rec[p] is not None)  # exactly its payloads
        seen.add(fig["path"])
    assert seen == {"concat", "sort"}
    with pytest.raises(S.DeviceError, match="names a target twice"):
        engine.merge_hits([h, h], (0, 0))


def test_every_mixed_pair_carries_the_intersection(engine, zoo):
    kept, refused = set(), 0
    for x in NAMES:
        for y in NAMES:
            if x == y:
                continue
            (hx, rx, _, _), (hy, ry, _, _) = zoo.items[x], zoo.items[y]
            base = int(rx["t"].max()) + 1
            rc, slot = raw_merge(engine, [hx.h, hy.h], (0, base))
            if len(rx["o"]) != len(ry["o"]):
                assert rc == L.ERR_ARG and not slot.value and b"differ in their rows" in engine.lib.bsk_last_error(engine.ctx), (x, y)
                refused += 1
                continue
            assert rc == L.OK, (x, y)
            res = wrapped(engine, slot, len(rx["o"]) - 1)
            want, wfig = MC.merge_model([rx, ry], (0, base))
            assert not SC.same(rec_of(res), want) and figures(res) == wfig and flags_of(res) == MC.carried([rx, ry]), (x, y)
            kept.add(MC.carried([rx, ry]))
            res.close()
    assert {(), ("dot", "msum")} <= kept and refused  # members meet totals: neither; weights meet weights and totals: the weights


def test_reuse_into_objects_of_every_history(engine, zoo):
    small = [SC.record([0, 2, 3], [1, 4, 4], [7, 8, 9]), SC.record([0, 0, 1], [2], [5])]
    big, bbases = MC.row_length_parts(False)
    weighted, wrec = zoo.items["totals+weights"][0], zoo.items["totals+weights"][1]
    wnt = int(wrec["t"].max()) + 1

    def slots():
        folded = upload(engine, TC.row_length_record(False)[0]).fold(np.arange(0, 201, 20, dtype=U64))
        return dict(none=upload(engine, small[0]), totals=upload(engine, big[2]), weights=zoo.a.neighbors_counted(zoo.a), members=folded)

    hs = [upload(engine, r) for r in small]
    for name, slot in slots().items():  # small inputs without payloads into every history
        res = engine.merge_hits(hs, (0, 5), reuse=slot)
        assert res is slot and not SC.same(rec_of(res), MC.merge_model(small, (0, 5))[0]) and flags_of(res) == (), name
        slot.close()
    for name, slot in slots().items():  # totals and weights into every history, on the sort path
        res = engine.merge_hits([weighted, weighted], (0, 0), add=True, reuse=slot)
        assert res is slot and not SC.same(rec_of(res), MC.merge_model([wrec, wrec], (0, 0), True)[0]) and flags_of(res) == ("total", "dot", "msum"), name
        res = engine.merge_hits([weighted, weighted], (0, wnt), reuse=slot)  # ... and again into what that left, on the other path
        assert res is slot and not SC.same(rec_of(res), MC.merge_model([wrec, wrec], (0, wnt))[0]), name
        slot.close()
    bs = [upload(engine, r) for r in big]
    for name, slot in slots().items():  # the larger input with totals
        res = engine.merge_hits(bs, bbases, reuse=slot)
        assert res is slot and not SC.same(rec_of(res), MC.merge_model(big, bbases)[0]) and flags_of(res) == ("total",), name
        slot.close()
    for h in hs + bs:
        h.close()


# ---- 4. shards by target are the search ----
@pytest.fixture(scope="module")
def database(engine):
    t, tc, q, qc = MC.search_sets()
    return dict(t=t, tc=tc, whole=engine.sets_from_arrays_counted(t[0], t[1], tc), queries=engine.sets_from_arrays_counted(q[0], q[1], qc))


def test_shards_by_target_are_the_search(engine, database):
    cuts = [0, 11, 12, 37]
    shards = [engine.sets_from_arrays_counted(c[0], c[1], k) for c, k in MC.target_shards(database["t"], database["tc"], cuts)]
    Q, T = database["queries"], database["whole"]
    go = np.array([0, 5, 11, 12, 20, 37], U64)
    for counted in (True, False):
        whole_ix = T.index_counted() if counted else T.index()
        ixs = [s.index_counted() if counted else s.index() for s in shards]
        for weights in (True, False):
            search = (lambda ix: ix.search_counted(Q, 2, 0.3)) if weights else (lambda ix: ix.search(Q, 2, 0.3))
            whole, parts = search(whole_ix), [search(ix) for ix in ixs]
            wrec = rec_of(whole)
            assert len(wrec["t"]) == 186 and int(np.diff(wrec["o"]).max()) > 3 and (wrec["dot"] is not None) == weights
            got, fig = merged(engine, parts, None)  # the default bases: the running sum of the shards' targets
            assert not SC.same(got, wrec) and fig["path"] == "concat" and fig["parts"] == 3, (counted, weights)
            m = engine.merge_hits(parts)
            assert np.array_equal(m.target_sizes, whole.target_sizes) and np.array_equal(m.query_sizes, whole.query_sizes)
            # reduce every shard to its best three, merge, take the best three again
            tops = [p.top(3) for p in parts]
            mt = engine.merge_hits(tops)
            assert figures(mt)["path"] == "sort" and not SC.same(rec_of(mt.top(3)), rec_of(whole.top(3))), (counted, weights)
            assert not TC.same_table(m.fold(go).top_by(1, "members").tally().fetch(), whole.fold(go).top_by(1, "members").tally().fetch())
            assert not SC.same(rec_of(m.transpose()), rec_of(whole.transpose()))
            if weights:
                assert np.array_equal(m.cosine(), whole.cosine()) and np.array_equal(m.weighted_jaccard(), whole.weighted_jaccard())
                assert not SC.same(rec_of(m.top_by(2, "cosine")), rec_of(whole.top_by(2, "cosine")))
                if not counted:
                    assert np.array_equal(m.weighted_containment(), whole.weighted_containment())
            for x in [whole, m, mt] + parts + tops:
                x.close()
        for x in [whole_ix] + ixs:
            x.close()
    for s in shards:
        s.close()


# ---- 5. shards by value are the search ----
def test_shards_by_value_are_the_search(engine, database):
    shards = [engine.sets_from_arrays_counted(c[0], c[1], k) for c, k in MC.value_shards(database["t"], database["tc"], 2)]
    Q, T = database["queries"], database["whole"]
    whole_ix, ixs = T.index_counted(), [s.index_counted() for s in shards]
    whole, parts = whole_ix.search_counted(Q, 1), [ix.search_counted(Q, 1) for ix in ixs]
    wrec = rec_of(whole)
    got, fig = merged(engine, parts, (0, 0), add=True)
    assert not SC.same(got, wrec) and fig["path"] == "sort" and 0 < fig["combined"] == sum(len(rec_of(p)["t"]) for p in parts) - len(wrec["t"])
    assert not SC.same(got, MC.merge_model([rec_of(p) for p in parts], (0, 0), True)[0])
    with pytest.raises(S.DeviceError, match="names a target twice"):
        engine.merge_hits(parts, (0, 0))
    m = engine.merge_hits(parts, (0, 0), add=True)
    assert np.array_equal(m.target_sizes, whole.target_sizes)  # a value shard holds part of every target
    three = whole_ix.search_counted(Q, 3)
    assert 0 < three.info()["n_hits"] < whole.info()["n_hits"]
    assert not SC.same(rec_of(m.filter("shared", 3)), rec_of(three))  # the threshold is on the sum
    assert np.array_equal(m.cosine(), whole.cosine()) and np.array_equal(m.weighted_jaccard(), whole.weighted_jaccard())
    plain = [ix.search(Q, 1) for ix in ixs]  # ... and without payloads
    assert not SC.same(merged(engine, plain, (0, 0), add=True)[0], rec_of(whole_ix.search(Q, 1)))
    for x in [whole, m, three, whole_ix] + parts + plain + ixs + shards:
        x.close()


# ---- 6. duplicates and saturation ----
def test_duplicates_and_saturation(engine):
    across, inside, saturating = MC.duplicate_parts()
    held = upload(engine, across[0]).transpose(7)
    before, handle = rec_of(held), held.h.value
    for parts in (across, inside, saturating):
        hs = [upload(engine, r) if MC.ascending(r) else upload_unsorted(engine, r) for r in parts]
        with pytest.raises(S.DeviceError, match="bad argument: bsk_hits_merge: a row names a target twice"):
            engine.merge_hits(hs, [0] * len(hs), reuse=held)
        assert held.h.value == handle and identical(rec_of(held), before)  # the slot is byte for byte what it was
        got, fig = merged(engine, hs, [0] * len(hs), add=True)
        want, wfig = MC.merge_model(parts, None, True)
        assert not SC.same(got, want) and fig == wfig and fig["path"] == "sort" and fig["combined"] > 0
        for h in hs:
            h.close()
    hs = [upload(engine, r) for r in across]
    got, _ = merged(engine, hs, (0, 0), add=True)
    assert int(got["s"][0]) == MC.MAX32 == int(got["total"][0]) and int(got["s"][2]) == 19  # 2^32 - 1 plus 1 saturates
    one = upload_unsorted(engine, inside[1])  # a duplicate inside ONE part under ADD combines too
    got, fig = merged(engine, [one], (0,), add=True)
    assert got["t"].tolist() == [3, 9] and got["s"].tolist() == [21, 42] and got["total"].tolist() == [31, 62] and fig["combined"] == 1
    with pytest.raises(S.DeviceError, match="names a target twice"):
        engine.merge_hits([one], (0,))
    for h in hs + [one, held]:
        h.close()


def test_dot_saturates_across_two_value_shards(engine):
    tg, t_cnt, qs, q_cnt, _, want = W.saturation_case(False)
    Q = engine.sets_from_arrays_counted(qs[0], qs[1], q_cnt)
    whole_ix = engine.sets_from_arrays_counted(tg[0], tg[1], t_cnt).index_counted()
    shards = [engine.sets_from_arrays_counted(c[0], c[1], k) for c, k in MC.value_shards(tg, t_cnt, 2)]
    ixs = [s.index_counted() for s in shards]
    parts = [ix.search_counted(Q, 1) for ix in ixs]
    M = MC.MAX32
    for p in parts:  # target 3 holds the values 1 and 4 with M each, the query too: M * M in either shard
        r = rec_of(p)
        assert int(r["dot"][r["t"].tolist().index(3)]) == M * M
    got, fig = merged(engine, parts, (0, 0), add=True)
    whole = whole_ix.search_counted(Q, 1)
    assert not SC.same(got, rec_of(whole)) and [int(x) for x in got["dot"][:5]] == want["dot"] and [int(x) for x in got["msum"][:5]] == want["min_sum"]
    assert int(got["dot"][3]) == MC.MAX64 and fig["combined"] == 4  # the targets 0, 2, 3 and 4 hold odd and even values
    m = engine.merge_hits(parts, (0, 0), add=True)
    assert np.isnan(m.cosine()[3]) and np.array_equal(np.isnan(m.cosine()), np.isnan(whole.cosine()))
    for x in [whole, m, whole_ix, Q] + parts + ixs + shards:
        x.close()


# ---- 7. limits and refusals: the slot is kept ----
def test_every_refusal_keeps_the_slot(engine):
    parts, bases = MC.row_length_parts(False)
    hs = [upload(engine, r) for r in parts]
    res = engine.merge_hits(hs, bases)
    before = rec_of(res)
    slot = C.c_void_p(res.h.value)
    other = S.Engine(0)
    foreign = other.hits_from_arrays(np.array([0, 1], U64), np.array([0], U32), np.array([1], U32))
    rows3 = upload(engine, SC.record([0, 0, 0, 0], [], []))
    dup = upload(engine, parts[0])
    h3 = [h.h.value for h in hs]
    top = (1 << 32) - 1
    one = upload(engine, SC.record([0, 1] + [1] * (len(parts[0]["o"]) - 2), [1], [1]))  # a target 1: with a base of 2^32 - 1 beyond 32 bits
    bad = [("null part", h3[:2] + [None], bases, 0, L.ERR_ARG), ("no parts", [], (), 0, L.ERR_ARG), ("65 parts", h3[:1] * 65, range(65), 0, L.ERR_ARG),
           ("a flag bit", h3, bases, 2, L.ERR_ARG), ("flag bits", h3, bases, 0x80000001, L.ERR_ARG), ("rows differ", h3[:2] + [rows3.h.value], bases, 0, L.ERR_ARG),
           ("out among the parts", h3[:2] + [res.h.value], bases, 0, L.ERR_ARG), ("a base of 2^32", h3, (0, 1 << 32, 0), 0, L.ERR_ARG),
           ("a base of 2^64 - 1", h3, (0, 0, (1 << 64) - 1), L.MERGE_ADD, L.ERR_ARG), ("duplicate", [h3[0], dup.h.value], (0, 0), 0, L.ERR_ARG),
           ("32-bit overflow", [h3[0], one.h.value], (0, top), 0, L.ERR_UNSUPPORTED), ("32-bit overflow, ADD", [one.h.value], (top,), L.MERGE_ADD, L.ERR_UNSUPPORTED)]
    for what, handles, b, flags, code in bad:
        rc, _ = raw_merge(engine, handles, b, flags, slot)
        assert rc == code and slot.value == res.h.value, what
    fslot = C.c_void_p(foreign.h.value)
    assert raw_merge(engine, h3, bases, 0, fslot)[0] == L.ERR_ARG and fslot.value == foreign.h.value  # *out of another context
    assert b"belongs to another context" in engine.lib.bsk_last_error(engine.ctx)
    assert raw_merge(engine, h3, bases, 0, slot, ctx=None)[0] == L.ERR_ARG and slot.value == res.h.value  # a NULL context
    arr = (C.c_void_p * 3)(*h3)
    assert engine.lib.bsk_hits_merge(engine.ctx, None, None, 3, 0, C.byref(slot)) == L.ERR_ARG and slot.value == res.h.value
    assert engine.lib.bsk_hits_merge(engine.ctx, arr, None, 3, 0, None) == L.ERR_ARG
    assert identical(rec_of(res), before)  # readable and unchanged
    # a base of 2^32 - 1 with a target 0 is the last legal one; and the same calls with nothing wrong go through, into that slot
    zero = upload(engine, SC.record([0, 1], [0], [9]))
    assert merged(engine, [zero], (top,))[0]["t"].tolist() == [top]
    rc, _ = raw_merge(engine, h3, None, L.MERGE_ADD, slot)
    assert rc == L.OK and slot.value == res.h.value and not SC.same(rec_of(res), MC.merge_model(parts, None, True)[0])
    with pytest.raises(ValueError, match="query_sizes"):
        engine.merge_hits([hs[0], rows3])
    with pytest.raises(S.DeviceError, match="bad argument: bsk_hits_merge: the result slot holds one of the parts"):
        engine.merge_hits(hs, bases, reuse=hs[1])
    for x in hs + [res, foreign, rows3, dup, one, zero, other]:
        x.close()


# ---- 8. contexts ----
def test_a_part_of_a_second_context_on_the_same_device(engine):
    for interleaved in (False, True):
        parts, bases = MC.row_length_parts(interleaved)
        want, wfig = MC.merge_model(parts, bases)
        other = S.Engine(0)
        hs = [upload(engine, parts[0]), upload(other, parts[1]), upload(engine, parts[2])]
        got, fig = merged(engine, hs, bases)
        assert not SC.same(got, want) and fig == wfig
        # into a warm object: the pool has its size and so have the result's arrays -- the part is read in place, nothing is copied
        res = engine.merge_hits(hs, bases)
        own = upload(engine, parts[1])
        engine.sync(), other.sync()
        before = free_bytes(0)
        assert engine.merge_hits(hs, bases, reuse=res) is res
        moved = abs(before - free_bytes(0))
        size = sum(x.nbytes for x in want.values() if x is not None)
        assert moved <= size, (moved, size)
        assert not SC.same(rec_of(res), want) and not SC.same(rec_of(hs[1]), parts[1])  # the part is intact
        with pytest.raises(S.DeviceError, match="belongs to another context"):
            engine.merge_hits([hs[0], own, hs[2]], bases, reuse=hs[1])
        for x in hs + [res, own, other]:
            x.close()


def test_a_part_on_a_second_device(engine):
    if n_devices() < 2:
        pytest.skip("one GPU visible: a part on another device needs two")
    far = S.Engine(1)
    for interleaved in (False, True):
        parts, bases = MC.row_length_parts(interleaved)
        hs = [upload(engine, parts[0]), upload(far, parts[1]), upload(far, parts[2])]
        got, fig = merged(engine, hs, bases)
        want, wfig = MC.merge_model(parts, bases)
        assert not SC.same(got, want) and fig == wfig
        assert not SC.same(rec_of(hs[1]), parts[1])
        for x in hs:
            x.close()
    far.close()


# ---- 9. the empties ----
def test_empties(engine):
    for o in (np.zeros(1, U64), np.zeros(5, U64)):  # no queries; queries without hits
        for total in (None, np.zeros(0, U32)):
            hs = [engine.hits_from_arrays(o, np.zeros(0, U32), np.zeros(0, U32), total) for _ in range(3)]
            for add in (False, True):
                got, fig = merged(engine, hs, (0, 5, 5), add)
                assert np.array_equal(got["o"], np.zeros(len(o), U64)) and len(got["t"]) == 0 and (got["total"] is not None) == (total is not None)
                assert fig == dict(path="concat", parts=3, hits=0, combined=0)
            for h in hs:
                h.close()
    # one part with hits among empty ones, in every place
    rec = SC.record([0, 1, 1, 3], [3, 0, 3], [5, 6, 7])
    none = SC.record([0, 0, 0, 0], [], [])
    for place in range(3):
        parts = [none, none, none]
        parts[place] = rec
        hs = [upload(engine, r) for r in parts]
        for bases in ((0, 0, 0), (9, 4, 2)):
            got, fig = merged(engine, hs, bases)
            want, wfig = MC.merge_model(parts, bases)
            assert not SC.same(got, want) and fig == wfig and fig["path"] == "concat"
        for h in hs:
            h.close()


# ---- 10. under a grid cap ----
@pytest.mark.parametrize("interleaved", [False, True])
def test_under_a_grid_cap_the_record_is_the_same(engine, interleaved):
    parts, bases = MC.caps_parts(interleaved)
    hs = [upload(engine, r) for r in parts]
    want, wfig = MC.merge_model(parts, bases)
    assert wfig["hits"] > 3 * 256 * 2 and len(want["o"]) == 601
    for cap in (None,) + GRID_CAPS:
        with switches(engine, dict(BSK_GRID_CAP=None if cap is None else str(cap))):
            s0, c0 = grid_stats(engine)
            res = engine.merge_hits(hs, bases)
            s1, c1 = grid_stats(engine)
        assert s1 - s0 == (11 if interleaved else 7), (cap, s1 - s0)  # check x 3, starts, place x 3; and rows, heads, runs, offsets
        if cap is None:
            assert c1 - c0 == 0, cap
        else:
            assert c1 - c0 >= 6 + (2 if interleaved else 0), (cap, c1 - c0)  # the grids over the hits were cut
        assert not SC.same(rec_of(res), want) and figures(res) == wfig, cap
        res.close()
    for h in hs:
        h.close()
