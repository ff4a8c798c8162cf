"""GPU: the counted set algebra (bsk_sets_op_counted; setops.hip), bsk_sets_filter_counts and bsk_sets_totals (counts.hip) against NumPy on
host arrays -- every offset, value and count.

The pairs are those of tests/setops_cases.py; counts are attached so that a wrong partner shows (ca = 1 + rank % 7, cb = 1000 (1 + rank % 5):
every sum names both ranks).  Before comparing, every call's pairs per path (bsk_sets_plan) are asserted against NumPy's count of t."""
import ctypes as C
import functools

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import counts_cases as CC
from tests import sets_cases as SC
from tests import setops_cases as SO
from tests.setops_cases import collection

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
CAPS = SO.read_caps()
GROUP_CAP, WAVE_CAP, TILE = CAPS["SO_GROUP_CAP"], CAPS["SO_WAVE_CAP"], CAPS["SO_TILE"]


@functools.lru_cache(None)
def cus():
    hip = C.CDLL("libamdhip64.so")
    hip.hipDeviceGetAttribute.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
    v = C.c_int()
    assert hip.hipDeviceGetAttribute(C.byref(v), 63, 0) == 0 and v.value > 0  # hipDeviceAttributeMultiprocessorCount
    return v.value


def load(engine, s):
    return engine.sets_from_arrays(s[0], s[1]) if s[2] is None else engine.sets_from_arrays_counted(*s)


def fetch3(sets):
    o, v = sets.fetch()
    return o, v, sets.fetch_counts()


def same(sets, want, what=""):
    assert sets.counted, what
    for name, g, w in zip(("offsets", "values", "counts"), fetch3(sets), want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, what)
    assert np.array_equal(sets.totals(), CC.ref_totals(want)), ("totals", what)


def check_ops(engine, a, b, what="", paths=None, ops=CC.OPS, same_object=False, into=None, counts=("a", "b")):
    """a op b on the device for ADD / KEEP / DROP: the paths as NumPy counts them, then offsets, values and counts"""
    a, b = CC.with_counts(a, counts[0]), CC.with_counts(a if same_object else b, counts[0] if same_object else counts[1])
    A = load(engine, a)
    B = A if same_object else load(engine, b)
    assert A.counted == (counts[0] is not None)
    counted = CC.path_counts(a[0], b[0], CAPS)
    if paths is not None:
        assert counted == paths, (what, counted, paths)
    for op in ops:
        R = A.op_counted(B, op, into)
        assert R.plan()["n_by_path"] == counted and "bsk_sets_op_counted" in R.plan()["plan"], (what, op, R.plan(), counted)
        same(R, CC.ref_op(a, b, op), (what, op))
        if into is None:
            R.close()
    A.close()
    if not same_object:
        B.close()


# ---- all three ops over the pairs of the uncounted algebra ----
def test_degenerate_pairs(engine):
    d = SO.degenerate_pairs()
    for name, (a, b) in d.items():
        check_ops(engine, collection([a]), collection([b]), name, paths=[1, 0, 0])
    a, b = collection([x for x, _ in d.values()]), collection([y for _, y in d.values()])
    check_ops(engine, a, b, "all degenerate pairs", paths=[len(d), 0, 0])
    e = (np.zeros(1, U64), np.zeros(0, U64))
    check_ops(engine, e, e, "zero sets", paths=[0, 0, 0])


@pytest.mark.parametrize("cap", [GROUP_CAP, WAVE_CAP])
def test_class_edges(engine, cap):
    for a, b, t, na in SO.class_edges(cap, np.random.default_rng(cap)):
        want = [1, 0, 0] if t <= GROUP_CAP else [0, 1, 0] if t <= WAVE_CAP else [0, 0, 1]
        check_ops(engine, collection([a]), collection([b]), (t, na), paths=want)


def test_all_three_classes_in_one_call_shuffled(engine):
    rng = np.random.default_rng(11)
    pairs = [(a, b) for cap in (GROUP_CAP, WAVE_CAP) for a, b, _, _ in SO.class_edges(cap, rng)]
    pairs += [SO.pair(t, t // 3, rng) for t in (0, 1, 2, 17, 3 * TILE + 5, 2 * TILE, 5 * TILE + 1)]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    a, b = collection([x for x, _ in pairs]), collection([y for _, y in pairs])
    counted = CC.path_counts(a[0], b[0], CAPS)
    assert min(counted) >= 5
    check_ops(engine, a, b, "mixed classes", paths=counted)


# ---- tiles ----
def test_tile_boundaries(engine):
    """a shared value's two copies in two tiles: a's copy, the last rank of its tile, takes its partner's count from behind the b slice"""
    for name, (a, b, at) in SO.tile_cases(TILE, np.random.default_rng(13)).items():
        check_ops(engine, collection([a]), collection([b]), name, paths=[0, 0, 1])
        check_ops(engine, collection([b]), collection([a]), name + " (swapped)", paths=[0, 0, 1])
    a, _ = SO.pair(3 * TILE + 6, (3 * TILE + 6) // 2, np.random.default_rng(14), shared=0)
    check_ops(engine, collection([a]), collection([a.copy()]), "every value shared", paths=[0, 0, 1])


def test_more_tiles_than_one_pass(engine):
    per_pass = cus() * CAPS["SO_TILE_BLOCKS_PER_CU"] * CAPS["SO_WAVES"]
    t = (per_pass + per_pass // 4 + 1) * TILE + 7
    a, b = SO.pair(t, t // 2 + 3, np.random.default_rng(17), shared=t // 4)
    assert (len(a) + len(b) + TILE - 1) // TILE > per_pass
    check_ops(engine, collection([a]), collection([b]), "one large pair", paths=[0, 0, 1])


# ---- counts ----
def test_saturation(engine):
    a, b, sums = CC.saturation_pairs()
    A, B = load(engine, a), load(engine, b)
    R = A.add(B)
    want = CC.ref_op(a, b, CC.ADD)
    same(R, want, "saturation")
    assert [list(x) for x in SO.split(want[0], want[2])] == sums and sums[2] == [2**32 - 1] and int(a[2][2]) + int(b[2][2]) == 2**32 - 1
    t = R.totals()
    assert int(t[3]) == 2 * (2**32 - 1)  # totals do not saturate


@pytest.mark.parametrize("counts", [(None, "b"), ("a", None), (None, None)])
def test_uncounted_operands_count_one(engine, counts):
    rng = np.random.default_rng(19)
    pairs = [SO.pair(t, t // 2, rng) for t in (10, 50, 300, 2 * TILE + 9)]
    a, b = collection([x for x, _ in pairs]), collection([y for _, y in pairs])
    check_ops(engine, a, b, counts, paths=[2, 1, 1], counts=counts)


@pytest.mark.parametrize("t", [40, WAVE_CAP - 24, 2 * TILE + 100])
def test_a_op_a_as_the_same_object(engine, t):
    a, _ = SO.pair(t, t // 2, np.random.default_rng(t))
    a = collection([a, a[: len(a) // 3]])
    check_ops(engine, a, a, "a op a", same_object=True)
    A = load(engine, CC.with_counts(a, "a"))
    o, v, c = fetch3(A.add(A))
    assert np.array_equal(c, 2 * CC.counts_a(a[0])) and np.array_equal(v, a[1])
    same(A.keep(A), CC.with_counts(a, "a"), "KEEP is a")
    assert A.drop(A).info() == dict(n_sets=2, n_values=0)


# ---- broadcast ----
def test_broadcast_of_b(engine):
    rng = np.random.default_rng(29)
    big = np.unique(rng.integers(0, 1 << 20, size=6000, dtype=U64))[:5000]
    small = [np.unique(np.concatenate([rng.choice(big, size=int(rng.integers(0, 9))), rng.integers(0, 1 << 20, size=int(rng.integers(0, 9)), dtype=U64)]))
             for _ in range(300)]
    check_ops(engine, collection(small), collection([big]), "b broadcast", paths=[0, 0, 300])


def test_broadcast_of_a(engine):
    """one sample against every genome: a of one set against 1 000 small sets, and against sets on the tiled path"""
    rng = np.random.default_rng(31)
    sample = np.unique(rng.integers(0, 1 << 12, size=30, dtype=U64))
    small = [np.unique(rng.integers(0, 1 << 12, size=int(rng.integers(0, 30)), dtype=U64)) for _ in range(1000)]
    assert len(sample) + max(len(s) for s in small) <= GROUP_CAP
    check_ops(engine, collection([sample]), collection(small), "a against 1000", paths=[1000, 0, 0])
    big = np.unique(rng.integers(0, 1 << 16, size=3000, dtype=U64))
    targets = [np.unique(rng.integers(0, 1 << 16, size=n, dtype=U64)) for n in (0, 5, 2000, 1, 4000)]
    check_ops(engine, collection([big]), collection(targets), "a against tiled", paths=[0, 0, 5])
    check_ops(engine, collection([big[:40]]), collection(targets), "a against mixed", paths=[3, 0, 2])
    check_ops(engine, collection([np.zeros(0, U64)]), collection(targets), "an empty a", paths=[3, 0, 2])
    check_ops(engine, collection(targets), collection([np.zeros(0, U64)]), "an empty b", paths=[3, 0, 2])
    check_ops(engine, collection([big[:7]]), collection([big[3:90]]), "one against one", paths=[0, 1, 0])


def test_refused_pairings(engine):
    three = engine.sets_from_arrays(*collection([[1], [2], [3]]))
    two = engine.sets_from_arrays(*collection([[1], [2]]))
    one = engine.sets_from_arrays(*collection([[1]]))
    none = engine.sets_from_arrays(np.zeros(1, U64), np.zeros(0, U64))
    for a, b in ((three, two), (two, three), (three, none), (none, two)):
        out = C.c_void_p()
        assert engine.lib.bsk_sets_op_counted(engine.ctx, a.h, b.h, L.COUNTOP_ADD, C.byref(out)) == L.ERR_ARG and not out.value
    out = C.c_void_p()
    assert engine.lib.bsk_sets_op(engine.ctx, one.h, three.h, L.SETOP_UNION, C.byref(out)) == L.ERR_ARG and not out.value  # bsk_sets_op keeps refusing it
    assert one.add(three).info()["n_sets"] == 3 and three.add(one).info()["n_sets"] == 3
    assert none.add(one).info()["n_sets"] == 0 and one.add(none).info()["n_sets"] == 0


# ---- *out ----
def test_out_reused_across_the_entries(engine):
    rng = np.random.default_rng(37)
    large = [collection([x]) for x in SO.pair(6 * TILE + 3, 3 * TILE, rng)]
    small = [collection([x]) for x in SO.pair(9, 4, rng)]
    into = S.Sets(engine, None)
    for a, b in (large, small, large):
        check_ops(engine, a, b, "reused", into=into)
    A, B = load(engine, CC.with_counts(large[0], "a")), load(engine, CC.with_counts(large[1], "b"))
    assert A.union(B, into=into) is into and not into.counted  # bsk_sets_op leaves it uncounted
    o, v = into.fetch()
    assert np.array_equal(v, np.union1d(large[0][1], large[1][1]))
    cnt = np.zeros(4, U32)
    assert engine.lib.bsk_sets_fetch_counts(engine.ctx, into.h, 0, 1, cnt.ctypes.data, 4) == L.ERR_ARG
    added = A.add(B)
    assert added.filter_counts(1000, into=into) is into and into.counted
    same(into, CC.ref_filter(fetch3(added), 1000, 2**32 - 1), "filter into an op's object")
    assert A.reduce(np.array([0, 1], U64), into=into) is into and not into.counted  # and so does bsk_sets_reduce
    assert A.keep(B, into=into) is into
    same(into, CC.ref_op(CC.with_counts(large[0], "a"), CC.with_counts(large[1], "b"), CC.KEEP), "after a reduce")


def test_argument_errors_leave_out_untouched(engine):
    a = engine.sets_from_arrays_counted(*collection([[1, 2, 3], [4]]), np.array([1, 2, 3, 4], U32))
    b = engine.sets_from_arrays(*collection([[2, 3], [4, 5]]))
    out = a.add(b)
    want = fetch3(out)
    other = S.Engine(0)
    foreign = other.sets_from_arrays(*collection([[1], [2]]))
    lib, ctx = engine.lib, engine.ctx
    slot = C.c_void_p(out.h.value)
    for x, y, o, s in ((a.h, b.h, 3, slot), (a.h, b.h, -1, slot), (foreign.h, b.h, 0, slot), (a.h, foreign.h, 0, slot), (a.h, None, 0, slot), (None, b.h, 0, slot),
                       (a.h, b.h, 0, C.c_void_p(a.h.value)), (a.h, b.h, 0, C.c_void_p(b.h.value)), (a.h, b.h, 0, C.c_void_p(foreign.h.value))):
        before = s.value
        assert lib.bsk_sets_op_counted(ctx, x, y, o, C.byref(s)) == L.ERR_ARG and s.value == before, (o,)
    assert lib.bsk_sets_op_counted(ctx, a.h, b.h, 0, None) == L.ERR_ARG
    for x, lo, hi, s in ((a.h, 0, 5, slot), (a.h, 3, 2, slot), (b.h, 1, 5, slot), (foreign.h, 1, 5, slot), (None, 1, 5, slot), (a.h, 1, 5, C.c_void_p(a.h.value))):
        before = s.value
        assert lib.bsk_sets_filter_counts(ctx, x, lo, hi, C.byref(s)) == L.ERR_ARG and s.value == before, (lo, hi)
    assert lib.bsk_sets_filter_counts(ctx, a.h, 1, 5, None) == L.ERR_ARG
    t = np.zeros(4, U64)
    assert lib.bsk_sets_totals(ctx, foreign.h, 0, 1, t.ctypes.data) == L.ERR_ARG and lib.bsk_sets_totals(ctx, a.h, 0, 2, None) == L.ERR_ARG
    for n, (g, w) in enumerate(zip(fetch3(out), want)):
        assert np.array_equal(g, w), n
    # host-loaded counts: a count of 0 is refused and nothing is kept
    o, v = collection([[1, 2, 3], [4]])
    h = C.c_void_p(77)
    bad = np.array([1, 0, 3, 4], U32)
    assert lib.bsk_sets_from_host_counted(ctx, o.ctypes.data, 2, v.ctypes.data, bad.ctypes.data, C.byref(h)) == L.ERR_ARG and h.value is None
    assert lib.bsk_sets_from_host_counted(ctx, o.ctypes.data, 2, v.ctypes.data, None, C.byref(h)) == L.ERR_ARG and h.value is None
    v2 = np.array([1, 3, 2, 4], U64)
    assert lib.bsk_sets_from_host_counted(ctx, o.ctypes.data, 2, v2.ctypes.data, bad.ctypes.data, C.byref(h)) == L.ERR_ARG and h.value is None
    foreign.close()
    other.close()


# ---- filter ----
def test_filter_counts(engine):
    s, lo, hi = CC.filter_sets(SC.SCAN_CHUNK)
    S_ = load(engine, s)
    want = CC.ref_filter(s, lo, hi)
    sizes = np.diff(want[0].astype(np.int64))
    assert sizes[0] == sizes[3] == sizes[-1] == 0 and sizes[2] > 0 and sizes[4] > 0 and len(s[1]) > SC.SCAN_CHUNK
    assert lo in want[2] and hi in want[2] and want[2].min() == lo and want[2].max() == hi
    same(S_.filter_counts(lo, hi), want, "bounds")
    same(S_.filter_counts(), s, "all kept")
    same(S_.filter_counts(1, 2**32 - 1), s, "all kept, explicit")
    same(S_.filter_counts(13), CC.ref_filter(s, 13, 2**32 - 1), "none kept")
    assert len(CC.ref_filter(s, 13, 2**32 - 1)[1]) == 0
    same(S_.filter_counts(lo, lo), CC.ref_filter(s, lo, lo), "one count")
    plain = engine.sets_from_arrays(s[0], s[1])
    with pytest.raises(S.DeviceError):
        plain.filter_counts(1)
    none = engine.sets_from_arrays_counted(np.zeros(3, U64), np.zeros(0, U64), np.zeros(0, U32))
    same(none.filter_counts(2), (np.zeros(3, U64), np.zeros(0, U64), np.zeros(0, U32)), "no values")


# ---- totals ----
def test_totals(engine):
    offs, vals = collection([[], [1, 2, 3], [], [5, 6, 7], [9], []])
    c = np.array([4, 5, 6, 2**32 - 1, 2**32 - 1, 2**32 - 1, 7], U32)
    s = engine.sets_from_arrays_counted(offs, vals, c)
    assert [int(x) for x in s.totals()] == [0, 15, 0, 3 * (2**32 - 1), 7, 0]
    t = np.full(3, 99, U64)
    assert engine.lib.bsk_sets_totals(engine.ctx, s.h, 2, 2, t.ctypes.data) == L.OK and [int(x) for x in t] == [0, 3 * (2**32 - 1), 99]
    assert engine.lib.bsk_sets_totals(engine.ctx, s.h, 6, 0, t.ctypes.data) == L.OK and engine.lib.bsk_sets_totals(engine.ctx, s.h, 6, 1, t.ctypes.data) == L.ERR_ARG
    plain = engine.sets_from_arrays(offs, vals)
    assert [int(x) for x in plain.totals()] == [0, 3, 0, 3, 1, 0]


# ---- end to end: a gather ----
def test_gather_of_a_sample_against_three_genomes(engine, oracle):
    g = CC.gather_case()
    pk, scale = g["pk"], g["scale"]
    p = engine.params(L.MINIMIZER, pk["k"], w=pk["w"])

    def oracle_values(seqs):
        return [np.asarray(SC.oracle_values(oracle, "minimizer", pk, s), U64) for s in seqs]

    batches = [engine.batch(b) for b in g["batches"] + [g["batches"][0] + g["batches"][1], g["genomes"]]]
    results = [engine.run(b, p) for b in batches]
    parts = [r.counted_sets(whole_batch=True, scale=scale) for r in results[:2]]
    sample = parts[0].add(parts[1])
    once = results[2].counted_sets(whole_batch=True, scale=scale)
    want = CC.ref_counted(oracle_values(g["batches"][0] + g["batches"][1]), scale, True)
    same(once, want, "all reads in one call")
    same(sample, want, "two batches added")
    assert want[2].max() >= 3 and len(want[1]) > 300
    gv = oracle_values(g["genomes"])
    gsets = SC.ref_sets(gv, scale, False)
    genomes = results[3].device_sets(scale=scale)
    assert np.array_equal(genomes.fetch()[1], gsets[1])
    # weighted containment of the sample in every genome: the sample broadcast, KEEP, totals
    kept = sample.keep(genomes)
    assert kept.info()["n_sets"] == 3
    want_kept = CC.ref_op(want, (gsets[0], gsets[1], None), CC.KEEP)
    same(kept, want_kept, "KEEP(sample, genomes)")
    total = int(want[2].astype(U64).sum())
    weighted = kept.totals().astype(np.float64) / total
    ref_w = np.array([int(want[2][np.isin(want[1], x)].astype(U64).sum()) for x in SO.split(*gsets)], np.float64) / total
    assert np.array_equal(weighted, ref_w) and weighted[0] > weighted[1] > weighted[2] == 0.0 and int(sample.totals()[0]) == total
    # subtract the best genome, then drop the values seen once
    best = int(np.argmax(weighted))
    best_set = engine.sets_from_arrays(*collection([SO.split(*gsets)[best]]))
    rest = sample.drop(best_set)
    want_rest = CC.ref_op(want, (*collection([SO.split(*gsets)[best]]), None), CC.DROP)
    same(rest, want_rest, "DROP of the best genome")
    solid = rest.filter_counts(min_count=2)
    same(solid, CC.ref_filter(want_rest, 2, 2**32 - 1), "seen at least twice")
    assert 0 < solid.info()["n_values"] < rest.info()["n_values"] < sample.info()["n_values"]
