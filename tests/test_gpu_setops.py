"""GPU: bsk_sets_op / bsk_sets_reduce (bio_amd/csrc/setops.hip) against NumPy, exactly -- every offset and every value.

Every test first asserts from bsk_sets_plan that the pairs took the paths NumPy counts for them (t = |a_i| + |b_i| against the caps read
from setops.hip), then compares with np.union1d / np.intersect1d / np.setdiff1d / np.setxor1d per pair, and for reduce with np.unique's
counts against the threshold (tests/setops_cases.py; its claims are re-derived in tests/test_setops_cases.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import setops_cases as SC
from tests.search_cases import ref_search
from tests.setops_cases import collection

pytestmark = pytest.mark.gpu
U64 = np.uint64
CAPS = SC.read_caps()
GROUP_CAP, WAVE_CAP, TILE = CAPS["SO_GROUP_CAP"], CAPS["SO_WAVE_CAP"], CAPS["SO_TILE"]


@functools.lru_cache(None)
def cus():
    hip = C.CDLL("libamdhip64.so")
    hip.hipDeviceGetAttribute.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
    v = C.c_int()
    assert hip.hipDeviceGetAttribute(C.byref(v), 63, 0) == 0 and v.value > 0  # hipDeviceAttributeMultiprocessorCount
    return v.value


def same(sets, want, what=""):
    o, v = sets.fetch()
    assert np.array_equal(o, want[0]), ("offsets", what)
    assert np.array_equal(v, want[1]), ("values", what)


def check_ops(engine, a, b, what="", paths=None, ops=SC.OPS, want=None, same_object=False, into=None):
    """a op b on the device for every op: the paths as NumPy counts them, then every offset and value"""
    A = engine.sets_from_arrays(*a)
    B = A if same_object else engine.sets_from_arrays(*b)
    counted = SC.path_counts(a[0], b[0], CAPS)
    if paths is not None:
        assert counted == paths, (what, counted, paths)
    for op in ops:
        R = A.op(B, op, into)
        assert R.plan()["n_by_path"] == counted, (what, op, R.plan(), counted)
        same(R, want(op) if want else SC.ref_op(a, b, op), (what, op))
        if into is None:
            R.close()
    A.close()
    if not same_object:
        B.close()


# ---- degenerate pairs ----
def test_degenerate_pairs(engine):
    d = SC.degenerate_pairs()
    for name, (a, b) in d.items():  # one pair per call ...
        check_ops(engine, collection([a]), collection([b]), name, paths=[1, 0, 0])
    a, b = collection([x for x, _ in d.values()]), collection([y for _, y in d.values()])  # ... and all of them in one
    check_ops(engine, a, b, "all degenerate pairs", paths=[len(d), 0, 0])


def test_no_pairs_at_all(engine):
    e = (np.zeros(1, U64), np.zeros(0, U64))
    check_ops(engine, e, e, "zero sets", paths=[0, 0, 0])


@pytest.mark.parametrize("t", [40, WAVE_CAP - 24, 2 * TILE + 100])
def test_a_op_a_as_the_same_object(engine, t):
    a, _ = SC.pair(t, t // 2, np.random.default_rng(t))
    a = collection([a, a[: len(a) // 3]])
    check_ops(engine, a, a, "a op a", same_object=True)


# ---- class edges ----
@pytest.mark.parametrize("cap", [GROUP_CAP, WAVE_CAP])
def test_class_edges(engine, cap):
    for a, b, t, na in SC.class_edges(cap, np.random.default_rng(cap)):
        want = [1, 0, 0] if t <= GROUP_CAP else [0, 1, 0] if t <= WAVE_CAP else [0, 0, 1]
        check_ops(engine, collection([a]), collection([b]), (t, na), paths=want)


def test_all_three_classes_in_one_call_shuffled(engine):
    rng = np.random.default_rng(11)
    pairs = [(a, b) for cap in (GROUP_CAP, WAVE_CAP) for a, b, _, _ in SC.class_edges(cap, rng)]
    pairs += [SC.pair(t, t // 3, rng) for t in (0, 1, 2, 17, 3 * TILE + 5, 2 * TILE, 5 * TILE + 1)]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    a, b = collection([x for x, _ in pairs]), collection([y for _, y in pairs])
    counted = SC.path_counts(a[0], b[0], CAPS)
    assert min(counted) >= 5
    check_ops(engine, a, b, "mixed classes", paths=counted)


# ---- tile boundaries ----
def test_tile_boundaries(engine):
    for name, (a, b, at) in SC.tile_cases(TILE, np.random.default_rng(13)).items():
        check_ops(engine, collection([a]), collection([b]), name, paths=[0, 0, 1])
        check_ops(engine, collection([b]), collection([a]), name + " (swapped)", paths=[0, 0, 1])  # then b's copy comes first
    a, _ = SC.pair(3 * TILE + 6, (3 * TILE + 6) // 2, np.random.default_rng(14), shared=0)
    check_ops(engine, collection([a]), collection([a.copy()]), "every value shared", paths=[0, 0, 1])


# ---- spread: beyond one pass of every capped grid ----
def test_one_pair_beyond_one_pass_of_the_tile_grid(engine):
    per_pass = cus() * CAPS["SO_TILE_BLOCKS_PER_CU"] * CAPS["SO_WAVES"]  # tiles one pass of k_so_tile's grid covers
    t = (per_pass + per_pass // 4 + 1) * TILE + 7
    a, b = SC.pair(t, t // 2 + 3, np.random.default_rng(17), shared=t // 4)
    assert (len(a) + len(b) + TILE - 1) // TILE > per_pass
    check_ops(engine, collection([a]), collection([b]), "one large pair", paths=[0, 0, 1])


def test_group_pairs_beyond_one_pass(engine):
    n = cus() * CAPS["SO_GROUP_BLOCKS_PER_CU"] * 16 + 9
    a, b, base, shift = SC.shifted_pairs(n, 0, 12, np.random.default_rng(19))
    assert n == cus() * 512 + 9 or CAPS["SO_GROUP_BLOCKS_PER_CU"] != 32
    check_ops(engine, a, b, "group pairs", paths=[n, 0, 0], want=lambda op: SC.ref_shifted(base, shift, op))


def test_wave_pairs_beyond_one_pass(engine):
    n = cus() * CAPS["SO_WAVE_BLOCKS_PER_CU"] * CAPS["SO_WAVES"] + 3
    a, b, base, shift = SC.shifted_pairs(n, GROUP_CAP + 1, GROUP_CAP + 40, np.random.default_rng(23), n_base=61)
    assert n == cus() * 64 + 3 or CAPS["SO_WAVE_BLOCKS_PER_CU"] * CAPS["SO_WAVES"] != 64
    check_ops(engine, a, b, "wave pairs", paths=[0, n, 0], want=lambda op: SC.ref_shifted(base, shift, op))


# ---- broadcast ----
def test_broadcast_of_one_large_set(engine):
    rng = np.random.default_rng(29)
    big = np.unique(rng.integers(0, 1 << 20, size=6000, dtype=U64))[:5000]
    assert len(big) == 5000
    small = [np.unique(np.concatenate([rng.choice(big, size=int(rng.integers(0, 9))), rng.integers(0, 1 << 20, size=int(rng.integers(0, 9)), dtype=U64)]))
             for _ in range(1000)]
    assert max(len(s) for s in small) <= GROUP_CAP  # group-class a sets ...
    check_ops(engine, collection(small), collection([big]), "broadcast", paths=[0, 0, 1000])  # ... on the tiled path


def test_broadcast_of_an_empty_set_and_onto_one_set(engine):
    rng = np.random.default_rng(31)
    sets = [np.unique(rng.integers(0, 1 << 30, size=n, dtype=U64)) for n in (0, 5, 70, 1500)]
    check_ops(engine, collection(sets), collection([np.zeros(0, U64)]), "empty broadcast", paths=[2, 1, 1])
    check_ops(engine, collection(sets[2:3]), collection(sets[1:2]), "one against one", paths=[0, 1, 0])


def test_pairings_that_are_argument_errors(engine):
    three = engine.sets_from_arrays(*collection([[1], [2], [3]]))
    two = engine.sets_from_arrays(*collection([[1], [2]]))
    one = engine.sets_from_arrays(*collection([[1]]))
    none = engine.sets_from_arrays(np.zeros(1, U64), np.zeros(0, U64))
    for a, b in ((three, two), (one, three), (three, none), (one, none)):
        out = C.c_void_p()
        assert engine.lib.bsk_sets_op(engine.ctx, a.h, b.h, L.SETOP_UNION, C.byref(out)) == L.ERR_ARG and not out.value
    same(none.union(one), (np.zeros(1, U64), np.zeros(0, U64)), "no sets against one set: broadcast over nothing")


# ---- object rules ----
def test_out_reused_large_small_large(engine):
    rng = np.random.default_rng(37)
    large = [collection([x]) for x in SC.pair(6 * TILE + 3, 3 * TILE, rng)]
    small = [collection([x]) for x in SC.pair(9, 4, rng)]
    many = [collection(list(x)) for x in zip(*[SC.pair(int(t), int(t) // 2, rng) for t in rng.integers(0, 200, size=300)])]
    into = S.Sets(engine, None)
    for a, b in (large, small, many, large, small):
        check_ops(engine, a, b, "reused", into=into)
    (offs, vals), go = SC.reduce_groups(rng)
    s = engine.sets_from_arrays(offs, vals)
    assert s.reduce(go, 2, into=into) is into  # an op's object takes a reduce, and the other way round
    same(into, SC.ref_reduce((offs, vals), go, 2))
    assert into.plan()["n_by_path"] == [0, 0, 0] and "reduce" in into.plan()["plan"]
    check_ops(engine, *small, "after a reduce", into=into)
    fresh = engine.sets_from_arrays(offs, vals)
    assert fresh.plan() == dict(plan="", n_by_path=[0, 0, 0])  # sets of any other origin


def test_argument_errors_leave_out_untouched(engine):
    a = engine.sets_from_arrays(*collection([[1, 2, 3], [4]]))
    b = engine.sets_from_arrays(*collection([[2, 3], [4, 5]]))
    go = np.array([0, 2], U64)
    out = a.union(b)
    want = SC.ref_op(*[collection(x) for x in ([[1, 2, 3], [4]], [[2, 3], [4, 5]])], SC.UNION)
    other = S.Engine(0)
    foreign = other.sets_from_arrays(*collection([[1], [2]]))
    lib, ctx = engine.lib, engine.ctx

    def op(x, y, o, slot):
        return lib.bsk_sets_op(ctx, x, y, o, C.byref(slot))

    slot = C.c_void_p(out.h.value)
    for x, y, o, s in ((a.h, b.h, 4, slot), (a.h, b.h, -1, slot), (foreign.h, b.h, 0, slot), (a.h, foreign.h, 0, slot), (a.h, None, 0, slot),
                       (a.h, b.h, 0, C.c_void_p(a.h.value)), (a.h, b.h, 0, C.c_void_p(b.h.value)), (a.h, b.h, 0, C.c_void_p(foreign.h.value))):
        before = s.value
        assert op(x, y, o, s) == L.ERR_ARG and s.value == before, (o,)
    assert lib.bsk_sets_op(ctx, a.h, b.h, 0, None) == L.ERR_ARG
    gp = go.ctypes.data
    for x, g, ng, m, s in ((a.h, gp, 1, 0, slot), (foreign.h, gp, 1, 1, slot), (a.h, None, 1, 1, slot), (a.h, gp, 1, 1, C.c_void_p(a.h.value))):
        before = s.value
        assert lib.bsk_sets_reduce(ctx, x, g, ng, m, C.byref(s)) == L.ERR_ARG and s.value == before, (ng, m)
    same(out, want, "the object every refused call was given")
    same(a, collection([[1, 2, 3], [4]]), "a")
    foreign.close()
    other.close()


# ---- reduce ----
@pytest.mark.parametrize("m", [1, 2, 3, 63, 64, 65, SC.MEMBERS_ALL])
def test_reduce_groups(engine, m):
    (offs, vals), go = SC.reduce_groups(np.random.default_rng(7))
    r = engine.sets_from_arrays(offs, vals).reduce(go, m)
    assert r.info()["n_sets"] == len(go) - 1
    same(r, SC.ref_reduce((offs, vals), go, m), m)


def test_reduce_run_across_a_group_border(engine):
    s = collection([[1, 5, 1000], [1000, 2000], [1000, 3000], [3000], [3000]])
    S_ = engine.sets_from_arrays(*s)
    for go in ([0, 1, 3, 4, 5], [0, 1, 2, 3, 5], [0, 2, 5], [0, 0, 1, 1, 2, 5, 5]):
        go = np.array(go, U64)
        for m in (1, 2, 3, SC.MEMBERS_ALL):
            same(S_.reduce(go, m), SC.ref_reduce(s, go, m), (go.tolist(), m))


def test_reduce_bad_group_offsets(engine):
    s = engine.sets_from_arrays(*collection([[1], [2], [3]]))
    out = s.reduce(np.array([0, 3], U64))
    slot = C.c_void_p(out.h.value)
    for go in ([1, 3], [0, 2, 1, 3], [0, 2], [0, 4], [0, 3, 2]):
        go = np.array(go, U64)
        assert engine.lib.bsk_sets_reduce(engine.ctx, s.h, go.ctypes.data, len(go) - 1, 1, C.byref(slot)) == L.ERR_ARG and slot.value == out.h.value, go
    same(out, collection([[1, 2, 3]]))
    with pytest.raises(S.DeviceError):
        s.reduce(np.array([0, 2], U64))
    same(s.reduce(np.array([0, 0, 3, 3], U64), 1), collection([[], [1, 2, 3], []]))


def test_reduce_without_groups_or_values(engine):
    none = engine.sets_from_arrays(np.zeros(1, U64), np.zeros(0, U64))
    same(none.reduce(np.zeros(1, U64)), (np.zeros(1, U64), np.zeros(0, U64)))
    empty = engine.sets_from_arrays(np.zeros(4, U64), np.zeros(0, U64))
    same(empty.reduce(np.array([0, 1, 3], U64), SC.MEMBERS_ALL), (np.zeros(3, U64), np.zeros(0, U64)))


@functools.lru_cache(None)
def many_small_sets(every_set_holds_zero):
    """200 000 sets of up to 6 values below 350 000, ascending by construction (running sums of positive steps inside a set)"""
    rng = np.random.default_rng(41)
    n = 200_000
    sizes = rng.integers(1 if every_set_holds_zero else 0, 7, size=n)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum(sizes)
    step = rng.integers(1, 50_000, size=int(offs[-1]))
    run = np.cumsum(step)
    first = np.repeat(offs[:-1], sizes)
    vals = run - np.repeat((run - step)[offs[:-1][sizes > 0]], sizes[sizes > 0])  # the running sum restarts with every set
    if every_set_holds_zero:
        vals = vals - step[first]  # a set's first value becomes 0
    return offs.astype(U64), vals.astype(U64)


@pytest.mark.parametrize("m", [1, 2, SC.MEMBERS_ALL])
def test_reduce_one_group_of_200000_sets(engine, m):
    s = many_small_sets(m == SC.MEMBERS_ALL)
    n = len(s[0]) - 1
    go = np.array([0, n], U64)
    want = SC.ref_reduce(s, go, m)
    assert len(want[1]) >= (1 if m == SC.MEMBERS_ALL else 1000)
    same(engine.sets_from_arrays(*s).reduce(go, m), want, m)


# ---- what it is for, end to end ----
@pytest.fixture(scope="module")
def genomes(engine):
    """three genomes of 2, 3 and 4 contigs, 2 000 reads of 150 bases cut from them; the contigs' and the reads' minimizer sets"""
    rng = np.random.default_rng(43)
    contigs = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(rng.integers(2500, 4000)))) for _ in range(9)]
    go = np.array([0, 2, 5, 9], U64)
    reads = []
    for _ in range(2000):
        c = contigs[int(rng.integers(0, 9))]
        at = int(rng.integers(0, len(c) - 150))
        reads.append(c[at:at + 150])
    p = engine.params(L.MINIMIZER, 21, w=11)
    cb, rb = engine.batch(contigs), engine.batch(reads)
    csets = engine.run(cb, p).device_sets()
    rsets = engine.run(rb, p).device_sets()
    return dict(go=go, csets=csets, rsets=rsets, c=csets.fetch(), r=rsets.fetch())


def hits_equal(hits, want):
    o, t, s = hits.fetch()
    assert np.array_equal(o, want[0]) and np.array_equal(t, want[1]) and np.array_equal(s, want[2])


def test_multi_contig_genomes_as_targets(engine, genomes):
    g = genomes
    targets = g["csets"].reduce(g["go"])
    tg = SC.ref_reduce(g["c"], g["go"], 1)
    same(targets, tg, "genome sets")
    assert targets.info()["n_sets"] == 3 and len(tg[1]) > 3000
    want = ref_search(*tg, *g["r"], 1, 0.5, 0.0)
    hits = targets.index().search(g["rsets"], min_query_cov=0.5)
    hits_equal(hits, want)
    assert int(want[0][-1]) >= 2000 and np.all(np.diff(want[0].astype(np.int64)) >= 1)  # every read finds its genome


def test_read_pairs_as_queries(engine, genomes):
    g = genomes
    pairs_go = np.arange(0, 2001, 2, dtype=U64)
    queries = g["rsets"].reduce(pairs_go)
    q = SC.ref_reduce(g["r"], pairs_go, 1)
    same(queries, q, "pair sets")
    tg = SC.ref_reduce(g["c"], g["go"], 1)
    ix = engine.sets_from_arrays(*tg).index()
    hits_equal(ix.search(queries), ref_search(*tg, *q))
    both = g["rsets"].reduce(pairs_go, SC.MEMBERS_ALL)  # what both mates hold
    same(both, SC.ref_reduce(g["r"], pairs_go, SC.MEMBERS_ALL), "pair intersections")


def test_masking_a_genome_out_of_the_reads(engine, genomes):
    g = genomes
    host = SC.collection([SC.split(*SC.ref_reduce(g["c"], g["go"], 1))[1]])
    mask = engine.sets_from_arrays(*host)
    masked = g["rsets"].difference(mask)
    assert masked.plan()["n_by_path"] == SC.path_counts(g["r"][0], host[0], CAPS) == [0, 0, 2000]
    want = SC.ref_op(g["r"], host, SC.DIFF)
    same(masked, want, "masked reads")
    sizes = np.diff(want[0].astype(np.int64))
    assert (sizes == 0).sum() > 300 and (sizes > 0).sum() > 300  # reads of the masked genome lose everything, the others nothing much
