"""GPU: the all-pairs comparison (bsk_sets_compare; compare.hip's k_cmp_tile) and bsk_sets_bottom against NumPy on host arrays -- every
cell of both matrices, every offset, value and count.  Where a case claims a branch of the round rule, bsk_compare_plan's figures are
asserted first, against the pure-Python restatement of the rule in tests/compare_cases.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import compare_cases as CC
from tests.compare_cases import collection

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
CAPS = CC.read_caps()
R, COLS, W, PER_CU = CAPS["CMP_ROWS"], CAPS["CMP_COLS"], CAPS["CMP_WINDOW"], CAPS["CMP_BLOCKS_PER_CU"]


@functools.lru_cache(None)
def cus():
    hip = C.CDLL("libamdhip64.so")
    hip.hipDeviceGetAttribute.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
    v = C.c_int()
    assert hip.hipDeviceGetAttribute(C.byref(v), 63, 0) == 0 and v.value > 0  # hipDeviceAttributeMultiprocessorCount
    return v.value


def load(engine, sets):
    return engine.sets_from_arrays(*collection(sets))


def figures(cmp):
    p = cmp.plan()
    return p["tiles"], p["rounds"], p["max_rounds"]


def check(engine, A, B, limit, what="", dA=None, dB=None, reuse=None, rounds=True, want=None):
    """A x B on the device: the plan's figures as the restatement counts them, then every cell"""
    dA = dA if dA is not None else load(engine, A)
    dB = dB if dB is not None else (dA if B is A else load(engine, B))
    cmp = dA.compare(dB, limit, reuse)
    assert cmp.info() == dict(n_a=len(A), n_b=len(B), limit=limit), what
    got = figures(cmp)
    assert got[0] == CC.n_tiles(len(A), len(B), CAPS), (what, got)
    if rounds:
        assert got == CC.plan_figures(A, B, limit, CAPS), (what, limit, got)
    assert "k_cmp_tile" in cmp.plan()["plan"] and f"{R} x {COLS}" in cmp.plan()["plan"]
    want = want if want is not None else CC.ref_compare(A, B, limit)
    assert cmp.shared.dtype == U32 and cmp.shared.shape == (len(A), len(B)) == cmp.total.shape, what
    assert np.array_equal(cmp.total, want[1]), (what, limit, "total", np.argwhere(cmp.total != want[1])[:5])
    assert np.array_equal(cmp.shared, want[0]), (what, limit, "shared", np.argwhere(cmp.shared != want[0])[:5])
    return cmp


def test_hand_case(engine):
    A, B, want = CC.hand_case()
    dA, dB = load(engine, A), load(engine, B)
    for limit, (sh, tt) in want.items():
        cmp = check(engine, A, B, limit, "hand", dA, dB, want=(np.array(sh, U32), np.array(tt, U32)))
        assert figures(cmp) == (1, 1, 1)
    j = dA.compare(dB).jaccard()
    assert j.tolist() == [[2 / 5, 1 / 4], [0.0, 0.0], [1 / 4, 0.0]]
    assert dA.compare(dB).containment().tolist() == [[2 / 4, 1 / 4], [0.0, 0.0], [1 / 2, 0.0]]
    with pytest.raises(ValueError):
        dA.compare(dB, limit=2).containment()


def test_window_edges(engine):
    A, B, claim = CC.window_edges(W)
    dA, dB = load(engine, A), load(engine, B)
    cmp = None
    for limit in claim["limits"]:
        cmp = check(engine, A, B, limit, "window edges", dA, dB, reuse=cmp)
    assert figures(check(engine, A, B, 0, "window edges", dA, dB))[2] >= 3 and figures(check(engine, A, B, 1, "window edges", dA, dB)) == (1, 1, 1)


def test_tile_edges(engine):
    A, B, claim = CC.tile_edges(R, COLS)
    dA, dB = {}, {}
    full = CC.ref_compare(A, B, 0), CC.ref_compare(A, B, 7)
    cmp = None
    for na, nb in claim["shapes"]:
        if na not in dA:
            dA[na] = load(engine, A[:na])
        if nb not in dB:
            dB[nb] = load(engine, B[:nb])
        for k, limit in enumerate((0, 7)):
            want = full[k][0][:na, :nb], full[k][1][:na, :nb]
            cmp = check(engine, A[:na], B[:nb], limit, f"tile edges {na} x {nb}", dA[na], dB[nb], reuse=cmp, rounds=False, want=want)
            tiles = -(-na // R) * -(-nb // COLS)
            assert figures(cmp) == (tiles, tiles, 1)  # sets of 20 values: one round a tile


def test_one_against_many_and_self(engine):
    A, B, _ = CC.tile_edges(R, COLS)
    check(engine, A[:1], B, 0, "one against many")
    check(engine, A, B[:1], 0, "many against one")
    check(engine, A, B[:1], 5, "many against one")
    cmp = check(engine, A, A, 0, "a is b")
    assert np.array_equal(np.diag(cmp.shared), [len(s) for s in A]) and np.array_equal(cmp.shared, cmp.shared.T)
    check(engine, A, A, 9, "a is b")


def test_empty_operands(engine):
    A, _, _ = CC.tile_edges(R, COLS)
    dA, none = load(engine, A[:5]), load(engine, [])
    for a, b, shape in ((none, dA, (0, 5)), (dA, none, (5, 0)), (none, none, (0, 0))):
        cmp = a.compare(b, 3)
        assert cmp.info() == dict(n_a=shape[0], n_b=shape[1], limit=3) and figures(cmp) == (0, 0, 0)
        assert cmp.shared.shape == shape and cmp.total.shape == shape and cmp.jaccard().shape == shape
    empties = [np.zeros(0, U64)] * 3
    cmp = check(engine, empties, A[:2], 0, "empty sets")
    assert not cmp.shared.any() and np.array_equal(cmp.total, [[len(A[0]), len(A[1])]] * 3)


def test_extreme_values(engine):
    S_, _, claim = CC.extreme_values(W)
    d = load(engine, S_)
    for limit in claim["limits"]:
        check(engine, S_, S_, limit, "extreme values", d, d)
    e = claim["edge_index"]
    # the set whose window boundary falls between 2^64-2 and 2^64-1 takes a second round
    assert figures(check(engine, [S_[e]], [S_[e], S_[4]], 0, "window boundary at the top"))[2] == 2


def test_skew(engine):
    for name, (A, B) in CC.skew_cases(W).items():
        for limit in (0, W + 3):
            check(engine, A, B, limit, "skew " + name)
    A, B = CC.skew_cases(W)["low"]
    assert figures(check(engine, A, B, 0, "skew low")) == (1, 5, 5)
    A, B = CC.skew_cases(W)["dense"]
    assert figures(check(engine, A, B, 0, "skew dense")) == (1, 10, 10)


def test_where_the_limit_lands(engine):
    for a, b, limit, sh, tt in CC.limit_landings():
        cmp = check(engine, [a], [b], limit, "limit landing")
        assert (int(cmp.shared[0, 0]), int(cmp.total[0, 0])) == (sh, tt), (a, b, limit)


def test_early_stop(engine):
    rng = np.random.default_rng(21)
    sets = [np.sort(rng.choice(1 << 30, 8 * W, replace=False).astype(U64)) for _ in range(6)]
    assert figures(check(engine, sets, sets, 3, "early stop")) == (1, 1, 1)
    # a limit beyond one window stops the tile as soon as every pair has walked it: long before the sets end
    got = figures(check(engine, sets, sets, 3 * W, "early stop past a window"))
    assert 1 < got[2] < figures(check(engine, sets, sets, 0, "no stop"))[2]


def test_compare_equals_compare_of_bottoms(engine):
    sets, claim = CC.mash_shape()
    A, B = sets[:9], sets[9:20]
    dA, dB = load(engine, A), load(engine, B)
    for n in (1, 77, W, 1000):
        full = dA.compare(dB, n)
        cut = dA.bottom(n).compare(dB.bottom(n), n)
        assert np.array_equal(full.shared, cut.shared) and np.array_equal(full.total, cut.total), n
        assert np.all(full.total == n) and (n == 1 or full.shared.max() > 0)


def test_mash_shape(engine):
    sets, claim = CC.mash_shape()
    cmp = check(engine, sets, sets, claim["limit"], "mash shape", rounds=False)
    tiles, rounds, most = figures(cmp)
    assert tiles == CC.n_tiles(40, 40, CAPS) and rounds >= 3 * tiles and most >= 3  # several rounds a tile
    assert np.all(cmp.total == 1000) and np.all(np.diag(cmp.shared) == 1000)
    j = cmp.jaccard()
    assert 0.1 < np.median(j) < 0.35  # 1 000 of 3 000 each: the Jaccard of two such sets is about 1/5


def test_more_tiles_than_one_pass_of_the_grid(engine):
    tiles_wanted = cus() * PER_CU + 3
    ty = int(np.ceil(np.sqrt(tiles_wanted)))
    tx = -(-tiles_wanted // ty)
    na, nb = ty * R - 3, tx * COLS - 5
    assert CC.n_tiles(na, nb, CAPS) >= tiles_wanted
    A, ma = CC.small_pool_sets(na, seed=31)
    B, mb = CC.small_pool_sets(nb, seed=32)
    dA, dB = load(engine, A), load(engine, B)
    cmp = dA.compare(dB, 0)
    assert figures(cmp) == (ty * tx, ty * tx, 1)
    sh, tt = CC.mask_compare(ma, mb)
    assert np.array_equal(cmp.shared, sh) and np.array_equal(cmp.total, tt)
    cmp = dA.compare(dB, 2, reuse=cmp)
    assert figures(cmp) == (ty * tx, ty * tx, 1) and np.all(cmp.total == 2)
    rng = np.random.default_rng(33)
    cells = [(int(i), int(j)) for i, j in zip(rng.integers(0, na, 2000), rng.integers(0, nb, 2000))]
    for i0, j0 in ((0, 0), (0, nb - COLS), (na - R, 0), (na - R, nb - COLS)):  # the corner tiles
        cells += [(i0 + i, j0 + j) for i in range(R) for j in range(COLS)]
    for i, j in cells:
        assert (int(cmp.shared[i, j]), int(cmp.total[i, j])) == CC.ref_pair(A[i], B[j], 2), (i, j)


def test_object_rules(engine):
    lib = engine.lib
    A, B, _ = CC.tile_edges(R, COLS)
    big, small = (A, B), (A[:3], B[:2])
    cmp = None
    for a, b in (big, small, big):
        cmp = check(engine, a, b, 0, "reuse", reuse=cmp, rounds=False)
    dA, dB = load(engine, A[:4]), load(engine, B[:3])
    cmp = dA.compare(dB, 0)
    want = CC.ref_compare(A[:4], B[:3], 0)
    # a foreign context: BSK_ERR_ARG, *cmp kept
    other = S.Engine(0)
    foreign = load(other, B[:3])
    h = C.c_void_p(cmp.h.value)
    assert lib.bsk_sets_compare(engine.ctx, dA.h, foreign.h, 0, C.byref(h)) == L.ERR_ARG and h.value == cmp.h.value
    assert lib.bsk_sets_compare(other.ctx, foreign.h, foreign.h, 0, C.byref(h)) == L.ERR_ARG and h.value == cmp.h.value
    sh, tt = np.zeros(12, U32), np.zeros(12, U32)
    assert lib.bsk_compare_fetch(other.ctx, cmp.h, 0, 4, sh.ctypes.data, tt.ctypes.data, 12) == L.ERR_ARG
    foreign.close()
    other.close()
    # fetch: row ranges, either array, the cap
    for first, n in ((0, 4), (1, 2), (3, 1), (4, 0), (2, 0)):
        s, t = cmp.fetch(first, n)
        assert np.array_equal(s, want[0][first:first + n]) and np.array_equal(t, want[1][first:first + n])
    assert lib.bsk_compare_fetch(engine.ctx, cmp.h, 1, 2, None, tt.ctypes.data, 6) == L.OK and np.array_equal(tt[:6], want[1][1:3].ravel())
    assert lib.bsk_compare_fetch(engine.ctx, cmp.h, 1, 2, sh.ctypes.data, None, 6) == L.OK and np.array_equal(sh[:6], want[0][1:3].ravel())
    assert lib.bsk_compare_fetch(engine.ctx, cmp.h, 1, 2, sh.ctypes.data, tt.ctypes.data, 5) == L.ERR_ARG
    assert lib.bsk_compare_fetch(engine.ctx, cmp.h, 3, 2, sh.ctypes.data, tt.ctypes.data, 12) == L.ERR_ARG
    assert lib.bsk_compare_fetch(engine.ctx, cmp.h, 5, 0, sh.ctypes.data, tt.ctypes.data, 12) == L.ERR_ARG
    ps, pt = cmp.device()
    assert ps and pt and ps != pt
    # too many cells: BSK_ERR_UNSUPPORTED before anything is allocated, the object released
    rows, cols = load(engine, [np.zeros(0, U64)] * 65536), load(engine, [np.zeros(0, U64)] * 32769)
    h = C.c_void_p(cmp.h.value)
    cmp.h = None  # (the library releases it)
    assert lib.bsk_sets_compare(engine.ctx, rows.h, cols.h, 0, C.byref(h)) == L.ERR_UNSUPPORTED and h.value is None
    with pytest.raises(Exception):
        rows.compare(cols)
    assert rows.compare(load(engine, [np.zeros(0, U64)] * 5)).total.shape == (65536, 5)


# ---- bsk_sets_bottom ----
def same_sets(sets, want_sets, counts=None, what=""):
    o, v = sets.fetch()
    wo, wv = collection(want_sets)
    assert np.array_equal(o, wo) and np.array_equal(v, wv), what
    assert sets.plan() == dict(plan="", n_by_path=[0, 0, 0]), what
    assert sets.counted == (counts is not None), what
    if counts is not None:
        assert np.array_equal(sets.fetch_counts(), counts), what


def test_bottom_against_numpy(engine):
    sets, sizes = CC.bottom_sets()
    d = load(engine, sets)
    offs, vals = collection(sets)
    counts = (1 + (vals % U64(1000))).astype(U32)
    dc = engine.sets_from_arrays_counted(offs, vals, counts)
    into = None
    for n in list(range(1, 73)) + [1024, 1025, 1026, 1 << 40]:  # size - 1, size, size + 1 of every set size, and beyond all
        want = CC.ref_bottom(sets, n)
        same_sets(d.bottom(n), want, None, n)
        into = dc.bottom(n, into)  # the same object through every n: smaller, larger, smaller
        same_sets(into, want, np.concatenate([c[:n] for c in CC.split(offs, counts)]), n)
    plain = d.bottom(4, into)  # a counted object re-used for plain sets
    assert plain is into
    same_sets(plain, CC.ref_bottom(sets, 4), None, "reuse")
    # the result is an ordinary bsk_sets: the algebra takes it
    u = d.bottom(5).union(d.bottom(2))
    same_sets_values = collection(CC.ref_bottom(sets, 5))
    assert np.array_equal(u.fetch()[1], same_sets_values[1])


def test_bottom_argument_rules(engine):
    lib = engine.lib
    sets, _ = CC.bottom_sets()
    d = load(engine, sets)
    out = d.bottom(3)
    h = C.c_void_p(out.h.value)
    assert lib.bsk_sets_bottom(engine.ctx, d.h, 0, C.byref(h)) == L.ERR_ARG and h.value == out.h.value
    own = C.c_void_p(d.h.value)
    assert lib.bsk_sets_bottom(engine.ctx, d.h, 3, C.byref(own)) == L.ERR_ARG and own.value == d.h.value
    other = S.Engine(0)
    foreign = load(other, sets[:3])
    assert lib.bsk_sets_bottom(engine.ctx, foreign.h, 3, C.byref(h)) == L.ERR_ARG and h.value == out.h.value
    foreign.close()
    other.close()
    same_sets(out, CC.ref_bottom(sets, 3))
    empty = load(engine, [])
    assert empty.bottom(3).info() == dict(n_sets=0, n_values=0)
    same_sets(load(engine, [np.zeros(0, U64)] * 4).bottom(2), [np.zeros(0, U64)] * 4)


@pytest.mark.parametrize("size,n", [(5, 3), (60, 40)])
def test_bottom_beyond_one_pass_of_its_grid(engine, size, n):
    """more sets than one pass of the gather's capped grid, on the 8-lane path (n <= CMP_BT_SMALL) and on the wavefront path"""
    lanes = 8 if n <= CAPS["CMP_BT_SMALL"] else 64
    n_sets = cus() * CAPS["CMP_BT_BLOCKS_PER_CU"] * (256 // lanes) + 77
    rng = np.random.default_rng(size)
    sizes = rng.integers(0, size + 1, n_sets)
    offs = np.zeros(n_sets + 1, U64)
    offs[1:] = np.cumsum(sizes)
    N = int(offs[-1])
    vals = (np.arange(N, dtype=U64) * U64(7919)) + U64(11)  # ascending everywhere, so ascending inside every set
    got = engine.sets_from_arrays(offs, vals).bottom(n)
    kept = np.minimum(sizes, n)
    assert kept.sum() > (CAPS["CMP_BT_SMALL"] * n_sets if lanes == 64 else 0) and kept.sum() <= (CAPS["CMP_BT_SMALL"] * n_sets if lanes == 8 else N)
    wo = np.zeros(n_sets + 1, U64)
    wo[1:] = np.cumsum(kept)
    o, v = got.fetch()
    assert np.array_equal(o, wo)
    within = np.arange(int(wo[-1]), dtype=np.int64) - np.repeat(wo[:-1].astype(np.int64), kept)
    assert np.array_equal(v, vals[np.repeat(offs[:-1].astype(np.int64), kept) + within])


def test_an_index_of_bottoms_finds_what_numpy_truncation_finds(engine):
    sets, _ = CC.mash_shape()
    targets, queries = sets[:12], sets[12:20]
    dq = load(engine, queries)
    a = load(engine, targets).bottom(200).index().search(dq, min_shared=1)
    b = load(engine, CC.ref_bottom(targets, 200)).index().search(dq, min_shared=1)
    assert a.info()["n_hits"] > 0
    for x, y in zip(a.fetch(), b.fetch()):
        assert np.array_equal(x, y)


# ---- end to end through the Python mirror ----
def test_mutated_genomes_end_to_end(engine):
    seqs = CC.mutated_sequences()
    res = engine.run(engine.batch(seqs), engine.params(L.NTHASH, 21, canonical=True))
    sets = res.device_sets()
    host = CC.split(*sets.fetch())
    assert len(host) == 5 and all(len(s) > 150_000 for s in host)
    cmp = sets.compare(limit=1000)
    want = CC.ref_compare(host, host, 1000)
    assert np.array_equal(cmp.shared, want[0]) and np.array_equal(cmp.total, want[1])
    j = cmp.jaccard()
    assert np.all(np.diag(j) == 1.0) and j[0, 1] == 1.0  # the 0 % copy is the sequence itself
    d = cmp.mash_distance(21)
    assert d[0, 0] == 0.0 and d[0, 1] <= d[0, 2] <= d[0, 3] <= d[0, 4]  # no decrease with divergence
    assert np.array_equal(cmp.shared, cmp.shared.T)
    bottoms = sets.bottom(1000)
    assert bottoms.info() == dict(n_sets=5, n_values=5000)
    again = bottoms.compare(limit=1000)
    assert np.array_equal(again.shared, cmp.shared) and np.array_equal(again.total, cmp.total)
