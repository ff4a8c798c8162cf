"""GPU: sketch sets (bsk_result_sets, sets.hip) at the places where the code changes behaviour.

Every case takes reads crafted for one edge (tests/sets_cases.py), asserts from the engine's own offsets that the edge was reached --
the batch's largest count selects the DPP bitonic kernel (<= 64) or the segmented radix sort, the per-wave maxima select the 16-, 32-
or 64-value network, the plan names the layout -- and then compares offsets and values exactly with ref_sets over the ORACLE's values.
Per-sequence sets run four ways: default, BSK_SETS_NO_SMALL (the general path on the same input), BSK_NO_GROUP_GATHER (k_move_seqs in
place of k_move_groups) and both."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import sets_cases as SC

pytestmark = pytest.mark.gpu
U64 = np.uint64
KIND = {"kmer": L.KMER, "nthash": L.NTHASH, "minimizer": L.MINIMIZER, "syncmer": L.SYNCMER}
CONFIGS = [(), ("BSK_SETS_NO_SMALL",), ("BSK_NO_GROUP_GATHER",), ("BSK_SETS_NO_SMALL", "BSK_NO_GROUP_GATHER")]
TRIP = SC.SCAN_TRIP * SC.SCAN_CHUNK


@contextlib.contextmanager
def switches(engine, env):
    env = dict(env) if isinstance(env, dict) else {k: "1" for k in env}
    os.environ.update(env)
    try:
        engine.reload_options()
        yield
    finally:
        for k in env:
            del os.environ[k]
        engine.reload_options()


def sketch(engine, case, reads=None):
    b = engine.batch(case["reads"] if reads is None else reads)
    res = engine.run(b, engine.params(KIND[case["kind"]], **case["pk"]))
    res.batch = b  # (alive as long as its result)
    return res


def counts_of(res):
    return np.diff(res.fetch()[0]).astype(np.int64)


def fetch_sets(res, whole, scale):
    s = res.device_sets(whole_batch=whole, scale=scale)
    try:
        offs, vals = s.fetch()
        assert int(offs[-1]) == len(vals) == s.info()["n_values"] and len(offs) == s.info()["n_sets"] + 1
        return offs, vals
    finally:
        s.close()


def has(a, x):
    return bool((np.asarray(a, U64) == U64(x)).any())


def equal(got, want, what):
    assert np.array_equal(got[0], want[0]), ("offsets",) + what
    assert np.array_equal(got[1], want[1]), ("values",) + what


def check(engine, res, want_of, scales, small, counts, whole=True):
    """the path's condition from the engine's own offsets, then every configuration against the reference of every scale"""
    got_counts = counts_of(res)
    assert np.array_equal(got_counts, counts), "the engine's counts are not the oracle's"
    assert (got_counts.max() <= SC.SMALL_CAP) == small, got_counts.max()
    for scale in scales:
        want = want_of(scale, False)
        for cfg in CONFIGS:
            with switches(engine, cfg):
                equal(fetch_sets(res, False, scale), want, (scale, cfg))
        if whole:
            equal(fetch_sets(res, True, scale), want_of(scale, True), (scale, "whole"))


def check_reads(engine, oracle, case, scales, small, reads=None, whole=True):
    if reads is not None:
        case = dict(case, reads=reads)
    vals = SC.values_of(oracle, case)
    res = sketch(engine, case)
    check(engine, res, lambda scale, w: SC.ref_sets(vals, scale, w), scales, small, [len(v) for v in vals], whole)
    return res, vals


# ---- counts ----
@pytest.mark.parametrize("tail", [0, 1, 2, 3])
@pytest.mark.parametrize("k", [21, 4])
def test_count_ladder(engine, oracle, k, tail):
    """every count of 0 .. 64 around 16 / 32 / 48 at every row of a wave of four, each network forced on short rows by one long
    neighbour, n % 4 = tail with a loaded last wave; k = 21 without duplicates (and filtered at 2^41), k = 4 full of them"""
    case = SC.ladder_case(oracle, k, tail)
    res, _ = check_reads(engine, oracle, case, (1, 2**23) if k == 21 else (1,), small=True)
    got = counts_of(res)
    assert len(got) % 4 == tail and np.array_equal(SC.wave_widths(got), case["widths"]) and set(case["widths"]) == {16, 32, 64}
    assert np.array_equal(got[:4 * len(SC.ladder_waves())].reshape(-1, 4), SC.ladder_waves())


@pytest.mark.parametrize("k", [21, 4])
def test_one_read_of_65_moves_the_batch_to_the_general_path(engine, oracle, k):
    case = SC.ladder_case(oracle, k, 0, extra65=True)
    res, _ = check_reads(engine, oracle, case, (1,), small=False)
    got = counts_of(res)
    assert (got == SC.SMALL_CAP + 1).sum() == 1 and (got > SC.SMALL_CAP + 1).sum() == 0


def test_duplicates_at_register_boundaries(engine, oracle):
    """equal values at sorted ranks 15/16, 31/32, 47/48 (element reg * 16 + 15 against lane 0 of the register above) and just after
    them; poly-A and period-2 reads of 17, 33, 49 and 64 values"""
    case = SC.dup_boundary_case(oracle)
    res, vals = check_reads(engine, oracle, case, (1,), small=True)
    for v, f in zip(vals, case["facts"]):
        v = np.sort(v)
        if f["how"] == "at":
            assert v[f["b"] - 1] == v[f["b"]]
        elif f["how"] == "after":
            assert v[f["b"] - 1] != v[f["b"]] == v[f["b"] + 1]


def test_filter_boundaries(engine, oracle):
    """reads of 48 and 64 ntHash values of which exactly 0, 1, 15, 16, 17, 32, 48 or all pass their scale, duplicates on both sides
    of the cut among them: one batch, every scale any of its reads was searched for"""
    cases = SC.filter_case(oracle)
    case = dict(kind="nthash", pk=dict(k=SC.FILTER_K), reads=[e["read"] for e in cases])
    scales = sorted({e["scale"] for e in cases})
    res, vals = check_reads(engine, oracle, case, scales, small=True)
    assert any(e["straddle"] for e in cases)
    for e, v in zip(cases, vals):
        assert int((v <= U64(SC.maxhash(e["scale"]))).sum()) == e["b"] and len(v) == e["c"]
        offs, _ = fetch_sets(res, False, e["scale"])
        i = cases.index(e)
        assert int(offs[i + 1] - offs[i]) == len(np.unique(v[v <= U64(SC.maxhash(e["scale"]))])) <= e["b"]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_exact_thresholds(engine, oracle, which):
    """m = MaxUint64 // scale itself: m - 1 and m are kept, m + 1 is dropped -- as three one-value reads (small path) and inside one
    read of 65 values (general path)"""
    e = SC.threshold_case(oracle)[which]
    m, scale = e["m"], e["scale"]
    res, _ = check_reads(engine, oracle, e, (scale, 1), small=True, reads=e["short"])
    for cfg in CONFIGS:
        with switches(engine, cfg):
            offs, vals = fetch_sets(res, False, scale)
        assert list(offs) == [0, 1, 2, 2] and [int(x) for x in vals] == [m - 1, m], (cfg, offs, vals)
    res, _ = check_reads(engine, oracle, e, (scale, 1), small=False, reads=e["short"] + [e["long"]])
    offs, vals = fetch_sets(res, False, scale)
    long_set = vals[int(offs[3]):int(offs[4])]
    assert has(long_set, m - 1) and has(long_set, m) and not has(long_set, m + 1) and list(offs[:4]) == [0, 1, 2, 2]
    offs, vals = fetch_sets(res, True, scale)
    assert has(vals, m - 1) and has(vals, m) and not has(vals, m + 1)


def test_sentinel_value_is_a_legal_value(engine, oracle):
    """~0 (both-strand 32-mers of T x 32) is what filtered elements become: kept once at scale 0 and 1, dropped at 2 while 0 stays"""
    case = SC.sentinel_case()
    res, vals = check_reads(engine, oracle, case, (0, 1, 2), small=True)
    for cfg in CONFIGS:
        with switches(engine, cfg):
            for scale in (0, 1, 2):
                offs, v = fetch_sets(res, False, scale)
                for i, full in enumerate(case["holds_full"]):
                    s = v[int(offs[i]):int(offs[i + 1])]
                    assert int((s == U64(SC.FULL)).sum()) == (1 if full and scale < 2 else 0), (cfg, scale, i)
                    assert int((s == 0).sum()) == (1 if full else 0), (cfg, scale, i)
    check_reads(engine, oracle, case, (0, 1, 2), small=False, reads=case["reads"] + ["T" * 64])  # 66 values: the general path itself


# ---- layouts ----
@pytest.mark.parametrize("name", list(SC.LAYOUTS))
def test_result_layouts_in_the_small_path(engine, oracle, name):
    """unit rows (stride 64), per-read slabs, packed slabs and a wide (tiled) result, every count <= 64"""
    case = SC.layout_case(oracle, name)
    with switches(engine, case["env"]):
        res = sketch(engine, case)
        assert case["plan"] in res.plan()["kernel"], res.plan()
        vals = SC.values_of(oracle, case)
        check(engine, res, lambda scale, w: SC.ref_sets(vals, scale, w), (1, 3), True, [len(v) for v in vals])


# ---- scan trips ----
def test_scan_trips_per_sequence(engine, oracle):
    """2 * 1024 * 2048 + 2049 reads of four values: the counts scan and the distinct-count scan take three trips of k_scan_top"""
    case = SC.scan_reads_case(oracle)
    n = case["n"]
    assert n > 2 * TRIP + SC.SCAN_CHUNK
    res = engine.run(engine.batch_from_arrays(case["data"], case["offsets"]), engine.params(L.NTHASH, case["pk"]["k"]))
    counts = np.where(case["present"], case["step"], 0)
    got = counts_of(res)
    assert np.array_equal(got, counts) and got.max() <= SC.SMALL_CAP and not got[[0, TRIP - 1, TRIP, 2 * TRIP]].any() and got[-1]
    want = SC.ref_sets_rows(case["v2d"], 3, False, case["present"])
    assert len(np.unique(np.diff(want[0]))) > 2  # (the second scan's numbers differ from read to read)
    for cfg in CONFIGS:
        with switches(engine, cfg):
            equal(fetch_sets(res, False, 3), want, (3, cfg))
    equal(fetch_sets(res, False, 1), SC.ref_sets_rows(case["v2d"], 1, False, case["present"]), (1,))


def test_scan_trips_of_values(engine, oracle):
    """more than 1024 * 2048 values, every count 130: the general path's scan of the keep flags takes a second trip"""
    case = SC.scan_values_case()
    v2d = SC.scan_values_v2d(oracle, case)
    assert v2d.size > TRIP
    res = engine.run(engine.batch_from_arrays(case["data"], case["offsets"]), engine.params(L.NTHASH, case["pk"]["k"]))
    check(engine, res, lambda scale, w: SC.ref_sets_rows(v2d, scale, w), (1, 3), False, np.full(case["n"], case["count"]))


# ---- whole-batch scope ----
def test_whole_batch_with_one_loaded_read(engine, oracle):
    case = dict(kind="kmer", pk=dict(k=21), reads=[""] * 70 + ["ACGT"] * 3 + ["ACGTTGCATGCCAGTACCGATTAGCAT"])  # all empty but the last
    check_reads(engine, oracle, case, (1, 2**23), small=True)
    one = dict(case, reads=["", "ACGTTGCATGCCAGTACCGAT", "", ""])  # one value in total
    res, vals = check_reads(engine, oracle, one, (1,), small=True)
    offs, v = fetch_sets(res, True, 1)
    assert list(offs) == [0, 1] and int(v[0]) == int(vals[1][0])


# ---- bsk_result_sets_reuse ----
def _reuse(engine, h, res, scope, scale, ctx=None):
    engine._opts()
    return engine.lib.bsk_result_sets_reuse(ctx or engine.ctx, res.h if res is not None else None, scope, scale, C.byref(h))


def test_sets_reuse_through_one_object(engine, oracle):
    """small, then large -> small -> all-empty -> large -> whole-batch -> per-sequence through ONE object, each equal to a fresh bsk_result_sets;
    the device arrays stay where they are while nothing larger arrives; an error releases the object and leaves *sets NULL"""
    rng = np.random.default_rng(7)
    p = dict(kind="nthash", pk=dict(k=21))
    large = sketch(engine, p, [SC.rand_read(rng, int(rng.integers(100, 300))) for _ in range(900)])
    small = sketch(engine, p, [SC.rand_read(rng, int(rng.integers(0, 60))) for _ in range(300)])
    empty = sketch(engine, p, ["ACGT", "", "AC"] * 20)
    h = C.c_void_p()
    ptrs = []
    steps = [(small, 0, 3), (large, 0, 3), (small, 0, 3), (empty, 0, 1), (large, 0, 3), (large, 1, 3), (large, 0, 1), (small, 1, 0), (small, 0, 2)]
    for i, (res, scope, scale) in enumerate(steps):
        assert _reuse(engine, h, res, scope, scale) == L.OK and h.value
        s = S.Sets(engine, h)
        try:
            equal(s.fetch(), fetch_sets(res, bool(scope), scale), (i,))
            ptrs.append(s.device())
        finally:
            s.h = None  # (the object stays ours)
    assert all(a and b for a, b in ptrs)
    assert all(q == ptrs[1] for q in ptrs[2:]), ptrs  # grown once for `large`; nothing after it is larger: nothing moves
    other = S.Engine(0)
    try:
        foreign = sketch(other, p, ["ACGTTGCATGCCAGTACCGATTAGCAT"])
        for res, scope, scale in ((large, 2, 1), (large, 0, -1), (foreign, 0, 1)):
            if not h.value:
                assert _reuse(engine, h, small, 0, 1) == L.OK and h.value
            assert _reuse(engine, h, res, scope, scale) == L.ERR_ARG and h.value is None, (scope, scale)
            assert _reuse(engine, h, small, 0, 3) == L.OK and h.value  # the context is still usable, from NULL again
            s = S.Sets(engine, h)
            try:
                equal(s.fetch(), fetch_sets(small, False, 3), ("after an error",))
            finally:
                s.h = None
        assert _reuse(other, h, foreign, 0, 1, ctx=other.ctx) == L.ERR_ARG and h.value  # sets of another context: refused, left alone
        foreign.close()
        foreign.batch.close()
    finally:
        engine.lib.bsk_sets_release(h)
        other.close()


# ---- bsk_sets_fetch / bsk_sets_fetch_narrow ----
def _sets_for_fetch(engine, oracle):
    rng = np.random.default_rng(11)
    reads = [SC.rand_read(rng, int(rng.integers(21, 120))) for _ in range(64 * 4 + 9)]
    for i in range(100, 120):
        reads[i] = "ACGT"  # a run of empty sets
    reads[0] = ""
    case = dict(kind="nthash", pk=dict(k=21), reads=reads)
    return sketch(engine, case), SC.ref_sets(SC.values_of(oracle, case), 2, False)


def test_sets_fetch_sub_ranges(engine, oracle):
    res, (woffs, wvals) = _sets_for_fetch(engine, oracle)
    n = len(woffs) - 1
    s = res.device_sets(scale=2)
    lib, w = engine.lib, woffs.astype(np.int64)
    try:
        assert s.info() == dict(n_sets=n, n_values=len(wvals))
        for first, count in ((0, 0), (1, 1), (n - 1, 1), (n, 0), (63, 130), (101, 15), (0, n)):
            a, b = int(w[first]), int(w[first + count])
            offs, vals = np.full(count + 1, 99, U64), np.full(b - a + 1, 77, U64)
            assert lib.bsk_sets_fetch(engine.ctx, s.h, first, count, offs.ctypes.data, vals.ctypes.data, b - a) == L.OK, (first, count)
            assert np.array_equal(offs, woffs[first:first + count + 1] - woffs[first]), (first, count)  # rebased
            assert np.array_equal(vals[:b - a], wvals[a:b]) and vals[b - a] == 77, (first, count)
            only = np.full(count + 1, 99, U64)
            assert lib.bsk_sets_fetch(engine.ctx, s.h, first, count, only.ctypes.data, None, 0) == L.OK and np.array_equal(only, offs)
            if b > a:  # one value short
                assert lib.bsk_sets_fetch(engine.ctx, s.h, first, count, offs.ctypes.data, vals.ctypes.data, b - a - 1) == L.ERR_ARG
        assert w[116] == w[101] and w[63 + 130] > w[63]  # (the range of empty sets only; a loaded one)
        offs, vals = np.zeros(n + 2, U64), np.zeros(len(wvals) + 1, U64)
        for first, count in ((0, n + 1), (n, 1), (n + 1, 0), (1, n), (2**64 - 1, 2)):  # (the last: first + count wraps to 1)
            assert lib.bsk_sets_fetch(engine.ctx, s.h, first, count, offs.ctypes.data, vals.ctypes.data, len(vals)) == L.ERR_ARG, (first, count)
        assert np.array_equal(s.fetch()[1], wvals)  # and the context goes on
    finally:
        s.close()


def test_sets_fetch_narrow_and_foreign_sets(engine, oracle):
    res, (woffs, wvals) = _sets_for_fetch(engine, oracle)
    n, nv = len(woffs) - 1, len(wvals)
    lib = engine.lib
    other = S.Engine(0)
    s = res.device_sets(scale=2)
    try:
        o32, vals = np.full(n + 1, 9, np.uint32), np.full(nv + 1, 77, U64)
        assert lib.bsk_sets_fetch_narrow(engine.ctx, s.h, o32.ctypes.data, vals.ctypes.data, nv) == L.OK
        wide = s.fetch()
        assert np.array_equal(o32.astype(U64), wide[0]) and np.array_equal(vals[:nv], wide[1]) and vals[nv] == 77
        equal(wide, (woffs, wvals), ("wide",))
        only = np.full(n + 1, 9, np.uint32)
        assert lib.bsk_sets_fetch_narrow(engine.ctx, s.h, only.ctypes.data, None, 0) == L.OK and np.array_equal(only, o32)
        assert lib.bsk_sets_fetch_narrow(engine.ctx, s.h, o32.ctypes.data, vals.ctypes.data, nv - 1) == L.ERR_ARG  # one value short
        # sets of another context: both fetches refuse them
        o64 = np.zeros(n + 1, U64)
        assert lib.bsk_sets_fetch_narrow(other.ctx, s.h, o32.ctypes.data, vals.ctypes.data, nv) == L.ERR_ARG
        assert lib.bsk_sets_fetch(other.ctx, s.h, 0, n, o64.ctypes.data, vals.ctypes.data, nv) == L.ERR_ARG
        assert lib.bsk_sets_fetch(other.ctx, s.h, 0, 0, o64.ctypes.data, None, 0) == L.ERR_ARG
        assert b"another context" in lib.bsk_last_error(other.ctx)
        equal(s.fetch(), (woffs, wvals), ("after the refusals",))
    finally:
        s.close()
        other.close()


def test_scales_accepted_and_refused(engine, oracle):
    case = SC.ladder_case(oracle, 21, 1)
    vals = SC.values_of(oracle, case)
    res = sketch(engine, case)
    for scale in (0, 1, 2**31 - 1):
        for whole in (False, True):
            equal(fetch_sets(res, whole, scale), SC.ref_sets(vals, scale, whole), (scale, whole))
    assert len(SC.ref_sets(vals, 2**31 - 1, True)[1]) > 0  # (codes below 2^33 exist: the largest scale keeps something)
    for whole in (0, 1):
        h = C.c_void_p()
        assert engine.lib.bsk_result_sets(engine.ctx, res.h, whole, -1, C.byref(h)) == L.ERR_ARG and h.value is None
