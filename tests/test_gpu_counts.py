"""GPU: counted sketch sets from a result (bsk_result_sets_counted; sets.hip + counts.hip) against np.unique(return_counts=True) over the
ORACLE's values -- every offset, every value and every count, and offsets and values also against bsk_result_sets of the same call.

Every case runs per sequence -- with and without BSK_SETS_NO_SMALL, the switch that forces the uncounted call onto the general path --
and for the whole batch."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import counts_cases as CC
from tests import sets_cases as SC

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
CHUNK = CC.read_chunk()
CONFIGS = [(), ("BSK_SETS_NO_SMALL",)]
KIND = {"kmer": L.KMER, "nthash": L.NTHASH, "minimizer": L.MINIMIZER, "syncmer": L.SYNCMER}


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


@functools.lru_cache(None)
def cus():
    hip = C.CDLL("libamdhip64.so")
    hip.hipDeviceGetAttribute.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
    v = C.c_int()
    assert hip.hipDeviceGetAttribute(C.byref(v), 63, 0) == 0 and v.value > 0  # hipDeviceAttributeMultiprocessorCount
    return v.value


def fetch_counted(res, whole, scale, into=None):
    s = res.counted_sets(whole_batch=whole, scale=scale, into=into)
    try:
        assert s.counted
        offs, vals = s.fetch()
        cnt = s.fetch_counts()
        inf = s.info()
        assert int(offs[-1]) == len(vals) == len(cnt) == inf["n_values"] and len(offs) == inf["n_sets"] + 1
        assert np.array_equal(s.totals(), CC.ref_totals((offs, vals, cnt)))
        return offs, vals, cnt
    finally:
        if into is None:
            s.close()


def equal(got, want, what):
    for name, g, w in zip(("offsets", "values", "counts"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name,) + tuple(what)


def check(engine, res, want_of, scales):
    for scale in scales:
        for whole in (False, True):
            want = want_of(scale, whole)
            for cfg in CONFIGS if not whole else [()]:
                with switches(engine, cfg):
                    got = fetch_counted(res, whole, scale)
                    plain = res.device_sets(whole_batch=whole, scale=scale)
                equal(got, want, (scale, whole, cfg))
                po, pv = plain.fetch()
                assert not plain.counted and np.array_equal(po, got[0]) and np.array_equal(pv, got[1]), (scale, whole, cfg)
                plain.close()


class Ref:
    def __init__(self, values):
        self.values = values

    def __call__(self, scale, whole):
        return CC.ref_counted(self.values, scale, whole)


def check_reads(engine, oracle, case, scales, reads=None):
    if reads is not None:
        case = dict(case, reads=reads)
    vals = SC.values_of(oracle, case)
    res = sketch(engine, case)
    assert np.array_equal(np.diff(res.fetch()[0]).astype(np.int64), [len(v) for v in vals]), "the engine's counts are not the oracle's"
    check(engine, res, Ref(vals), scales)
    return res, vals


# ---- the small path's edges (counted calls take the general path: the same reads must count the same) ----
def test_duplicates_at_register_boundaries(engine, oracle):
    case = SC.dup_boundary_case(oracle)
    res, vals = check_reads(engine, oracle, case, (1,))
    offs, v, c = fetch_counted(res, False, 1)
    for i, f in enumerate(case["facts"]):
        mine = c[int(offs[i]):int(offs[i + 1])]
        if f["how"] == "poly":
            assert list(mine) == [f["count"]] and f["count"] in (17, 33, 49, 64)
        elif f["how"] == "period2":
            assert len(mine) == 2 and int(mine.sum()) == f["count"]
        else:
            assert int(mine.sum()) == f["count"] and mine.max() >= 2


@pytest.mark.parametrize("tail", [0, 1, 2, 3])
@pytest.mark.parametrize("k", [21, 4])
def test_count_ladder(engine, oracle, k, tail):
    check_reads(engine, oracle, SC.ladder_case(oracle, k, tail), (1, 2**23) if k == 21 else (1,))


@pytest.mark.parametrize("k", [21, 4])
def test_ladder_with_one_read_of_65(engine, oracle, k):
    check_reads(engine, oracle, SC.ladder_case(oracle, k, 0, extra65=True), (1,))


def test_neighbouring_reads_that_share_values(engine, oracle):
    """copies of one read in a row and reads whose extreme values meet: per sequence the runs stop at the border, whole batch they add"""
    case = CC.neighbours_case(oracle)
    res, vals = check_reads(engine, oracle, case, (1, 3))
    f = case["facts"]
    offs, v, c = fetch_counted(res, False, 1)
    wo, wv, wc = fetch_counted(res, True, 1)
    for copies in (2, 3, 130):
        i = f["copies%d" % copies]
        first = v[int(offs[i]):int(offs[i + 1])]
        for j in range(copies):
            assert np.array_equal(v[int(offs[i + j]):int(offs[i + j + 1])], first)
        assert np.all(wc[np.isin(wv, first)] >= copies) and c[int(offs[i]):int(offs[i + copies])].max() < copies
    i = f["max_then_single"]
    assert v[int(offs[i + 1]) - 1] == v[int(offs[i + 1])] and int(offs[i + 2] - offs[i + 1]) == 1 and c[int(offs[i + 1]) - 1] == c[int(offs[i + 1])] == 1
    assert wc[wv == v[int(offs[i + 1])]] == 2
    i = f["single_then_min"]
    assert v[int(offs[i])] == v[int(offs[i + 1])] and int(offs[i + 1] - offs[i]) == 1 and c[int(offs[i])] == c[int(offs[i + 1])] == 1


def test_filter_boundaries(engine, oracle):
    cases = SC.filter_case(oracle)
    case = dict(kind="nthash", pk=dict(k=SC.FILTER_K), reads=[e["read"] for e in cases])
    assert any(e["straddle"] for e in cases)
    check_reads(engine, oracle, case, sorted({e["scale"] for e in cases}))


@pytest.mark.parametrize("which", [0, 1, 2])
def test_exact_thresholds(engine, oracle, which):
    e = SC.threshold_case(oracle)[which]
    check_reads(engine, oracle, e, (e["scale"], 1), reads=e["short"] + [e["long"]] + e["short"])
    res, _ = check_reads(engine, oracle, e, (e["scale"],), reads=e["short"] * 2)
    offs, v, c = fetch_counted(res, True, e["scale"])
    assert [int(x) for x in v] == [e["m"] - 1, e["m"]] and list(c) == [2, 2]  # m + 1 is neither kept nor counted


def test_sentinel_value_is_counted_like_any_other(engine, oracle):
    """2^64 - 1, the general path's filler for filtered elements: a real value with its real count at scale <= 1, gone at scale 2"""
    case = SC.sentinel_case()
    res, vals = check_reads(engine, oracle, case, (0, 1, 2))
    full = sum(int((v == U64(SC.FULL)).sum()) for v in vals)
    assert full > 10
    for scale in (0, 1, 2):
        offs, v, c = fetch_counted(res, True, scale)
        assert (int(c[v == U64(SC.FULL)].sum()) if scale < 2 else int((v == U64(SC.FULL)).sum())) == (full if scale < 2 else 0)
    check_reads(engine, oracle, case, (0, 1, 2), reads=case["reads"] + ["T" * 64])


@pytest.mark.parametrize("name", list(SC.LAYOUTS))
def test_result_layouts(engine, oracle, name):
    case = SC.layout_case(oracle, name)
    with switches(engine, case["env"]):
        res = sketch(engine, case)
        assert case["plan"] in res.plan()["kernel"], res.plan()
        check(engine, res, Ref(SC.values_of(oracle, case)), (1, 3))


# ---- sizes ----
def test_runs_at_the_chunk_borders(engine, oracle):
    """whole-batch runs of 1, 2 047 .. 2 049 and 5 000 that end at and span a border of SCAN_CHUNK and of the run kernels' chunk"""
    assert CHUNK == SC.SCAN_CHUNK  # (one layout serves both; a change of either needs a second layout)
    case = CC.runs_case(oracle, CHUNK)
    res = sketch(engine, case)
    want = CC.ref_counted([[x] for x in case["values"]], 1, True)
    assert np.array_equal(want[2], case["lengths"])
    equal(fetch_counted(res, True, 1), want, ("whole",))
    equal(fetch_counted(res, False, 1), CC.ref_counted([[x] for x in case["values"]], 1, False), ("per sequence",))
    for scale in (2, 5):
        equal(fetch_counted(res, True, scale), CC.ref_counted([[x] for x in case["values"]], scale, True), ("whole", scale))


def test_one_run_that_is_the_whole_input(engine, oracle):
    n = 2 * CHUNK + 904
    case = dict(kind="kmer", pk=dict(k=21), reads=["A" * (n + 20)])
    res, vals = check_reads(engine, oracle, case, (1,))
    assert len(vals[0]) == n and len(np.unique(vals[0])) == 1
    for whole in (False, True):
        offs, v, c = fetch_counted(res, whole, 1)
        assert list(offs) == [0, 1] and list(c) == [n]
    case = dict(case, reads=["A" * 25] * 1000 + ["A" * (n + 20)] + ["A" * 21] * 1500)
    res, vals = check_reads(engine, oracle, case, (1,))
    assert list(fetch_counted(res, True, 1)[2]) == [5 * 1000 + n + 1500]


@pytest.fixture(scope="module")
def scan_values(oracle):
    case = SC.scan_values_case()
    return case, SC.scan_values_v2d(oracle, case)


@pytest.mark.parametrize("scale", [1, 3])
def test_more_values_than_one_pass_of_the_capped_grids(engine, scan_values, scale):
    """2.1 million values: beyond one pass of k_flag_unique's and the scatter's grids (16 workgroups of 256 per CU), a second trip of
    the scan's top kernel, a thousand chunks for the suffix minimum"""
    case, v2d = scan_values
    assert v2d.size > cus() * 16 * 256 and v2d.size > SC.SCAN_TRIP * SC.SCAN_CHUNK
    res = engine.run(engine.batch_from_arrays(case["data"], case["offsets"]), engine.params(L.NTHASH, case["pk"]["k"]))
    for whole in (False, True):
        equal(fetch_counted(res, whole, scale), CC.ref_counted_rows(v2d, scale, whole), (scale, whole))


# ---- empty ----
def test_empty_inputs(engine, oracle):
    for name, reads in CC.empty_cases().items():
        case = dict(kind="kmer", pk=dict(k=21), reads=reads)
        res = sketch(engine, case)
        for whole in (False, True):
            offs, v, c = fetch_counted(res, whole, 1)
            assert len(offs) == (2 if whole else len(reads) + 1) and not offs.any() and len(v) == len(c) == 0, name
    case = dict(kind="nthash", pk=dict(k=21), reads=[SC.rand_read(np.random.default_rng(3), 90)] * 4)
    res, vals = check_reads(engine, oracle, case, (2**31 - 1,))  # everything filtered
    assert len(fetch_counted(res, True, 2**31 - 1)[1]) == 0 and len(vals[0]) == 70


# ---- re-use ----
def test_reuse_between_counted_and_plain_calls(engine, oracle):
    rng = np.random.default_rng(5)
    p = dict(kind="nthash", pk=dict(k=21))
    large = sketch(engine, p, [SC.rand_read(rng, int(rng.integers(100, 300))) for _ in range(700)] * 2)
    small = sketch(engine, p, [SC.rand_read(rng, int(rng.integers(0, 60))) for _ in range(200)] * 2)
    into = S.Sets(engine, None)
    ptrs = []
    for i, (res, whole, scale) in enumerate([(large, True, 1), (small, False, 3), (large, False, 3), (small, True, 1), (large, True, 2)]):
        got = fetch_counted(res, whole, scale, into=into)
        fresh = fetch_counted(res, whole, scale)
        equal(got, fresh, ("re-used", i))
        cp = C.c_void_p()
        assert engine.lib.bsk_sets_counts_device(into.h, C.byref(cp)) == L.OK and cp.value
        ptrs.append((into.device(), cp.value))
        # an uncounted call into the same object: the counts are gone, the array stays
        h = into.h
        assert engine.lib.bsk_result_sets_reuse(engine.ctx, res.h, int(whole), scale, C.byref(h)) == L.OK and h.value
        into.h = h
        assert not into.counted
        assert engine.lib.bsk_sets_counts_device(into.h, C.byref(cp)) == L.OK and cp.value is None
        cnt = np.zeros(8, U32)
        assert engine.lib.bsk_sets_fetch_counts(engine.ctx, into.h, 0, 0, cnt.ctypes.data, 8) == L.ERR_ARG
        po, pv = into.fetch()
        assert np.array_equal(po, got[0]) and np.array_equal(pv, got[1])
        assert np.array_equal(into.totals(), np.diff(po))  # an uncounted object's totals are its sizes
    assert all(q == ptrs[2] for q in ptrs[2:]), ptrs  # grown for `large` per sequence, nothing moves afterwards
    # errors: the object is released, *sets is NULL
    h = into.h
    assert engine.lib.bsk_result_sets_counted(engine.ctx, large.h, 2, 1, C.byref(h)) == L.ERR_ARG and h.value is None
    into.h = None
    h = C.c_void_p()
    assert engine.lib.bsk_result_sets_counted(engine.ctx, large.h, 0, -1, C.byref(h)) == L.ERR_ARG and h.value is None
    equal(fetch_counted(small, False, 3, into=into), fetch_counted(small, False, 3), ("from NULL again",))
    into.close()


def test_fetch_counts_ranges(engine, oracle):
    rng = np.random.default_rng(13)
    case = dict(kind="kmer", pk=dict(k=4), reads=[SC.rand_read(rng, int(rng.integers(0, 90))) for _ in range(200)])
    res = sketch(engine, case)
    woffs, wvals, wc = CC.ref_counted(SC.values_of(oracle, case), 1, False)
    s = res.counted_sets()
    n, w, lib = len(woffs) - 1, woffs.astype(np.int64), engine.lib
    for first, count in ((0, 0), (1, 1), (n, 0), (17, 100), (0, n)):
        a, b = int(w[first]), int(w[first + count])
        c = np.full(b - a + 1, 77, U32)
        assert lib.bsk_sets_fetch_counts(engine.ctx, s.h, first, count, c.ctypes.data, b - a) == L.OK
        assert np.array_equal(c[:b - a], wc[a:b]) and c[b - a] == 77
        t = np.full(count + 1, 99, U64)
        assert lib.bsk_sets_totals(engine.ctx, s.h, first, count, t.ctypes.data) == L.OK and t[count] == 99
        assert np.array_equal(t[:count], CC.ref_totals((woffs, wvals, wc))[first:first + count])
        if b > a:
            assert lib.bsk_sets_fetch_counts(engine.ctx, s.h, first, count, c.ctypes.data, b - a - 1) == L.ERR_ARG
    c = np.zeros(len(wc) + 1, U32)
    for first, count in ((0, n + 1), (n + 1, 0), (2**64 - 1, 2)):
        assert lib.bsk_sets_fetch_counts(engine.ctx, s.h, first, count, c.ctypes.data, len(c)) == L.ERR_ARG
        assert lib.bsk_sets_totals(engine.ctx, s.h, first, count, c.ctypes.data) == L.ERR_ARG
    s.close()
