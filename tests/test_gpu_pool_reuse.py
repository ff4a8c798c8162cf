"""The grow-only allocator behind the context's pool and the objects' own arrays (host_types.hpp: ctx_pool, grow_array), through the
entries that use it, family by family on ONE context of this module's own:

    the family's empty input (its first call: the family's pool slots are untouched) -> small -> large -> empty -> small

Small is 3 sets of at most 5 values.  Large is sized from the byte formulas of the entry's host code, restated beside each family, so
that every pooled buffer whose size depends on the input must regrow: a buffer taken for `b` bytes holds b + b / 4 + 256 (`regrows`).
The scan's parts -- (n + 2047) / 2048 + 2 words -- only regrow past 33 blocks, so the families that scan their sets take some 70 000
of them.  Not derived: the sort's temporary storage (rocprim's own figure), the search's staging spans (device-side sums) and the
compare's 64 bytes of figures (a constant).  Every step is checked against the case modules' references; the objects handed back in
(reuse / into) must keep their device pointers from the large call on: nothing shrinks, nothing is allocated twice."""
import ctypes as C

import numpy as np
import pytest

from bio_amd import _lib as L
from tests import compare_cases as CM
from tests import compare_counted_cases as CW
from tests import counts_cases as CC
from tests import search_cases as SR
from tests import setops_cases as SO
from tests import sets_cases as SC

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
K = 21
ORDER = ("none", "hollow", "small", "large", "none", "hollow", "small")  # none: no sets; hollow: sets without values


def regrows(small_bytes, large_bytes):
    return large_bytes > small_bytes + small_bytes // 4 + 256


def parts(n):  # sets_internal.hpp: scan_parts
    return (n + SC.SCAN_CHUNK - 1) // SC.SCAN_CHUNK + 2


def carve(*pieces):  # sets_internal.hpp: Carve -- (entries, bytes each), every piece 256-byte aligned
    return sum((max(n, 1) * size + 255) // 256 * 256 for n, size in pieces)


@pytest.fixture(scope="module")
def eng():
    from bio_amd import sketches as S
    return S.Engine(0)


def d2h(ptr, n, dt):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    a = np.empty(n, dt)
    if n:
        assert hip.hipMemcpy(a.ctypes.data, ptr, a.nbytes, 2) == 0
    return a


def rows(rng, n_sets, size, pool=None):
    """n_sets sorted sets of `size` distinct values (from `pool` if given) -> 2-D array"""
    if pool is None:
        v = np.sort(rng.integers(1, 2**63, (n_sets, size), dtype=np.int64).astype(U64), axis=1)
        assert (np.diff(v.astype(np.int64), axis=1) > 0).all()
        return v
    return np.stack([np.sort(rng.choice(pool, size, replace=False)) for _ in range(n_sets)]).astype(U64)


def shapes(rng, n_large, size_large, pool=None):
    """{name: list of sorted value arrays} of the four inputs of a family"""
    p = pool if pool is not None else np.sort(rng.integers(1, 2**63, 12, dtype=np.int64).astype(U64))
    return {"none": [], "hollow": [np.zeros(0, U64)] * 3,
            "small": [np.sort(rng.choice(p, 5, replace=False)), np.zeros(0, U64), np.sort(rng.choice(p, 3, replace=False))],
            "large": list(rows(rng, n_large, size_large, pool))}


def sets_ptrs(eng, s):
    """(offsets, values, counts) of a Sets or of a bare handle, on the device"""
    o, v, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    h = getattr(s, "h", s)
    assert eng.lib.bsk_sets_device(h, C.byref(o), C.byref(v)) == L.OK and eng.lib.bsk_sets_counts_device(h, C.byref(c)) == L.OK
    return o.value, v.value, c.value


def walk(step, ptrs):
    """step(name) runs and checks one input; ptrs() are the reused objects' device pointers, fixed from the large call on"""
    held = None
    for name in ORDER:
        step(name)
        if held is not None:
            assert ptrs() == held, name
        if name == "large":
            held = ptrs()
    assert held is not None and all(p for p in held)


# ---- result to sets (sets.hip: sets_build), with bsk_result_compact and the two fetches on the same results ----
def kmer_results(eng, oracle):
    """KMER results by input name -> (result, every read's values in order); hollow: reads too short for one k-mer (a batch holds a read)"""
    rng = np.random.default_rng(601)
    reads = {"hollow": ["ACGT", "", "AC"], "small": [SC.rand_read(rng, K + 4), SC.rand_read(rng, K - 1), SC.rand_read(rng, K + 2)]}
    out = {}
    for name, rd in reads.items():
        out[name] = (eng.run(eng.batch(rd), eng.params(L.KMER, K)), [np.asarray(SC.oracle_values(oracle, "kmer", dict(k=K), q), U64) for q in rd])
    rd, vals = CC.kmer_stream(oracle, 70_000, K)  # one value a read
    out["large"] = (eng.run(eng.batch(rd), eng.params(L.KMER, K)), vals.reshape(-1, 1))
    return out


def test_result_to_sets(eng, oracle):
    res = kmer_results(eng, oracle)
    n_s, n_l, N_s, N_l = 3, 70_000, sum(len(v) for v in res["small"][1]), 70_000
    assert N_s <= 15
    for small, large in (((n_s + 2) * 8, (n_l + 2) * 8), (parts(n_s) * 8, parts(n_l) * 8), (N_s * 8, N_l * 8), (N_s, N_l), (N_s * 4, N_l * 4), ((N_s + 1) * 8, (N_l + 1) * 8),
                         (parts(N_s) * 8, parts(N_l) * 8), ((N_s // CC.read_chunk() + 2) * 8, (N_l // CC.read_chunk() + 2) * 8)):
        assert regrows(small, large), (small, large)  # offsets, their scan, values (in, sorted), heads, flags, positions, their scan, run lengths
    objs = [C.c_void_p(), C.c_void_p(), C.c_void_p()]  # per sequence (k_sets_rows), whole batch (the sort), counted per sequence (the sort + run lengths)
    from bio_amd import sketches as S

    def step(name):
        if name == "none":
            return  # (a batch holds at least one read)
        r, per = res[name]
        for i, (whole, counted) in enumerate(((False, False), (True, False), (False, True))):
            call = eng.lib.bsk_result_sets_counted if counted else eng.lib.bsk_result_sets_reuse
            assert call(eng.ctx, r.h, int(whole), 1, C.byref(objs[i])) == L.OK and objs[i].value
            s = S.Sets(eng, objs[i])
            try:
                offs, vals = s.fetch()
                if name == "large":
                    want = CC.ref_counted_rows(per, 1, whole) if counted else SC.ref_sets_rows(per, 1, whole)
                else:
                    want = CC.ref_counted(per, 1, whole) if counted else SC.ref_sets(per, 1, whole)
                assert np.array_equal(offs, want[0]) and np.array_equal(vals, want[1]), (name, whole, counted)
                assert s.counted == counted and (not counted or np.array_equal(s.fetch_counts(), want[2])), (name, whole)
            finally:
                s.h = None  # (the handle stays this test's)

    try:
        walk(step, lambda: sets_ptrs(eng, objs[0])[:2] + sets_ptrs(eng, objs[1])[:2] + sets_ptrs(eng, objs[2]))
    finally:
        for o in objs:
            eng.lib.bsk_sets_release(o)


def minimizer_results(eng, oracle):
    """the same for a kind with positions -> (result, per read (hash, pos, strand))"""
    rng = np.random.default_rng(607)
    reads = {"hollow": ["ACGT", "", "AC"], "small": [SC.rand_read(rng, 33) for _ in range(3)], "large": [SC.rand_read(rng, 150) for _ in range(100)]}
    out = {}
    for name, rd in reads.items():
        per = [oracle.minimizer(q, K, 11, False, closed=True)[:3] if len(q) >= K + 10 else (np.zeros(0, U64),) * 3 for q in rd]
        out[name] = (eng.run(eng.batch(rd), eng.params(L.MINIMIZER, K, w=11)), per)
    return out


def test_compact_and_fetches(eng, oracle):
    km, mn = kmer_results(eng, oracle), minimizer_results(eng, oracle)
    T_s, T_l = sum(len(h) for h, _, _ in mn["small"][1]), sum(len(h) for h, _, _ in mn["large"][1])
    assert T_s <= 9
    for small, large in (((3 + 2) * 8, (70_000 + 2) * 8), (parts(3) * 8, parts(70_000) * 8), ((3 + 2) * 12, (70_000 + 2) * 12), (3 * 8, 100 * 8),  # offsets (compact, narrow, fetch), the scan
                         ((T_s + 1) * 8, (T_l + 1) * 8), ((T_s + 1) * 4, (T_l + 1) * 4), ((T_s + 1) * 2, (T_l + 1) * 2), (T_s * 8, T_l * 8), (T_s * 4, T_l * 4)):  # hashes, positions
        assert regrows(small, large), (small, large)
    last = {}

    def check(name, r, offs, hash_, pos, strand):
        n, T = len(offs) - 1, len(hash_)
        o, _, h, p = r.fetch()
        assert np.array_equal(o, offs) and np.array_equal(h, hash_), name
        o2, _, h2, p2 = r.fetch_narrow()
        assert np.array_equal(o2.astype(U64), offs) and np.array_equal(h2, hash_), name
        o0, _, h0, _ = r.fetch_narrow(0, 0)  # count == 0
        assert list(o0) == [0] and len(h0) == 0
        po, ph, pp, nt = r.compact()
        assert nt == T and np.array_equal(d2h(po, n + 1, U64), offs) and np.array_equal(d2h(ph, T, U64), hash_), name
        if pos is None:
            assert p is None and p2 is None and pp is None
        else:
            assert np.array_equal(p & L.POS_MASK, pos) and np.array_equal(p >> 31, strand), name
            assert np.array_equal((p2 & 0x7FFF).astype(U32), pos) and np.array_equal((p2 >> 15).astype(U32), strand), name
            assert np.array_equal(d2h(pp, T, U32), p), name
        last["ptrs"] = (po, ph) + ((pp,) if pos is not None else ())

    def kmer_step(name):
        if name == "none":
            return
        r, per = km[name]
        offs = np.concatenate([[0], np.cumsum([len(v) for v in per])]).astype(U64)
        check(name, r, offs, np.concatenate(list(per)).astype(U64), None, None)

    def minimizer_step(name):
        if name == "none":
            return
        r, per = mn[name]
        offs = np.concatenate([[0], np.cumsum([len(h) for h, _, _ in per])]).astype(U64)
        cat = [np.concatenate([np.asarray(x[i]) for x in per]) for i in range(3)]
        check(name, r, offs, cat[0].astype(U64), cat[1].astype(U32), cat[2].astype(U32))

    walk(kmer_step, lambda: last["ptrs"])
    walk(minimizer_step, lambda: last["ptrs"])


# ---- set operations (setops.hip) ----
def test_set_operations(eng):
    rng = np.random.default_rng(613)
    caps = SO.read_caps()
    pool = np.sort(rng.integers(1, 2**63, 400, dtype=np.int64).astype(U64))
    a, b = shapes(rng, 100, 40, pool), shapes(rng, 100, 40, pool)
    a["large"].append(rows(rng, 1, 700)[0])  # one pair of the tiled path: its own pooled buffer, which the small calls never take
    b["large"].append(rows(rng, 1, 700)[0])
    assert 1400 > caps["SO_WAVE_CAP"]
    n_s, n_l = 3, 101
    N_s, N_l = sum(len(s) for s in a["small"]), sum(len(s) for s in a["large"])
    pairs = lambda n: carve((n + 1, 8), (n + 1, 8), (n + 1, 8), (n, 8), (parts(n), 8), (8, 8), (n, 4))  # op_impl's carve
    assert regrows(pairs(n_s), pairs(n_l))
    groups = lambda g: carve((g + 1, 8), (g + 1, 8), (8, 8))  # reduce_impl's two carves and its sorted copy
    assert regrows(groups(2), groups(n_l - 1)) and regrows(N_s * 8, N_l * 8)
    assert regrows(carve((N_s + 1, 8), (parts(N_s), 8), (N_s, 4)), carve((N_l + 1, 8), (parts(N_l), 8), (N_l, 4)))
    out, outc, red = [eng.sets_from_arrays(np.zeros(1, U64), np.zeros(0, U64)) for _ in range(3)]

    def step(name):
        ha, hb = SO.collection(a[name]), SO.collection(b[name])
        sa, sb = eng.sets_from_arrays(*ha), eng.sets_from_arrays(*hb)
        for op in SO.OPS:
            got, want = sa.op(sb, op, into=out).fetch(), SO.ref_op(ha, hb, op)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, op)
        ca, cb = (ha[0], ha[1], CC.counts_a(ha[0])), (hb[0], hb[1], CC.counts_b(hb[0]))
        r = eng.sets_from_arrays_counted(*ca).add(eng.sets_from_arrays_counted(*cb), into=outc)
        want = CC.ref_op(ca, cb, CC.ADD)
        assert all(np.array_equal(x, y) for x, y in zip(r.fetch() + (r.fetch_counts(),), want)), name
        n = len(a[name])
        go = np.array([0], U64) if n == 0 else np.concatenate([np.arange(n - 1), [n]]).astype(U64)  # the last two sets share a group
        got, want = sa.reduce(go, 1, into=red).fetch(), SO.ref_reduce(ha, go, 1)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name

    walk(step, lambda: out.device() + sets_ptrs(eng, outc) + red.device())


# ---- counted filter (counts.hip) and bottom-n (compare.hip): their scans want more than 33 blocks of values / of sets ----
def test_counted_filter(eng):
    rng = np.random.default_rng(617)
    s = shapes(rng, 1850, 40)
    N_s, N_l = 8, 1850 * 40
    for small, large in ((N_s * 4, N_l * 4), ((N_s + 1) * 8, (N_l + 1) * 8), ((parts(N_s) + 8) * 8, (parts(N_l) + 8) * 8)):  # flags, positions, figures + the scan
        assert regrows(small, large), (small, large)
    out = eng.sets_from_arrays(np.zeros(1, U64), np.zeros(0, U64))

    def step(name):
        offs, vals = SO.collection(s[name])
        c = CC.counts_a(offs)
        got = eng.sets_from_arrays_counted(offs, vals, c).filter_counts(2, 5, into=out)
        want = CC.ref_filter((offs, vals, c), 2, 5)
        assert all(np.array_equal(x, y) for x, y in zip(got.fetch() + (got.fetch_counts(),), want)), name

    walk(step, lambda: sets_ptrs(eng, out))


def test_bottom(eng):
    rng = np.random.default_rng(619)
    s = shapes(rng, 74_000, 3)
    assert regrows((parts(3) + 8) * 8, (parts(74_000) + 8) * 8)  # figures + the scan of the sets' kept sizes
    out = eng.sets_from_arrays(np.zeros(1, U64), np.zeros(0, U64))

    def step(name):
        offs, vals = SO.collection(s[name])
        c = CC.counts_a(offs)
        got = eng.sets_from_arrays_counted(offs, vals, c).bottom(2, into=out)
        want = CM.collection(CM.ref_bottom(s[name], 2))
        assert np.array_equal(got.fetch()[0], want[0]) and np.array_equal(got.fetch()[1], want[1]), name
        assert np.array_equal(got.fetch_counts(), np.concatenate(CM.ref_bottom(SO.split(offs, c), 2) + [np.zeros(0, U32)])), name

    walk(step, lambda: sets_ptrs(eng, out))


# ---- compare and compare_counted (compare.hip): the object's arrays hold one cell a pair ----
def test_compares(eng):
    from bio_amd import sketches as S
    rng = np.random.default_rng(631)
    s = shapes(rng, 40, 40, np.sort(rng.integers(1, 2**63, 400, dtype=np.int64).astype(U64)))
    assert regrows(3 * 3 * 4, 40 * 40 * 4) and regrows(3 * 3 * 8, 40 * 40 * 8)
    plain, weighted = S.Compare(eng), S.Compare(eng)

    def step(name):
        A = s[name]
        offs, vals = SO.collection(A)
        counts = CC.counts_a(offs)
        sa, sc = eng.sets_from_arrays(offs, vals), eng.sets_from_arrays_counted(offs, vals, counts)
        for limit in (0, 4):
            c, w = sa.compare(limit=limit, reuse=plain), sc.compare_counted(limit=limit, reuse=weighted)
            assert c.info() == w.info() == dict(n_a=len(A), n_b=len(A), limit=limit), name
            if not A:
                continue  # no pairs: nothing to fetch
            want = CM.ref_compare(A, A, limit)
            assert np.array_equal(c.fetch()[0], want[0]) and np.array_equal(c.fetch()[1], want[1]), (name, limit)
            CA = SO.split(offs, counts)
            want = CW.ref_compare(A, CA, A, CA, limit)
            assert all(np.array_equal(x, y) for x, y in zip(w.fetch() + w.fetch_weights(), want)), (name, limit)

    def ptrs():
        pd, pm = C.c_void_p(), C.c_void_p()
        assert eng.lib.bsk_compare_weights_device(weighted.h, C.byref(pd), C.byref(pm)) == L.OK
        return plain.device() + weighted.device() + (pd.value, pm.value)

    walk(step, ptrs)


# ---- index search and top-n (search.hip) ----
def test_search_and_top(eng):
    from bio_amd import sketches as S
    rng = np.random.default_rng(641)
    pool = np.sort(rng.integers(1, 2**63, 400, dtype=np.int64).astype(U64))
    t_offs, t_vals = SR.collection(list(rows(rng, 100, 40, pool)))
    index = eng.sets_from_arrays(t_offs, t_vals).index()
    q = shapes(rng, 100, 40, pool)
    q["large"].append(np.sort(rng.choice(pool, 300, replace=False)))  # a query of the large path: its own two pooled buffers
    sums = SR.posting_sums(t_offs, t_vals, *SR.collection(q["large"]))
    assert sums[-1] > SR.SR_CAP and (sums[:-1] <= SR.SR_CAP).all(), sums.max()
    nq_s, nq_l, nv_s, nv_l = 3, 101, 8, 100 * 40 + 300
    per_query = lambda n: carve((n, 8), (n + 1, 8), (n, 8), (n + 1, 8), (n + 1, 8), (parts(n), 8), (8, 8), (n, 4))  # search_impl's carve
    assert regrows(per_query(nq_s), per_query(nq_l)) and regrows(nv_s * 8, nv_l * 8)
    hits, top = S.Hits(eng), S.Hits(eng)

    def step(name):
        q_offs, q_vals = SR.collection(q[name])
        h = index.search(eng.sets_from_arrays(q_offs, q_vals), reuse=hits)
        want = SR.ref_search(t_offs, t_vals, q_offs, q_vals)
        got = h.fetch()
        assert all(np.array_equal(x, y) for x, y in zip(got, want)), name
        assert h.plan()["n_large_queries"] == (1 if name == "large" else 0), name
        want = SR.ref_top(*want, 2)
        assert all(np.array_equal(x, y) for x, y in zip(h.top(2, reuse=top).fetch(), want)), name

    walk(step, lambda: hits.device() + top.device())
