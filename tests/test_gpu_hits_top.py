"""GPU: bsk_hits_top -- the n best hits of every query -- on every branch of search.hip's reduction.

The expected values are NumPy's alone: ref_search (tests/search_cases.py) gives the hits, np.lexsort((target, -shared)) inside
every query and a cut at n give the best.  The search's own hits are compared with ref_search first, so a wrong search cannot
excuse a wrong reduction; then every offset, target and shared count of the reduction is compared, and bsk_hits_plan must name
the branch the case was written for with exactly the number of queries NumPy puts on it."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from bio_amd import _lib as L
from tests import search_cases as SC
from tests.search_cases import collection, ref_search, ref_top

pytestmark = pytest.mark.gpu
U64 = np.uint64
# search.hip's named caps
TOP_GROUP = 16       # hits a group of 16 lanes ranks in registers
TOP_SELECT_N = 16    # the largest n taken by rounds of a wave-wide maximum
TOP_LDS_KEYS = 1024  # keys one wavefront sorts in LDS
NS = (1, 2, 3, 16, 17, 64, 1024, 1025, 2048, 2049)


@functools.lru_cache(None)
def one_pass():
    """how many items one pass of each capped grid of bsk_hits_top covers on device 0 (grid_for in sets_internal.hpp)"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipDeviceGetAttribute.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
    v = C.c_int()
    assert hip.hipDeviceGetAttribute(C.byref(v), 63, 0) == 0  # hipDeviceAttributeMultiprocessorCount
    cus = v.value
    assert cus > 0
    # queries: k_top_group (32 blocks x 16 per CU), k_top_select / k_top_lds (8 blocks x 4 waves x 64), k_top_classes and k_top_list
    # (8 blocks x 256); sort-path queries: k_top_emit (16 blocks x 4 waves); hits: k_top_place (16 x 256), k_top_maxshared (8 x 256)
    return dict(cus=cus, group=cus * 512, wave=cus * 2048, classes=cus * 2048, emit=cus * 64, place=cus * 4096, maxshared=cus * 2048)


def branches(o, n):
    """the number of queries on each branch, by the hit counts alone"""
    c = np.diff(o).astype(np.int64)
    group = int(((c >= 1) & (c <= TOP_GROUP)).sum())
    if n <= TOP_SELECT_N:
        return dict(group=group, kernel="k_top_select", wave=int((c > TOP_GROUP).sum()), sort=0, sort_hits=0)
    big = c > TOP_LDS_KEYS
    return dict(group=group, kernel="k_top_lds", wave=int(((c > TOP_GROUP) & ~big).sum()), sort=int(big.sum()), sort_hits=int(c[big].sum()))


def parse_plan(top):
    pl = top.plan()
    m = re.fullmatch(r"bsk_hits_top n = (\d+): k_top_group (\d+) queries \(<= 16 hits\); (k_top_select|k_top_lds) (\d+) queries; "
                     r"sort path: (\d+) queries, (\d+) hits", pl["plan"])
    assert m, pl
    got = dict(group=int(m.group(2)), kernel=m.group(3), wave=int(m.group(4)), sort=int(m.group(5)), sort_hits=int(m.group(6)))
    assert pl["n_large_queries"] == got["sort"]
    return int(m.group(1)), got


def searched(engine, tg, qs, **kw):
    """the search's hits, checked against ref_search -> (hits, (offsets, target, shared))"""
    ix = engine.sets_from_arrays(*tg).index()
    hits = ix.search(engine.sets_from_arrays(*qs), **kw)
    want = ref_search(*tg, *qs, kw.get("min_shared", 1), kw.get("min_query_cov", 0.0), kw.get("min_target_cov", 0.0))
    o, t, s = hits.fetch()
    assert np.array_equal(o, want[0]) and np.array_equal(t, want[1]) and np.array_equal(s, want[2]), "the search itself"
    return hits, want


def check_top(hits, want, n, reuse=None):
    top = hits.top(n, reuse=reuse)
    eo, et, es = ref_top(*want, n)
    o, t, s = top.fetch()
    assert np.array_equal(o, eo), ("offsets", n)
    assert np.array_equal(t, et), ("targets", n)
    assert np.array_equal(s, es), ("shared", n)
    assert top.info() == dict(n_queries=len(eo) - 1, n_hits=int(eo[-1]))
    got_n, got = parse_plan(top)
    assert got_n == n and got == branches(want[0], n), (n, got, branches(want[0], n))
    return top, got


def all_ns(want):
    return NS + (int(np.diff(want[0]).max()) + 5,)


# ---- the existing generators ----
@pytest.mark.parametrize("case", ["posting_edge", "boundary", "edge_large", "s2"])
def test_generated_cases(engine, case):
    """posting_edge_case (hit counts 1 .. 5 000 and runs of 2 048), boundary_case (half of the queries beyond the search's LDS budget),
    edge_large_case (2 049 and more hits per query), s2_case (2 000 sets all against all: 2 000 hits per query); every n of the list
    and one above the largest hit count, where the result is a re-ordering of all hits"""
    if case == "s2":
        tg = qs = SC.s2_case(n_sets=2000, size=600, pool=60_000)
    else:
        tg, qs, _ = {"posting_edge": SC.posting_edge_case, "boundary": lambda: SC.boundary_case(40, 40), "edge_large": SC.edge_large_case}[case]()
    hits, want = searched(engine, tg, qs)
    c = np.diff(want[0]).astype(np.int64)
    if case == "s2":
        assert len(c) == 2000 and c.min() > 1900
    seen = dict(select=0, lds=0, sort=0, group=0)
    for n in all_ns(want):
        top, got = check_top(hits, want, n)
        seen["group"] += got["group"]
        seen["select" if got["kernel"] == "k_top_select" else "lds"] += got["wave"]
        seen["sort"] += got["sort"]
        if n > c.max():  # every hit, re-ordered
            assert top.info()["n_hits"] == len(want[1])
    assert seen["select"] and seen["sort"], seen
    if case == "posting_edge":
        assert seen["group"] and seen["lds"], seen


# ---- crafted hit counts and orders ----
def crafted(counts, kind, seed=7):
    """one query per entry of counts with exactly that many hits.  kind 'tie': every hit shares one value (order = ascending
    target); 'differ': hit j of a query shares a number of values no other hit of it shares; 'mixed': shared counts 1 .. 3"""
    rng = np.random.default_rng(seed)
    T = max(max(counts), 1) + 37
    tv, tt, queries = [], [], []
    nxt = 1 << 33
    for c in counts:
        tg_ids = rng.permutation(T)[:c]
        if kind == "tie":
            shared = np.ones(c, np.int64)
        elif kind == "differ":
            shared = rng.permutation(c) + 1
        else:
            shared = rng.integers(1, 4, c)
        # value i of the query is held by the targets whose shared count exceeds i
        m = int(shared.max()) if c else 0
        vals = nxt + 2 * np.arange(m + 1)  # (one more value that nobody holds)
        nxt += 2 * (m + 1) + 10
        for i in range(m):
            hold = tg_ids[shared > i]
            tv.append(np.full(len(hold), vals[i], U64))
            tt.append(hold)
        queries.append(vals)
    tv, tt = np.concatenate(tv), np.concatenate(tt)
    order = np.lexsort((tv, tt))
    t_offs = np.zeros(T + 1, U64)
    t_offs[1:] = np.cumsum(np.bincount(tt, minlength=T))
    return (t_offs, tv[order]), collection(queries)


CAPS = (0, 1, TOP_GROUP - 1, TOP_GROUP, TOP_GROUP + 1, 63, 64, 65, TOP_LDS_KEYS - 1, TOP_LDS_KEYS, TOP_LDS_KEYS + 1)


@pytest.mark.parametrize("kind", ["tie", "mixed"])
def test_hit_counts_around_every_cap(engine, kind):
    """queries of 0, 1, 15, 16, 17 (the group of 16 lanes), 63, 64, 65 (one key per lane), 1 023, 1 024 and 1 025 hits (the LDS sort's
    keys), in both orders and repeated; n on both sides of TOP_SELECT_N and of every count"""
    counts = list(CAPS) + list(CAPS[::-1]) + [TOP_GROUP + 1] * 3 + [TOP_LDS_KEYS + 1] * 2
    tg, qs = crafted(counts, kind)
    hits, want = searched(engine, tg, qs)
    assert list(np.diff(want[0])) == counts
    if kind == "tie":
        assert (want[2] == 1).all()
    for n in (1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 1026):
        _, got = check_top(hits, want, n)
        b = branches(want[0], n)
        assert b["group"] == 2 * 3 and b["wave"] > 0 and (b["sort"] == 4 or n <= TOP_SELECT_N)


def test_all_shared_counts_differ(engine):
    """inside every query no two hits share the same number of values: the order is the shared counts', descending, whatever the
    targets are; 17, 40, 64, 65 and 300 hits by rounds of a maximum and by the LDS sort, 1 100 by the sort path"""
    counts = [3, 17, 40, 64, 65, 300, 1100, 16]
    tg, qs = crafted(counts, "differ")
    hits, want = searched(engine, tg, qs)
    assert list(np.diff(want[0])) == counts
    for n in (1, 5, 16, 17, 299, 300, 1100, 5000):
        top, got = check_top(hits, want, n)
        o, t, s = top.fetch()
        for q in range(len(counts)):
            sq = s[int(o[q]):int(o[q + 1])].astype(np.int64)
            assert (np.diff(sq) == -1).all() and (len(sq) == 0 or sq[0] == counts[q])


def test_queries_without_hits_first_last_and_in_runs(engine):
    counts = [0, 0, 5, 0, 0, 0, 0, 0, 20, 1, 0, 2000, 0, 0, 0, 17, 0, 0]
    tg, qs = crafted(counts, "mixed", seed=11)
    hits, want = searched(engine, tg, qs)
    assert list(np.diff(want[0])) == counts
    for n in (1, 3, 17, 2000, 2001):
        check_top(hits, want, n)
    # nothing but queries without hits, and no queries at all
    ix = engine.sets_from_arrays(*tg).index()
    for qs0 in (collection([[1], [2], []]), (np.zeros(1, U64), np.zeros(0, U64))):
        h0 = ix.search(engine.sets_from_arrays(*qs0))
        nq = len(qs0[0]) - 1
        for n in (1, 17):
            top = h0.top(n)
            assert top.info() == dict(n_queries=nq, n_hits=0)
            o, t, s = top.fetch()
            assert np.array_equal(o, np.zeros(nq + 1, U64)) and len(t) == 0 and len(s) == 0
            assert parse_plan(top)[1] == dict(group=0, kernel="k_top_select" if n <= 16 else "k_top_lds", wave=0, sort=0, sort_hits=0)


def test_thresholds_change_the_input_not_the_order(engine):
    tg, qs, _ = SC.posting_edge_case()
    hits, want = searched(engine, tg, qs, min_shared=2)
    for n in (1, 17):
        check_top(hits, want, n)


def test_top_object_is_reused_and_bad_arguments(engine):
    """*top from a larger result to a smaller one and back: the arrays are kept, the numbers are each call's own"""
    tg, qs = crafted([2000, 30, 0, 7, 1500], "mixed", seed=13)
    hits, want = searched(engine, tg, qs)
    small_tg, small_qs = crafted([3, 0, 18], "tie", seed=17)
    small_hits, small_want = searched(engine, small_tg, small_qs)
    top, _ = check_top(hits, want, 3000)
    ptr = top.device()
    for h, w, n in ((small_hits, small_want, 2), (hits, want, 17), (small_hits, small_want, 100), (hits, want, 3000), (hits, want, 1)):
        t2, _ = check_top(h, w, n, reuse=top)
        assert t2 is top and top.device() == ptr  # the first call sized the arrays for the largest
    lib = engine.lib
    keep = top.h
    assert lib.bsk_hits_top(engine.ctx, hits.h, 0, C.byref(keep)) == L.ERR_ARG and keep.value == top.h.value  # n == 0: *top as it was
    same = C.c_void_p(hits.h.value)
    assert lib.bsk_hits_top(engine.ctx, hits.h, 1, C.byref(same)) == L.ERR_ARG  # *top == h
    check_top(hits, want, 2, reuse=top)  # and the object still works
    from bio_amd import sketches as S
    other = S.Engine(0)
    fresh = C.c_void_p()
    assert lib.bsk_hits_top(other.ctx, hits.h, 1, C.byref(fresh)) == L.ERR_ARG and not fresh.value  # the hits of another context
    other.close()


def test_more_queries_than_one_pass_of_every_grid(engine):
    """more queries than k_top_group, k_top_select / k_top_lds (64 queries per wavefront step) and k_top_classes cover in one pass, with
    every kind of query also behind the first pass"""
    lim = one_pass()
    nq = max(lim["group"], lim["wave"], lim["classes"]) + 4097
    T = 64
    tsets = [[100 + j] + ([7] if j < 17 else []) + ([9] if j < 40 else []) + [11 + (j % 3)] for j in range(T)]
    tg = collection(tsets)
    i = np.arange(nq)
    kind = i % 4  # 0: no hit; 1: two values of one target each; 2: three values, two of them of one target; 3: now and then 17 or 40 + hits
    a, b = 100 + (i * 7) % T, 100 + (i * 13 + 5) % T
    rows = [np.stack([a, b], 1)[kind == 1], np.stack([a, b, 11 + i % 3], 1)[kind == 2]]
    v = np.full((nq, 3), 5, np.int64)  # 5: a miss
    v[kind == 1, :2] = rows[0]
    v[kind == 2] = rows[1]
    dense = (kind == 3) & (i % 101 == 3)
    v[dense] = np.stack([np.full(dense.sum(), 7), np.full(dense.sum(), 9), 100 + i[dense] % T], 1)
    v[kind == 3, 0] = np.where(dense[kind == 3], 7, 5)
    v.sort(1)
    keepv = np.ones_like(v, bool)
    keepv[:, 1:] = v[:, 1:] != v[:, :-1]
    q_offs = np.zeros(nq + 1, U64)
    q_offs[1:] = np.cumsum(keepv.sum(1))
    qs = (q_offs, v[keepv].astype(U64))
    hits, want = searched(engine, tg, qs)
    c = np.diff(want[0]).astype(np.int64)
    first = max(lim["group"], lim["wave"])
    assert (c[first:] == 0).any() and ((c[first:] >= 1) & (c[first:] <= TOP_GROUP)).any() and (c[first:] > TOP_GROUP).any(), "every kind behind the first pass"
    for n in (1, 3, 17, 41):
        check_top(hits, want, n)


def test_more_sort_path_queries_than_one_pass(engine):
    """more queries of 1 025 hits than k_top_emit covers in one pass, and with them more hits than one pass of k_top_place and
    k_top_maxshared; a few queries of other sizes between them"""
    lim = one_pass()
    n_big = lim["emit"] + 9
    rng = np.random.default_rng(19)
    T = 1400
    K = 12  # values held by 1 025 targets each (one shared by every big query's pair with them), and a second value for a third of the targets
    tt, tv = [], []
    for k in range(K):
        hold = rng.permutation(T)[:TOP_LDS_KEYS + 1]
        tt += [hold, hold[::3]]
        tv += [np.full(len(hold), 1000 + 2 * k, U64), np.full(len(hold[::3]), 1001 + 2 * k, U64)]
    tt, tv = np.concatenate(tt), np.concatenate(tv)
    order = np.lexsort((tv, tt))
    t_offs = np.zeros(T + 1, U64)
    t_offs[1:] = np.cumsum(np.bincount(tt, minlength=T))
    tg = (t_offs, tv[order])
    k = rng.integers(0, K, n_big)
    queries = np.stack([1000 + 2 * k, 1001 + 2 * k], 1).astype(U64)
    q_offs = np.arange(n_big + 1, dtype=U64) * U64(2)
    qv = queries.reshape(-1)
    # (queries of one value: 342 hits, the LDS sort, in the middle and at the end)
    extra = np.array([1001, 1003], U64)
    q_offs = np.concatenate([q_offs, q_offs[-1] + np.arange(1, 3, dtype=U64)])
    qs = (q_offs, np.concatenate([qv, extra]))
    hits, want = searched(engine, tg, qs)
    c = np.diff(want[0]).astype(np.int64)
    assert (c[:n_big] == TOP_LDS_KEYS + 1).all() and int(c.sum()) > max(lim["place"], lim["maxshared"]) and n_big > lim["emit"]
    for n in (17, 1025):
        _, got = check_top(hits, want, n)
        assert got["sort"] == n_big and got["wave"] == 2
    check_top(hits, want, 2)
