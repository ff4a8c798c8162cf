"""The in/out object slot of the sets-side entries (bsk_sets **out, bsk_hits **hits, bsk_compare **cmp, bsk_clusters **out; host_types.hpp: take_over;
include/biosketch.h "The result slot"), entry by entry through raw ctypes on ONE context, on 3 sets of at most 5 values:

  1. an empty slot yields an object; the same call with that object in the slot yields the same handle and the same device pointers;
  2. an argument error the entry checks BEFORE it takes the slot over -- a bad op, n == 0, min_members == 0, min_count == 0, *out equal
     to the input, reserved != 0, an unknown flag of the neighbours, a host row that does not ascend, an unknown cluster method; for the two compares, whose checks of that kind are the null and the context ones only, a null `b` --
     returns BSK_ERR_ARG, leaves the handle where it is and the earlier result's contents intact;
  3. an object of ANOTHER context in the slot (made by a second engine on the same device; of the slot's own type) returns BSK_ERR_ARG
     and is left alone.  For bsk_result_sets_reuse / _counted this is the only error a re-used slot survives;
  4. those two release a re-used object on every other error: a bad scope returns BSK_ERR_ARG and the slot comes back NULL;
  5. the two compares take the slot BEFORE their size limits: more than 2^31 cells (65 536 x 32 769 sets without a value) return
     BSK_ERR_UNSUPPORTED, and a re-used bsk_compare is released, the slot NULL.

The 2^32 limits of the other entries would take tens of gigabytes of offsets and are not run; they stand in front of take_over in the code.
No case here makes the device fail."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest

from bio_amd import _lib as L
from tests import cluster_cases as CL
from tests import compare_cases as CM
from tests import compare_counted_cases as CW
from tests import counts_cases as CC
from tests import neighbor_cases as NC
from tests import neighbor_counted_cases as NW
from tests import search_cases as SR
from tests import setops_cases as SO
from tests import sets_cases as SC

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
K = 21
SETS = ("bsk_sets_op", "bsk_sets_op_counted", "bsk_sets_reduce", "bsk_sets_filter_counts", "bsk_sets_bottom")
COMPARES = ("bsk_sets_compare", "bsk_sets_compare_counted")
SEARCHES = ("bsk_index_search", "bsk_hits_top")
RESULTS = ("bsk_result_sets_reuse", "bsk_result_sets_counted")
GRAPHS = ("bsk_sets_neighbors", "bsk_sets_neighbors_counted", "bsk_hits_from_host", "bsk_hits_cluster")
ENTRIES = SETS + COMPARES + SEARCHES + RESULTS + GRAPHS


def fetch_sets(eng, h):
    """(offsets, values, counts or None) of a bare bsk_sets handle"""
    from bio_amd import sketches as S
    s = S.Sets(eng, h)
    try:
        return s.fetch() + ((s.fetch_counts(),) if s.counted else (None,))
    finally:
        s.h = None  # (the handle stays the test's)


def sets_ptrs(eng, h):
    o, v, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert eng.lib.bsk_sets_device(h, C.byref(o), C.byref(v)) == L.OK and eng.lib.bsk_sets_counts_device(h, C.byref(c)) == L.OK
    return o.value, v.value, c.value


def fetch_hits(eng, h):
    """(offsets, target, shared) and, where the hits carry them, (total,) and (dot, min_sum) behind them"""
    from bio_amd import sketches as S
    x = S.Hits(eng)
    x.h = h
    try:
        return x.fetch() + ((x.fetch_totals(),) if x.has_totals() else ()) + (x.fetch_weights() if x.has_weights() else ())
    finally:
        x.h = None


def fetch_clusters(eng, h):
    from bio_amd import sketches as S
    x = S.Clusters(eng)
    x.h = h
    try:
        return x.fetch()
    finally:
        x.h = None


def clusters_ptrs(eng, h):
    p = [C.c_void_p() for _ in range(4)]
    assert eng.lib.bsk_clusters_device(h, *[C.byref(x) for x in p]) == L.OK
    return tuple(x.value for x in p)


def hits_ptrs(eng, h):
    p = [C.c_void_p() for _ in range(3)]
    assert eng.lib.bsk_hits_device(h, *[C.byref(x) for x in p]) == L.OK
    return tuple(x.value for x in p)


def fetch_compare(eng, h):
    """(shared, total) and, from a weighted object, (dot, min_sum) behind them"""
    from bio_amd import sketches as S
    x = S.Compare(eng)
    x.h = h
    try:
        return x.fetch() + (x.fetch_weights() if x.weighted else ())
    finally:
        x.h = None


def compare_ptrs(eng, h):
    p = [C.c_void_p() for _ in range(4)]
    assert eng.lib.bsk_compare_device(h, C.byref(p[0]), C.byref(p[1])) == L.OK
    assert eng.lib.bsk_compare_weights_device(h, C.byref(p[2]), C.byref(p[3])) == L.OK
    return tuple(x.value for x in p)


KINDS = {  # what a slot holds -> (fetch, device pointers, the release function's name)
    "sets": (fetch_sets, sets_ptrs, "bsk_sets_release"),
    "hits": (fetch_hits, hits_ptrs, "bsk_hits_release"),
    "compare": (fetch_compare, compare_ptrs, "bsk_compare_release"),
    "clusters": (fetch_clusters, clusters_ptrs, "bsk_clusters_release"),
}


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None and w is None) or np.array_equal(g, w), (got, want)


@pytest.fixture(scope="module")
def world(oracle):
    """The one engine, its inputs, a second engine's objects, and per entry: its kind, the good call, the refused calls, the reference"""
    from bio_amd import sketches as S
    eng, other = S.Engine(0), S.Engine(0)
    lib, ctx = eng.lib, eng.ctx
    rng = np.random.default_rng(701)
    pool = np.sort(rng.integers(1, 2**63, 9, dtype=np.int64).astype(U64))
    A = [np.sort(rng.choice(pool, 5, replace=False)), np.zeros(0, U64), np.sort(rng.choice(pool, 3, replace=False))]
    B = [np.sort(rng.choice(pool, 4, replace=False)), np.sort(rng.choice(pool, 2, replace=False)), np.sort(rng.choice(pool, 5, replace=False))]
    ha, hb = SO.collection(A), SO.collection(B)
    ca, cb = ha + (CC.counts_a(ha[0]),), hb + (CC.counts_b(hb[0]),)
    sa, sb = eng.sets_from_arrays(*ha), eng.sets_from_arrays(*hb)
    sca, scb = eng.sets_from_arrays_counted(*ca), eng.sets_from_arrays_counted(*cb)
    index = sa.index()  # targets: A; queries: B
    hits = index.search(sb)
    want_hits = SR.ref_search(ha[0], ha[1], hb[0], hb[1])
    go = np.array([0, 2, 3], U64)
    reads = [SC.rand_read(rng, K + 4), SC.rand_read(rng, K - 1), SC.rand_read(rng, K + 2)]  # 5, 0 and 3 k-mers
    batch = eng.batch(reads)
    result = eng.run(batch, eng.params(L.KMER, K))
    per = [np.asarray(SC.oracle_values(oracle, "kmer", dict(k=K), q), U64) for q in reads]
    assert [len(v) for v in per] == [5, 0, 3]
    good_sp, bad_sp = L.SearchParams(1, 0, 0.0, 0.0), L.SearchParams(1, 1, 0.0, 0.0)  # (min_shared, reserved, covers)
    CA, CB = SO.split(ha[0], ca[2]), SO.split(hb[0], cb[2])
    # a second engine on the same device: one object of every kind a slot holds, and a result
    f_sets = other.sets_from_arrays(*ha)
    f_batch = other.batch(reads)
    foreign = NS(sets=f_sets, compare=f_sets.compare(), hits=f_sets.index().search(f_sets), result=other.run(f_batch, other.params(L.KMER, K)),
                 want=dict(sets=ha + (None,), compare=CM.ref_compare(A, A, 0), hits=SR.ref_search(ha[0], ha[1], ha[0], ha[1])))
    foreign.clusters = foreign.hits.cluster()
    foreign.want["clusters"] = CL.model_components(3, *foreign.want["hits"][:2])[:4]
    flag_np, cl_bad = L.NeighborParams(1, 2, 0, 0), L.ClusterParams(7, 0)  # (an unknown flag bit; an unknown method)
    g_offs, g_tgt, g_sh, g_tot = np.array([0, 2, 2, 3], U64), np.array([0, 2, 1], U32), np.array([4, 5, 6], U32), np.array([7, 8, 9], U32)
    g_unsorted = np.array([2, 0, 1], U32)
    by = lambda out: C.byref(out)
    e = {
        "bsk_sets_op": NS(kind="sets", good=lambda o: lib.bsk_sets_op(ctx, sa.h, sb.h, L.SETOP_UNION, by(o)), want=SO.ref_op(ha, hb, SO.UNION) + (None,),
                          bad=[lambda o: lib.bsk_sets_op(ctx, sa.h, sb.h, 99, by(o))], aliased=(sa, ha + (None,))),
        "bsk_sets_op_counted": NS(kind="sets", good=lambda o: lib.bsk_sets_op_counted(ctx, sca.h, scb.h, L.COUNTOP_ADD, by(o)), want=CC.ref_op(ca, cb, CC.ADD),
                                  bad=[lambda o: lib.bsk_sets_op_counted(ctx, sca.h, scb.h, 99, by(o))], aliased=(scb, cb)),
        "bsk_sets_reduce": NS(kind="sets", good=lambda o: lib.bsk_sets_reduce(ctx, sa.h, go.ctypes.data, 2, 1, by(o)), want=SO.ref_reduce(ha, go, 1) + (None,),
                              bad=[lambda o: lib.bsk_sets_reduce(ctx, sa.h, go.ctypes.data, 2, 0, by(o))], aliased=(sa, ha + (None,))),
        "bsk_sets_filter_counts": NS(kind="sets", good=lambda o: lib.bsk_sets_filter_counts(ctx, sca.h, 2, 4, by(o)), want=CC.ref_filter(ca, 2, 4),
                                     bad=[lambda o: lib.bsk_sets_filter_counts(ctx, sca.h, 0, 4, by(o))], aliased=(sca, ca)),
        "bsk_sets_bottom": NS(kind="sets", good=lambda o: lib.bsk_sets_bottom(ctx, sa.h, 2, by(o)), want=CM.collection(CM.ref_bottom(A, 2)) + (None,),
                              bad=[lambda o: lib.bsk_sets_bottom(ctx, sa.h, 0, by(o))], aliased=(sa, ha + (None,))),
        "bsk_sets_compare": NS(kind="compare", good=lambda o: lib.bsk_sets_compare(ctx, sa.h, sb.h, 0, by(o)), want=CM.ref_compare(A, B, 0),
                               bad=[lambda o: lib.bsk_sets_compare(ctx, sa.h, None, 0, by(o))]),
        "bsk_sets_compare_counted": NS(kind="compare", good=lambda o: lib.bsk_sets_compare_counted(ctx, sca.h, scb.h, 0, by(o)), want=CW.ref_compare(A, CA, B, CB, 0),
                                       bad=[lambda o: lib.bsk_sets_compare_counted(ctx, sca.h, None, 0, by(o))]),
        "bsk_index_search": NS(kind="hits", good=lambda o: lib.bsk_index_search(ctx, index.h, sb.h, by(good_sp), by(o)), want=want_hits,
                               bad=[lambda o: lib.bsk_index_search(ctx, index.h, sb.h, by(bad_sp), by(o))]),
        "bsk_hits_top": NS(kind="hits", good=lambda o: lib.bsk_hits_top(ctx, hits.h, 1, by(o)), want=SR.ref_top(*want_hits, 1),
                           bad=[lambda o: lib.bsk_hits_top(ctx, hits.h, 0, by(o))], aliased=(hits, want_hits)),
        "bsk_result_sets_reuse": NS(kind="sets", good=lambda o: lib.bsk_result_sets_reuse(ctx, result.h, L.SETS_PER_SEQUENCE, 1, by(o)), want=SC.ref_sets(per, 1, False) + (None,),
                                    bad=[], scope=lambda o: lib.bsk_result_sets_reuse(ctx, result.h, 2, 1, by(o))),
        "bsk_result_sets_counted": NS(kind="sets", good=lambda o: lib.bsk_result_sets_counted(ctx, result.h, L.SETS_PER_SEQUENCE, 1, by(o)), want=CC.ref_counted(per, 1, False),
                                      bad=[], scope=lambda o: lib.bsk_result_sets_counted(ctx, result.h, 2, 1, by(o))),
        "bsk_sets_neighbors": NS(kind="hits", good=lambda o: lib.bsk_sets_neighbors(ctx, sa.h, sb.h, 0, None, by(o)), want=NC.ref_neighbors(A, B, 0),
                                 bad=[lambda o: lib.bsk_sets_neighbors(ctx, sa.h, sb.h, 0, by(flag_np), by(o))]),
        "bsk_sets_neighbors_counted": NS(kind="hits", good=lambda o: lib.bsk_sets_neighbors_counted(ctx, sca.h, scb.h, 0, None, by(o)),
                                         want=NW.filter_weighted(*CW.ref_compare(A, CA, B, CB, 0)),
                                         bad=[lambda o: lib.bsk_sets_neighbors_counted(ctx, sca.h, scb.h, 0, by(flag_np), by(o))]),
        "bsk_hits_from_host": NS(kind="hits", good=lambda o: lib.bsk_hits_from_host(ctx, g_offs.ctypes.data, 3, g_tgt.ctypes.data, g_sh.ctypes.data, g_tot.ctypes.data, by(o)),
                                 want=(g_offs, g_tgt, g_sh, g_tot),
                                 bad=[lambda o: lib.bsk_hits_from_host(ctx, g_offs.ctypes.data, 3, g_unsorted.ctypes.data, g_sh.ctypes.data, g_tot.ctypes.data, by(o))]),
        "bsk_hits_cluster": NS(kind="clusters", good=lambda o: lib.bsk_hits_cluster(ctx, hits.h, None, None, by(o)), want=CL.model_components(3, *want_hits[:2])[:4],
                               bad=[lambda o: lib.bsk_hits_cluster(ctx, hits.h, by(cl_bad), None, by(o))]),
    }
    assert tuple(e) == ENTRIES
    yield NS(eng=eng, other=other, entries=e, foreign=foreign, result=result)
    for x in (foreign.clusters, foreign.sets, foreign.compare, foreign.hits, foreign.result, f_batch, hits, index, sa, sb, sca, scb, result, batch):
        x.close()
    other.close()
    eng.close()


def made(w, name):
    """the entry's good call into an empty slot -> (entry, slot, fetch, pointers, release)"""
    e = w.entries[name]
    fetch, ptrs, release = KINDS[e.kind]
    slot = C.c_void_p()
    w.eng._opts()
    assert e.good(slot) == L.OK and slot.value
    return e, slot, fetch, ptrs, getattr(w.eng.lib, release)


@pytest.mark.parametrize("name", ENTRIES)
def test_empty_slot_then_the_same_object(world, name):
    e, slot, fetch, ptrs, release = made(world, name)
    try:
        first, where = slot.value, ptrs(world.eng, slot)
        same(fetch(world.eng, slot), e.want)
        assert all(p for p, x in zip(where, e.want) if x is not None), where
        assert e.good(slot) == L.OK and slot.value == first and ptrs(world.eng, slot) == where
        same(fetch(world.eng, slot), e.want)
    finally:
        release(slot)


@pytest.mark.parametrize("name", SETS + COMPARES + SEARCHES + GRAPHS)
def test_argument_error_keeps_the_slot(world, name):
    e, slot, fetch, ptrs, release = made(world, name)
    try:
        first, where = slot.value, ptrs(world.eng, slot)
        for bad in e.bad:
            assert bad(slot) == L.ERR_ARG and slot.value == first and ptrs(world.eng, slot) == where
            same(fetch(world.eng, slot), e.want)
        assert e.good(slot) == L.OK and slot.value == first  # and is taken again
    finally:
        release(slot)
    if hasattr(e, "aliased"):  # *out equal to an input: refused, and the input is the caller's as before
        mine, want = e.aliased
        alias = C.c_void_p(mine.h.value)
        assert e.good(alias) == L.ERR_ARG and alias.value == mine.h.value
        same(fetch(world.eng, mine.h), want)


@pytest.mark.parametrize("name", ENTRIES)
def test_object_of_another_context_is_left_alone(world, name):
    e = world.entries[name]
    fetch = KINDS[e.kind][0]
    theirs = getattr(world.foreign, e.kind)
    slot = C.c_void_p(theirs.h.value)
    world.eng._opts()
    assert e.good(slot) == L.ERR_ARG and slot.value == theirs.h.value
    same(fetch(world.other, theirs.h), world.foreign.want[e.kind])  # still whole, still the second engine's


@pytest.mark.parametrize("name", RESULTS)
def test_result_sets_release_on_any_other_error(world, name):
    e, slot, _, _, release = made(world, name)
    try:
        assert e.scope(slot) == L.ERR_ARG and slot.value is None
        assert world.eng.lib.bsk_last_error(world.eng.ctx).decode() == "bsk_result_sets: bad scope"
        # ... also where the error is nominally an argument's: a bad scale, a result of another context
        call = getattr(world.eng.lib, name)
        for r, scope, scale in ((world.result, 0, -1), (world.foreign.result, 0, 1)):
            assert e.good(slot) == L.OK and slot.value
            assert call(world.eng.ctx, r.h, scope, scale, C.byref(slot)) == L.ERR_ARG and slot.value is None
        assert e.good(slot) == L.OK and slot.value  # from NULL again
        same(fetch_sets(world.eng, slot), e.want)
    finally:
        release(slot)


@pytest.mark.parametrize("name", COMPARES)
def test_compare_releases_past_its_cell_limit(world, name):
    e, slot, _, _, release = made(world, name)
    eng = world.eng
    a = eng.sets_from_arrays(np.zeros(65_536 + 1, U64), np.zeros(0, U64))
    b = eng.sets_from_arrays(np.zeros(32_769 + 1, U64), np.zeros(0, U64))  # 2^31 + 2^16 cells
    try:
        assert getattr(eng.lib, name)(eng.ctx, a.h, b.h, 0, C.byref(slot)) == L.ERR_UNSUPPORTED and slot.value is None
        assert eng.lib.bsk_last_error(eng.ctx).decode() == name + ": more than 2^31 cells (split the sets)"
        assert getattr(eng.lib, name)(eng.ctx, a.h, b.h, 0, C.byref(slot)) == L.ERR_UNSUPPORTED and slot.value is None  # an empty slot stays empty
        assert e.good(slot) == L.OK and slot.value
        same(fetch_compare(eng, slot), e.want)
    finally:
        release(slot)
        a.close()
        b.close()
