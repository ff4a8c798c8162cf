"""GPU: bsk_hits_cluster and bsk_hits_from_host against the models of tests/cluster_cases.py -- every generator, both methods, every
kind of score; the arrays, the figures and the number of rounds are the models'."""
import ctypes as C
import re

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import cluster_cases as CL
from tests import neighbor_cases as NC

pytestmark = pytest.mark.gpu
U64, U32 = np.uint64, np.uint32
CASES = CL.cases()


def fetched(c):
    label, rep, offsets, members = c.fetch()
    inf = c.info()
    assert inf["n_items"] == len(label) and inf["n_clusters"] == len(rep)
    return label, rep, offsets, members, inf["largest"]


def check(engine, n, pairs, method, score, reuse=None, what=""):
    o, t, s = CL.csr(n, pairs)
    hits = engine.hits_from_arrays(o, t, s)
    c = hits.cluster(method, score, reuse=reuse)
    want, rounds = CL.ROUND_MODELS[method](n, o, t, score)
    assert CL.same(want, CL.MODELS[method](n, o, t, score)), what
    got = fetched(c)
    assert CL.same(got, want), (what, [a.tolist() for a in got[:4]], [a.tolist() for a in want[:4]])
    p = c.plan()
    edges = CL.n_offdiagonal(o, t)
    name = "k_cl_mis" if method == "greedy" else "k_cl_hook+k_cl_jump"
    assert p["plan"] == f"{name}, n={n} edges={edges} rounds={rounds}" and p["rounds"] == rounds and p["edges"] == edges, (what, p, rounds)
    assert np.array_equal(c.sizes, np.diff(want[2]))
    hits.close()
    return c


@pytest.mark.parametrize("form", ["full", "upper", "mixed"])
@pytest.mark.parametrize("method", CL.METHODS)
def test_every_generator_every_score(engine, method, form):
    c = None
    for k, (name, n, pairs) in enumerate(CASES):
        if not name.endswith("-" + form):
            continue
        for sname, sc in CL.scores(n, seed=k).items():
            c = check(engine, n, pairs, method, sc, reuse=c, what=(name, sname))
    c.close()


def test_the_forms_of_one_graph_give_the_same_bytes(engine):
    for k in range(0, len(CASES), 3):
        n = CASES[k][1]
        sc = CL.scores(n, seed=k)["random"]
        for method in CL.METHODS:
            got = []
            for name, _, pairs in CASES[k:k + 3]:
                o, t, s = CL.csr(n, pairs)
                h = engine.hits_from_arrays(o, t, s)
                c = h.cluster(method, sc)
                got.append(b"".join(a.tobytes() for a in c.fetch()) + repr(c.info()).encode())
                c.close()
                h.close()
            assert got[0] == got[1] == got[2], (CASES[k][0], method)


def test_hits_from_arrays_round_trips(engine):
    o, t, s = CL.csr(65, dict((nm, p) for nm, _, p in CASES)["gnp_dense_65-mixed"])
    s = (np.arange(len(t), dtype=U32) * U32(7) + U32(1))
    tt = s + U32(3)
    h = engine.hits_from_arrays(o, t, s)
    assert NC.same(h.fetch(), (o, t, s)) and not h.has_totals() and h.total is None and h.plan() == dict(plan="from host", n_large_queries=0)
    assert h.info() == dict(n_queries=65, n_hits=len(t))
    h2 = engine.hits_from_arrays(o, t, s, tt)
    assert NC.same(h2.fetch(), (o, t, s)) and h2.has_totals() and np.array_equal(h2.fetch_totals(), tt) and np.array_equal(h2.total, tt)
    # into an existing object: the arrays are kept, the totals go when none are given
    before = h2.device()
    h3 = engine.hits_from_arrays(o[:5], t[:int(o[4])], s[:int(o[4])], reuse=h2)
    assert h3 is h2 and h2.device() == before and not h2.has_totals() and NC.same(h2.fetch(), (o[:5], t[:int(o[4])], s[:int(o[4])]))
    # rectangular hits are hits too (targets beyond the rows), and the top of them works
    r = engine.hits_from_arrays(np.array([0, 2, 3], U64), np.array([5, 9, 0], U32), np.array([1, 4, 2], U32))
    assert NC.same(r.top(1).fetch(), (np.array([0, 1, 2]), np.array([9, 0]), np.array([4, 2])))
    e = engine.hits_from_arrays(np.zeros(1, U64), np.zeros(0, U32), np.zeros(0, U32))
    assert e.info() == dict(n_queries=0, n_hits=0)
    # the host checks, with a context: BSK_ERR_ARG, the slot as it was
    lib, ctx = engine.lib, engine.ctx
    slot = C.c_void_p(h.h.value)
    for bad_o, bad_t, text in (([0, 2, 1], [1, 2], b"offsets decrease"), ([1, 2, 2], [1, 2], b"offsets[0] != 0"), ([0, 2, 2], [2, 1], b"strictly ascending"),
                               ([0, 2, 2], [1, 1], b"strictly ascending")):
        bo, bt, bs = np.array(bad_o, U64), np.array(bad_t, U32), np.ones(2, U32)
        assert lib.bsk_hits_from_host(ctx, bo.ctypes.data, 2, bt.ctypes.data, bs.ctypes.data, None, C.byref(slot)) == L.ERR_ARG and slot.value == h.h.value
        assert text in lib.bsk_last_error(ctx)
    bo, bt = np.array([0, 2, 2], U64), np.array([1, 2], U32)
    assert lib.bsk_hits_from_host(ctx, bo.ctypes.data, 2, bt.ctypes.data, None, None, C.byref(slot)) == L.ERR_ARG and slot.value == h.h.value
    assert NC.same(h.fetch(), (o, t, s))  # intact
    for x in (h, h2, r, e):
        x.close()


def families(seed):
    """64 families of 4 sets: 1 000 values each, the three copies with 100 of them replaced -> (list of sorted u64 arrays, family of every set)"""
    rng = np.random.default_rng(seed)
    sets, fam = [], []
    for f in range(64):
        base = np.unique(rng.integers(0, 1 << 62, 1100, dtype=U64))[:1000]
        assert len(base) == 1000
        for copy in range(4):
            v = base.copy()
            if copy:
                v[rng.choice(1000, 100, replace=False)] = rng.integers(1 << 62, 1 << 63, 100, dtype=U64)
            sets.append(np.unique(v))
            fam.append(f)
    order = rng.permutation(len(sets))
    return [sets[i] for i in order], np.array(fam)[order]


def test_end_to_end_families(engine):
    sets, fam = families(20261)
    n = len(sets)
    offsets = np.zeros(n + 1, U64)
    offsets[1:] = np.cumsum([len(s) for s in sets], dtype=U64)
    # on the CPU first: at Jaccard >= 1/2 the seeds join no two families and leave none apart
    owners = {}
    for i, s in enumerate(sets):
        for v in s.tolist():
            owners.setdefault(v, []).append(i)
    sh = [[0] * n for _ in range(n)]
    for own in owners.values():
        for a in own:
            for b in own:
                sh[a][b] += 1
    sh = np.array(sh, U32)
    size = np.diff(offsets).astype(np.int64)
    tt = (size[:, None] + size[None, :] - sh).astype(U32)
    want = NC.filter_matrices(sh, tt, 1, 1, 2, upper=True)  # neighbor_cases' rule over the whole sets (limit 0)
    for i in range(n):
        for p in range(int(want[0][i]), int(want[0][i + 1])):
            assert fam[i] == fam[int(want[1][p])]
    comp = CL.model_components(n, want[0], want[1])
    assert len(comp[1]) == 64 and comp[4] == 4
    d = engine.sets_from_arrays(offsets, np.concatenate(sets))
    h = d.neighbors(upper=True, min_jaccard=(1, 2))
    assert NC.same(h.fetch(), want[:3])
    c = h.cluster("components")
    assert CL.same(fetched(c), comp) and c.info() == dict(n_items=256, n_clusters=64, largest=4)
    label = c.label
    for f in range(64):
        assert len(set(label[fam == f].tolist())) == 1
    assert len(set(label.tolist())) == 64
    size = np.diff(offsets)
    g = h.cluster("greedy", score=size, reuse=c)
    assert g is c and CL.same(fetched(g), CL.model_greedy(n, want[0], want[1], size))
    assert g.info()["n_clusters"] == 64 and sorted(fam[g.rep].tolist()) == list(range(64))  # one representative per family
    # the full result of the same call clusters identically
    full = d.neighbors(min_jaccard=(1, 2))
    for m, sc in (("components", None), ("greedy", size)):
        a, b = full.cluster(m, sc), h.cluster(m, sc)
        assert CL.same(fetched(a), fetched(b)) and a.plan()["edges"] == 2 * b.plan()["edges"]
        a.close(), b.close()
    for x in (c, h, full, d):
        x.close()


def test_rectangular_hits_are_refused_and_the_slot_stays(engine):
    lib, ctx = engine.lib, engine.ctx
    o, t, s = CL.csr(17, [(i, (5 * i) % 17) for i in range(17)])
    good = engine.hits_from_arrays(o, t, s)
    c = good.cluster("components")
    before, arrays = fetched(c), c.device()
    # 17 rows, one target of 17 and one of 32: a 17 x 33 comparison's hits
    for bad_target in (17, 32, 0xFFFFFFFF):
        o2, t2, s2 = CL.csr(17, [(3, 4), (16, 2)])
        t2 = t2.copy()
        t2[-1] = bad_target
        rect = engine.hits_from_arrays(o2, t2, s2)
        for method in (L.CLUSTER_COMPONENTS, L.CLUSTER_GREEDY):
            cp = L.ClusterParams(method, 0)
            slot = C.c_void_p(c.h.value)
            assert lib.bsk_hits_cluster(ctx, rect.h, C.byref(cp), None, C.byref(slot)) == L.ERR_ARG and slot.value == c.h.value
            assert b"target >= n_queries" in lib.bsk_last_error(ctx)
            empty = C.c_void_p()
            assert lib.bsk_hits_cluster(ctx, rect.h, C.byref(cp), None, C.byref(empty)) == L.ERR_ARG and not empty.value
        with pytest.raises(Exception):
            rect.cluster("greedy", reuse=c)
        assert c.h and c.device() == arrays and CL.same(fetched(c), before)
        rect.close()
    # through the sets, 17 rows against 33 columns: while every listed column is below 17 the hits cluster, a column from 17 on is refused
    A = engine.sets_from_arrays(np.arange(34, dtype=U64), np.arange(33, dtype=U64))
    B = engine.sets_from_arrays(np.arange(18, dtype=U64), np.arange(17, dtype=U64))
    wide = B.neighbors(A)  # set i of b only meets set i of a
    assert wide.info() == dict(n_queries=17, n_hits=17) and wide.cluster().info()["n_clusters"] == 17
    A2 = engine.sets_from_arrays(np.arange(34, dtype=U64), np.arange(33, dtype=U64)[::-1].copy())
    rect = B.neighbors(A2)  # set i of b meets set 32 - i of a: targets 16 .. 32
    with pytest.raises(Exception):
        rect.cluster()
    # unknown method, a flag bit: refused before anything runs, the slot kept
    slot = C.c_void_p(c.h.value)
    for cp in (L.ClusterParams(2, 0), L.ClusterParams(0, 1), L.ClusterParams(1, 0x80000000), L.ClusterParams(0xFFFFFFFF, 0)):
        assert lib.bsk_hits_cluster(ctx, good.h, C.byref(cp), None, C.byref(slot)) == L.ERR_ARG and slot.value == c.h.value
    assert CL.same(fetched(c), before)
    for x in (c, good, A, B, A2, wide, rect):
        x.close()


def test_the_slot(engine):
    name, n, pairs = next(x for x in CASES if x[0] == "gnp_257-full")
    sc = CL.scores(n, seed=5)["random"]
    c = check(engine, n, pairs, "components", sc, what="first")
    arrays = c.device()
    assert check(engine, n, pairs, "greedy", sc, reuse=c, what="other method, same object") is c and c.device()[0] == arrays[0] and c.device()[3] == arrays[3]
    arrays = c.device()  # (greedy has more clusters than components: rep and offsets may have grown, label and members did not move)
    # a smaller graph into the object last filled from a larger one: the arrays stay where they are
    small = next(x for x in CASES if x[0] == "two_k8_bridge-upper")
    assert check(engine, small[1], small[2], "components", None, reuse=c, what="smaller") is c and c.device() == arrays
    assert check(engine, 1, [], "greedy", None, reuse=c, what="one node") is c and c.device() == arrays
    assert check(engine, n, pairs, "components", sc, reuse=c, what="large again") is c
    # clusters, and hits, of another context: BSK_ERR_ARG, and they stay in the slot
    other = S.Engine(0)
    try:
        o, t, s = CL.csr(small[1], small[2])
        mine, theirs = engine.hits_from_arrays(o, t, s), other.hits_from_arrays(o, t, s)
        foreign = theirs.cluster()
        slot = C.c_void_p(foreign.h.value)
        assert engine.lib.bsk_hits_cluster(engine.ctx, mine.h, None, None, C.byref(slot)) == L.ERR_ARG and slot.value == foreign.h.value
        assert b"another context" in engine.lib.bsk_last_error(engine.ctx)
        slot = C.c_void_p(c.h.value)
        assert engine.lib.bsk_hits_cluster(engine.ctx, theirs.h, None, None, C.byref(slot)) == L.ERR_ARG and slot.value == c.h.value
        buf = np.full(16, 9, U32)
        assert engine.lib.bsk_clusters_fetch(engine.ctx, foreign.h, buf.ctypes.data, None, None, None) == L.ERR_ARG and (buf == 9).all()
        assert CL.same(fetched(foreign), CL.model_components(small[1], o, t))  # intact
        hslot = C.c_void_p(theirs.h.value)
        assert engine.lib.bsk_hits_from_host(engine.ctx, o.ctypes.data, small[1], t.ctypes.data, s.ctypes.data, None, C.byref(hslot)) == L.ERR_ARG
        assert hslot.value == theirs.h.value
        # any subset of the arrays may be asked for
        lab = np.zeros(16, U32)
        assert other.lib.bsk_clusters_fetch(other.ctx, foreign.h, None, None, None, None) == L.OK
        assert other.lib.bsk_clusters_fetch(other.ctx, foreign.h, lab.ctypes.data, None, None, None) == L.OK and lab.tolist() == [0] * 16
        for x in (foreign, theirs, mine):
            x.close()
    finally:
        other.close()
    c.close()


def test_ten_calls_give_identical_bytes(engine):
    name, n, pairs = next(x for x in CASES if x[0] == "gnp_257-mixed")
    o, t, s = CL.csr(n, pairs)
    h = engine.hits_from_arrays(o, t, s)
    sc = CL.scores(n, seed=9)["few"]
    for method in CL.METHODS:
        seen = set()
        c = None
        for k in range(10):
            c = h.cluster(method, sc, reuse=c if k % 2 else None)
            seen.add(b"".join(a.tobytes() for a in c.fetch()) + repr((c.info(), c.plan())).encode())
        assert len(seen) == 1, method
    h.close()


def test_no_nodes(engine):
    h = engine.hits_from_arrays(np.zeros(1, U64), np.zeros(0, U32), np.zeros(0, U32))
    for method in CL.METHODS:
        c = h.cluster(method)
        label, rep, offsets, members = c.fetch()
        assert c.info() == dict(n_items=0, n_clusters=0, largest=0) and len(label) == len(rep) == len(members) == 0 and offsets.tolist() == [0]
        assert re.fullmatch(r"k_cl_\S+, n=0 edges=0 rounds=0", c.plan()["plan"]) and len(c.sizes) == 0
        c = h.cluster(method, np.zeros(0, U64), reuse=c)
        assert c.info()["n_clusters"] == 0
    h.close()


def test_the_long_paths(engine):
    """components on 4 096 nodes in shuffled order: one cluster in at most 20 rounds; greedy on the 257-node path ranked from one end: the
    worst case, one node a round"""
    n = 4096
    c = check(engine, n, CL.forms(CL.path(n, seed=4096))["upper"], "components", None, what="shuffled path")
    assert c.info() == dict(n_items=n, n_clusters=1, largest=n) and c.plan()["rounds"] <= 20
    c = check(engine, 257, CL.forms(CL.path(257))["mixed"], "greedy", None, reuse=c, what="identity path")
    assert c.plan()["rounds"] == 257 and c.info()["n_clusters"] == 129
    with pytest.raises(ValueError):
        engine.hits_from_arrays(*CL.csr(3, [(0, 1)])).cluster("components", np.zeros(4, U64))
    with pytest.raises(ValueError):
        engine.hits_from_arrays(*CL.csr(3, [(0, 1)])).cluster("single")
    c.close()
