"""What the tests of the weighted sparse all-pairs comparison (bsk_sets_neighbors_counted) share: the model -- the rule of
tests/neighbor_cases.py applied to compare_counted_cases.ref_compare, dot and min_sum gathered at the kept cells -- and the cases the GPU
runs, built from the existing builders with counts attached.  tests/test_neighbor_counted_cases.py re-derives every expectation by a
second formulation (dense_compare on dense count vectors) and asserts on the CPU what makes a case meaningful;
tests/test_gpu_neighbors_counted.py runs the library against it."""
import collections
import functools

import numpy as np

from tests import compare_cases as CC
from tests import compare_counted_cases as WC
from tests import neighbor_cases as NC

U64, U32 = np.uint64, np.uint32

# B None: A against itself (one object).  runs: [(limit, parameters of Sets.neighbors_counted)].  dense: (da, db) count vectors over the
# case's own pool where the builder has them (small_pool_sets), else None (densify() makes them).
Case = collections.namedtuple("Case", "A CA B CB runs dense")


def rule(p):
    """parameters of Sets.neighbors_counted -> keyword arguments of neighbor_cases.keeps (min_jaccard here is a (num, den) pair or None)"""
    num, den = p.get("min_jaccard") or (0, 0)
    return dict(min_shared=p.get("min_shared", 1), num=num, den=den, upper=p.get("upper", False))


def thresholded(p):
    r = rule(p)
    return r["min_shared"] > 1 or r["den"] != 0


def filter_weighted(sh, tt, dt, ms, **r):
    """dense shared / total / dot / min_sum -> (offsets, target, shared, total, dot, min_sum): the kept cells of filter_matrices, and the
    weights of those cells -- they take no part in the rule"""
    offsets, target, shared, total = NC.filter_matrices(sh, tt, **r)
    rows = np.repeat(np.arange(sh.shape[0]), np.diff(offsets).astype(np.int64))
    cols = target.astype(np.int64)
    return offsets, target, shared, total, np.asarray(dt, U64)[rows, cols], np.asarray(ms, U64)[rows, cols]


def operands(case):
    return case.A, case.CA, (case.A if case.B is None else case.B), (case.CA if case.B is None else case.CB)


def expected(case, limit, p):
    """the model of one run"""
    return filter_weighted(*reference(case, limit), **rule(p))


_REF = {}


def reference(case, limit):
    """ref_compare of the case's operands, computed once per (case, limit)"""
    key = (id(case), limit)
    if key not in _REF:
        _REF[key] = (case, WC.ref_compare(*operands(case), limit))  # (the case is kept alive: its id stays its own)
    return _REF[key][1]


def densify(case):
    """dense count vectors [n, P] over the union of every value of the case (0: absent): what dense_compare works on"""
    if case.dense is not None:
        return case.dense
    A, CA, B, CB = operands(case)
    CA = WC.ones(A) if CA is None else CA
    CB = WC.ones(B) if CB is None else CB
    parts = [np.asarray(s, U64) for s in list(A) + list(B) if len(s)]
    pool = np.unique(np.concatenate(parts)) if parts else np.zeros(0, U64)

    def dense(sets, counts):
        out = np.zeros((len(sets), max(len(pool), 1)), np.int64)
        for i, (s, c) in enumerate(zip(sets, counts)):
            out[i, np.searchsorted(pool, np.asarray(s, U64))] = np.asarray(c, np.int64)
        return out

    return dense(A, CA), dense(B, CB)


ALL_RULES = [dict(min_shared=m, min_jaccard=j) for m in (1, 2) for j in (None, (1, 2), (1, 1))]


@functools.lru_cache(None)
def cases():
    """name -> Case.  The shapes are the smallest at which the kernel takes another path: sizes around the window, one set racing ahead
    of its tile, ragged tiles, the four operand kinds, every rule, more tiles than workgroups."""
    caps = CC.read_caps()
    R, Cc, W = caps["CMP_ROWS"], caps["CMP_COLS"], caps["CMP_WINDOW"]
    out = {}
    A, B, _ = CC.window_edges(W)
    # all values; a limit inside the second window; a limit beyond it with a Jaccard threshold
    out["window_edges"] = Case(A, WC.attach(A, 1, 9, 51), B, WC.attach(B, 1, 9, 52), [(0, {}), (W + 1, {}), (2 * W + 1, dict(min_jaccard=(1, 8)))], None)
    for k, (name, (A, B)) in enumerate(sorted(CC.skew_cases(W).items())):
        out["skew_" + name] = Case(A, WC.attach(A, 1, 9, 60 + k), B, WC.attach(B, 1, 9, 70 + k), [(0, {})], None)
    A, _, _ = CC.tile_edges(R, Cc)
    CA = WC.attach(A, 1, 9, 53)
    for n in (15, 16, 17, 33):
        out["tiles_%d" % n] = Case(A[:n], CA[:n], None, None, [(0, {}), (0, dict(upper=True))], None)
    # the operand kinds on one pool
    (sa, ma), (sb, mb) = CC.small_pool_sets(20, seed=22), CC.small_pool_sets(18, seed=23)
    (da, ca), (db, cb) = WC.pool_counts(ma, 1, 9, 54), WC.pool_counts(mb, 1, 9, 55)
    ua, ub = (da > 0).astype(np.int64), (db > 0).astype(np.int64)
    out["kinds_cc"] = Case(sa, ca, sb, cb, [(0, {})], (da, db))
    out["kinds_cu"] = Case(sa, ca, sb, None, [(0, {})], (da, ub))
    out["kinds_uc"] = Case(sa, None, sb, cb, [(0, {})], (ua, db))
    out["kinds_uu"] = Case(sa, None, sb, None, [(0, {})], (ua, ub))
    # every rule, 40 x 40 against itself: nine tiles (the stride loop under a cap of 2), more than 8 kept pairs (the second run)
    s, m = CC.small_pool_sets(40, seed=24)
    d, c = WC.pool_counts(m, 1, 9, 56)
    out["rules_40"] = Case(s, c, None, None, [(0, p) for p in ALL_RULES], (d, d))
    (sa, ma), (sb, mb) = CC.small_pool_sets(70, seed=25), CC.small_pool_sets(50, seed=26)
    (da, ca), (db, cb) = WC.pool_counts(ma, 1, 9, 57), WC.pool_counts(mb, 1, 9, 58)
    out["pool_70x50"] = Case(sa, ca, sb, cb, [(0, {})], (da, db))
    return out
