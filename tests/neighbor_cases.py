"""What the tests of the sparse all-pairs comparison (bsk_sets_neighbors) share: the model -- the rule of include/biosketch.h applied to
compare_cases.ref_compare -- a direct per-pair walk to check the model against, the tiles a call runs and skips, and the n best of a row
(tests/test_neighbor_cases.py checks all of it on the CPU, tests/test_gpu_neighbors.py runs the library against it)."""
import re

import numpy as np

from tests import compare_cases as CC

U64, U32 = np.uint64, np.uint32


def keeps(shared, total, i, j, min_shared=1, num=0, den=0, upper=False):
    """the rule for one pair, in Python integers (exact at any size)"""
    shared, total = int(shared), int(total)
    return shared >= max(int(min_shared), 1) and (den == 0 or shared * int(den) >= int(num) * total) and (not upper or j > i)


def filter_matrices(sh, tt, min_shared=1, num=0, den=0, upper=False):
    """dense shared / total [n_a, n_b] -> (offsets u64[n_a + 1], target u32[], shared u32[], total u32[]): CSR by row, columns ascending"""
    n_a = sh.shape[0]
    offsets, target, shared, total = np.zeros(n_a + 1, U64), [], [], []
    for i in range(n_a):
        for j in range(sh.shape[1]):
            if keeps(sh[i, j], tt[i, j], i, j, min_shared, num, den, upper):
                target.append(j)
                shared.append(int(sh[i, j]))
                total.append(int(tt[i, j]))
        offsets[i + 1] = len(target)
    return offsets, np.array(target, U32), np.array(shared, U32), np.array(total, U32)


def ref_neighbors(A, B, limit, min_shared=1, num=0, den=0, upper=False):
    """the model: lists of sorted distinct u64 arrays -> (offsets, target, shared, total)"""
    sh, tt = CC.ref_compare(A, B, limit)
    return filter_matrices(sh, tt, min_shared, num, den, upper)


def walk_pair(a, b, limit):
    """(shared, total) of one pair by a two-pointer merge in Python integers: the first `limit` distinct values of the union (0: all)"""
    a, b = [int(v) for v in a], [int(v) for v in b]
    ia = ib = shared = total = 0
    while (ia < len(a) or ib < len(b)) and not (limit and total >= limit):
        total += 1
        if ib >= len(b) or (ia < len(a) and a[ia] < b[ib]):
            ia += 1
        elif ia >= len(a) or b[ib] < a[ia]:
            ib += 1
        else:
            shared, ia, ib = shared + 1, ia + 1, ib + 1
    return shared, total


def walk_neighbors(A, B, limit, min_shared=1, num=0, den=0, upper=False):
    """ref_neighbors without ref_compare: pair by pair"""
    offsets, target, shared, total = np.zeros(len(A) + 1, U64), [], [], []
    for i, a in enumerate(A):
        for j, b in enumerate(B):
            s, t = walk_pair(a, b, limit)
            if keeps(s, t, i, j, min_shared, num, den, upper):
                target.append(j)
                shared.append(s)
                total.append(t)
        offsets[i + 1] = len(target)
    return offsets, np.array(target, U32), np.array(shared, U32), np.array(total, U32)


def expected_tiles(n_a, n_b, upper, caps):
    """(tiles run, tiles skipped) of one call: with upper a tile whose every pair has j <= i is not run"""
    R, Cc = caps["CMP_ROWS"], caps["CMP_COLS"]
    ty, tx = -(-n_a // R), -(-n_b // Cc)
    assert ty * tx == CC.n_tiles(n_a, n_b, caps)
    # tile (r, c) holds rows from r * R and columns up to c * Cc + Cc - 1: skipped when that last column is not above the first row
    skipped = sum(min(tx, (r * R - (Cc - 1)) // Cc + 1) for r in range(ty) if r * R >= Cc - 1) if upper else 0
    return ty * tx - skipped, skipped


def plan_figures(plan):
    """the decimal figures of bsk_hits_plan's string: {'tiles': .., 'skipped': .., 'rounds': .., 'runs': ..}"""
    return {k: int(v) for k, v in re.findall(r"\b(tiles|skipped|rounds|runs)=(\d+)", plan)}


def top_rows(offsets, target, shared, n):
    """bsk_hits_top's order on CSR hits: per row the min(n, hits) largest shared, ties by ascending target -> (offsets, target, shared)"""
    o, t, s = np.zeros(len(offsets), U64), [], []
    for i in range(len(offsets) - 1):
        a, e = int(offsets[i]), int(offsets[i + 1])
        order = sorted(range(a, e), key=lambda p: (-int(shared[p]), int(target[p])))[:n]
        t += [int(target[p]) for p in order]
        s += [int(shared[p]) for p in order]
        o[i + 1] = len(t)
    return o, np.array(t, U32), np.array(s, U32)


def same(x, y):
    """exact equality of two (offsets, target, shared[, total]) tuples, dtypes aside"""
    return len(x) == len(y) and all(np.array_equal(np.asarray(p).astype(U64), np.asarray(q).astype(U64)) for p, q in zip(x, y))


def pairs_case(n):
    """the collection beyond 2^31 cells: n sets, set i = {i // 2} -- every set shares its one value with exactly one other"""
    return np.arange(n + 1, dtype=U64), (np.arange(n, dtype=U64) // U64(2))
