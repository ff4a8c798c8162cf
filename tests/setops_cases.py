"""Set algebra on sketch sets (include/biosketch.h "set algebra", bio_amd/csrc/setops.hip): the host-side restatement and the crafted inputs.

ref_op / ref_reduce are the header's rules in NumPy (np.union1d, np.intersect1d, np.setdiff1d, np.setxor1d per pair; np.unique with
counts per group).  The builders are plain NumPy and take the kernels' caps as arguments (read_caps reads them from setops.hip); every
builder returns its sets with what it claims about them -- a pair's t, the merged ranks of a shared value's two copies -- and
tests/test_setops_cases.py re-derives each claim from the sets alone.  tests/test_gpu_setops.py asserts from bsk_sets_plan that the
device reached the path before it compares."""
import os
import re

import numpy as np

U64 = np.uint64
UNION, INTERSECT, DIFF, SYMDIFF = 0, 1, 2, 3
OPS = (UNION, INTERSECT, DIFF, SYMDIFF)
MEMBERS_ALL = 0xFFFFFFFF
MAX64 = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read_caps(path=os.path.join(ROOT, "bio_amd", "csrc", "setops.hip")):
    """the #defines at the top of setops.hip -> {name: int}; a define may name an earlier one (SO_TILE = SO_WAVE_CAP)"""
    caps = {}
    for name, val in re.findall(r"^#define\s+((?:SO|RD)_\w+)\s+(\w+)", open(path).read(), re.M):
        caps[name] = caps[val] if val in caps else int(val, 0)
    return caps


# ---- the reference ----
def collection(sets):
    """list of sorted distinct value arrays -> (offsets, values)"""
    sets = [np.asarray(s, U64) for s in sets]
    offs = np.zeros(len(sets) + 1, U64)
    offs[1:] = np.cumsum([len(s) for s in sets])
    vals = np.concatenate(sets).astype(U64) if sets and offs[-1] else np.zeros(0, U64)
    return offs, vals


def split(offs, vals):
    return [vals[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


def ref_pair(a, b, op):
    if op == UNION:
        return np.union1d(a, b)
    if op == INTERSECT:
        return np.intersect1d(a, b, assume_unique=True)
    if op == DIFF:
        return np.setdiff1d(a, b, assume_unique=True)
    return np.setxor1d(a, b, assume_unique=True)


def ref_op(a, b, op):
    """(offsets, values) x (offsets, values) -> (offsets, values); b of one set (and a of any other number) is broadcast"""
    sa, sb = split(*a), split(*b)
    if len(sb) != len(sa):
        assert len(sb) == 1
        sb = sb * len(sa)
    return collection([ref_pair(x, y, op).astype(U64) for x, y in zip(sa, sb)])


def ref_reduce(s, group_offsets, min_members):
    sets, out = split(*s), []
    for g in range(len(group_offsets) - 1):
        members = sets[int(group_offsets[g]):int(group_offsets[g + 1])]
        m = len(members) if min_members == MEMBERS_ALL else min_members
        if not members:
            out.append(np.zeros(0, U64))
            continue
        v, c = np.unique(np.concatenate(members), return_counts=True)
        out.append(v[c >= m].astype(U64))
    return collection(out)


def pair_t(a_offs, b_offs):
    """t = |a_i| + |b_i| of every pair"""
    na, nb = np.diff(a_offs).astype(np.int64), np.diff(b_offs).astype(np.int64)
    return na + (nb if len(nb) == len(na) else nb[0])


def path_counts(a_offs, b_offs, caps):
    """pairs on the group, wave and tiled path"""
    t = pair_t(a_offs, b_offs)
    return [int((t <= caps["SO_GROUP_CAP"]).sum()), int(((t > caps["SO_GROUP_CAP"]) & (t <= caps["SO_WAVE_CAP"])).sum()), int((t > caps["SO_WAVE_CAP"]).sum())]


def merged(a, b):
    """the merged order of one pair, a's copy of a shared value first -> (values, from_a)"""
    v = np.concatenate([a, b])
    side = np.concatenate([np.zeros(len(a), np.int8), np.ones(len(b), np.int8)])
    order = np.lexsort((side, v))
    return v[order], side[order] == 0


# ---- builders ----
def pair(t, na, rng, shared=None):
    """one pair of t = |a| + |b| values with |a| = na; `shared` values in both (default: half of the smaller set)"""
    nb = t - na
    k = min(na, nb) // 2 if shared is None else shared
    pool = np.unique(rng.integers(0, MAX64, size=2 * t + 8, dtype=U64, endpoint=True))
    pool = rng.permutation(pool)[: t - k]
    assert len(pool) == t - k
    a = np.sort(pool[:na])
    b = np.sort(np.concatenate([pool[:k], pool[na:]]))
    return a, b


def degenerate_pairs():
    """name -> (a, b)"""
    e = np.zeros(0, U64)
    x = np.array([3, 9, 27, 81, 243], U64)
    return {
        "both empty": (e, e),
        "a empty": (e, x),
        "b empty": (x, e),
        "identical": (x, x.copy()),
        "disjoint interleaved": (np.arange(0, 40, 2, dtype=U64), np.arange(1, 41, 2, dtype=U64)),
        "a below b": (np.arange(10, dtype=U64), np.arange(100, 110, dtype=U64)),
        "b below a": (np.arange(100, 110, dtype=U64), np.arange(10, dtype=U64)),
        "extremes on both sides": (np.array([0, 5, MAX64], U64), np.array([0, 7, MAX64], U64)),
        "extremes split": (np.array([0, 5], U64), np.array([5, MAX64], U64)),
    }


def class_edges(cap, rng):
    """pairs of t = cap - 1, cap, cap + 1, each with |a| = 0, 1, t / 2, t - 1 -> [(a, b, t, na)]"""
    out = []
    for t in (cap - 1, cap, cap + 1):
        for na in (0, 1, t // 2, t - 1):
            a, b = pair(t, na, rng)
            out.append((a, b, t, na))
    return out


def tile_pair(t, shared_at, rng):
    """One pair of t merged ranks.  shared_at: ranks r such that ranks r and r + 1 are the two copies of one value (a's at r); every
    other rank holds a value of its own, from a or b at random.  -> (a, b)"""
    shared_at = sorted(shared_at)
    assert all(y - x >= 2 for x, y in zip(shared_at, shared_at[1:])) and all(0 <= r and r + 1 < t for r in shared_at)
    second = np.zeros(t, bool)
    second[[r + 1 for r in shared_at]] = True
    n_distinct = t - len(shared_at)
    vals = np.sort(rng.choice(1 << 40, size=n_distinct, replace=False).astype(U64)) * U64(3) + U64(1)
    v = vals[np.cumsum(~second) - 1]  # rank -> value: a second copy repeats the value of the rank before it
    from_a = rng.integers(0, 2, size=t).astype(bool)
    from_a[shared_at] = True
    from_a[second] = False
    return v[from_a], v[~from_a]


def tile_cases(tile, rng):
    """name -> (a, b, ranks of the a copies of the shared values) for the pair of 3 * tile + 5 merged ranks"""
    t = 3 * tile + 5
    cases = {
        "straddles the boundary after tile 0": [tile - 1],
        "straddles the boundary after tile 1": [2 * tile - 1],
        "straddles both boundaries": [tile - 1, 2 * tile - 1],
        "last ranks of tile 0, not straddling": [tile - 2],
        "first ranks of tile 1": [tile],
        "straddles all three boundaries, and the last two ranks": [tile - 1, 2 * tile - 1, 3 * tile - 1, t - 2],
        "every value shared but the first (every boundary straddled)": list(range(1, t, 2)),
        "no value shared": [],
    }
    return {name: tile_pair(t, at, rng) + (at,) for name, at in cases.items()}


def shifted_pairs(n, t_lo, t_hi, rng, n_base=257):
    """n pairs with t in [t_lo, t_hi]: pair p is base pair p % n_base with p * 2^41 added to every value (base values are below 2^40,
    so the shift commutes with every op) -> (a, b, base pairs, shift per pair)"""
    base = []
    for i in range(n_base):
        t = int(rng.integers(t_lo, t_hi + 1))
        na = int(rng.integers(0, t + 1))
        nb = t - na
        k = int(rng.integers(0, min(na, nb) + 1))
        pool = rng.permutation(rng.choice(1 << 40, size=t - k, replace=False).astype(U64))
        base.append((np.sort(pool[:na]), np.sort(np.concatenate([pool[:k], pool[na:]]))))
    shift = np.arange(n, dtype=U64) << U64(41)
    return tile_shifted([x for x, _ in base], shift), tile_shifted([y for _, y in base], shift), base, shift


def tile_shifted(base_sets, shift):
    """collection whose set p is base_sets[p % len(base_sets)] + shift[p]"""
    n, nb = len(shift), len(base_sets)
    sizes = np.array([len(s) for s in base_sets], np.int64)
    which = np.arange(n) % nb
    offs = np.zeros(n + 1, U64)
    offs[1:] = np.cumsum(sizes[which])
    bo, bv = collection(base_sets)
    start = bo[:-1].astype(np.int64)[which]
    idx = np.repeat(start - offs[:-1].astype(np.int64), sizes[which]) + np.arange(int(offs[-1]))
    vals = bv[idx] + np.repeat(shift, sizes[which]) if int(offs[-1]) else np.zeros(0, U64)
    return offs, vals.astype(U64)


def ref_shifted(base, shift, op):
    """ref_op of shifted_pairs' collections: NumPy per base pair, then the pairs' shifts"""
    return tile_shifted([ref_pair(x, y, op).astype(U64) for x, y in base], shift)


def reduce_groups(rng):
    """-> (sets, group_offsets): groups of 0, 1, 2 and 64 members, empty members inside groups, an empty group first, in the middle and
    last; in the group of 64, value 7 is held by every member, 8 by 63, 9 by 2, 10 by 1; and the last value of group 1 equals the first
    value of group 2 (a run that would reach two members only across the groups' border)"""
    e = np.zeros(0, U64)
    sets, go = [], [0]

    def group(members):
        sets.extend(members)
        go.append(len(sets))

    group([])                                                       # 0: empty group first
    group([np.array([1, 5, 1000], U64)])                            # 1: one member; its last value ...
    group([np.array([1000, 2000], U64), np.array([1500, 2000], U64)])  # 2: ... is the first value of this group: held by ONE member here
    group([])                                                       # 3: empty group in the middle
    big = []
    for i in range(64):
        own = np.unique(rng.integers(100, 1 << 62, size=5, dtype=U64))
        fixed = [7] + ([8] if i != 17 else []) + ([9] if i in (3, 40) else []) + ([10] if i == 5 else [])
        big.append(np.unique(np.concatenate([np.array(fixed, U64), own])))
    group(big)                                                      # 4: 64 members
    group([np.array([4, 6], U64), e, np.array([4, 9], U64)])        # 5: an empty member inside: empties the intersection
    group([e, e])                                                   # 6: only empty members
    group([np.array([0, MAX64], U64), np.array([0, 3, MAX64], U64)])  # 7
    group([])                                                       # 8: empty group last
    return collection(sets), np.array(go, U64)
