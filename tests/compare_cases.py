"""What the all-pairs comparison and the bottom-n tests share: the NumPy references, the caps of compare.hip, a pure-Python restatement
of k_cmp_tile's round rule (how many rounds a tile takes), and the case builders -- each returns its sets together with what it claims
about them (tests/test_compare_cases.py re-derives every claim on the CPU, tests/test_gpu_compare.py runs the cases)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64, U32 = np.uint64, np.uint32
MAX = (1 << 64) - 1


def read_caps(path=os.path.join(ROOT, "bio_amd", "csrc", "compare.hip")):
    """the #define CMP_* NUMBER lines at the top of compare.hip -> {name: int}"""
    return {name: int(val, 0) for name, val in re.findall(r"^#define\s+(CMP_\w+)\s+(\d\w*)", open(path).read(), re.M)}


def u64(values):
    return np.array(sorted(set(int(v) for v in values)), U64)


def collection(sets):
    """list of sorted distinct value arrays -> (offsets, values)"""
    sets = [np.asarray(s, U64) for s in sets]
    offs = np.zeros(len(sets) + 1, U64)
    if sets:
        offs[1:] = np.cumsum([len(s) for s in sets])
    return offs, (np.concatenate(sets) if sets and int(offs[-1]) else np.zeros(0, U64))


def split(offsets, values):
    return [values[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


# ---- the references ----
def ref_pair(a, b, limit):
    """(shared, total) of one pair: the union cut at limit, the intersection's values at or below its last element"""
    u = np.union1d(a, b)
    if limit:
        u = u[:limit]
    if len(u) == 0:
        return 0, 0
    return int(np.count_nonzero(np.intersect1d(a, b) <= u[-1])), len(u)


def ref_compare(A, B, limit):
    """lists of sorted distinct u64 arrays -> (shared[n_a, n_b], total[n_a, n_b]) u32"""
    sh, tt = np.zeros((len(A), len(B)), U32), np.zeros((len(A), len(B)), U32)
    for i, a in enumerate(A):
        for j, b in enumerate(B):
            sh[i, j], tt[i, j] = ref_pair(a, b, limit)
    return sh, tt


def ref_bottom(sets, n):
    return [np.asarray(s, U64)[:n] for s in sets]


# ---- the round rule of k_cmp_tile, restated ----
def tile_rounds(a_sets, b_sets, limit, window):
    """One tile: (rounds, shared, total).  Every set has a prefix of min(limit, size) values and a cursor.  A round: v_hi is the smallest
    value[cursor + window] among the sets with more than `window` values left -- none: the last round, everything left is staged;
    every set stages its values below v_hi (at most `window`) and moves its cursor past them; every pair that has not reached the
    limit merges its two windows.  The tile stops after the last round or once every pair has reached the limit."""
    sets = [[int(v) for v in s] for s in list(a_sets) + list(b_sets)]
    na, nb = len(a_sets), len(b_sets)
    lens = [min(len(s), limit) if limit else len(s) for s in sets]
    start = [0] * len(sets)
    sh, tt = np.zeros((na, nb), U32), np.zeros((na, nb), U32)
    rounds = 0
    while True:
        rounds += 1
        cands = [sets[s][start[s] + window] for s in range(len(sets)) if lens[s] - start[s] > window]
        last = not cands
        wins = []
        for s in range(len(sets)):
            win = sets[s][start[s]:start[s] + min(lens[s] - start[s], window)]
            if not last:
                win = [v for v in win if v < min(cands)]
            start[s] += len(win)
            wins.append(win)
        for i in range(na):
            for j in range(nb):
                if limit and tt[i, j] >= limit:
                    continue
                ia = ib = 0
                wa, wb = wins[i], wins[na + j]
                while (ia < len(wa) or ib < len(wb)) and not (limit and tt[i, j] >= limit):
                    x = wa[ia] if ia < len(wa) else None
                    y = wb[ib] if ib < len(wb) else None
                    tt[i, j] += 1
                    if x is not None and y is not None and x == y:
                        sh[i, j] += 1
                        ia += 1
                        ib += 1
                    elif y is None or (x is not None and x < y):
                        ia += 1
                    else:
                        ib += 1
        if last or (limit and bool(np.all(tt >= limit))):
            return rounds, sh, tt


def plan_figures(A, B, limit, caps):
    """what bsk_compare_plan reports for A x B: (tiles run, rounds summed over the tiles, most rounds of one tile)"""
    R, Cc, W = caps["CMP_ROWS"], caps["CMP_COLS"], caps["CMP_WINDOW"]
    tiles = total = most = 0
    for i0 in range(0, len(A), R):
        for j0 in range(0, len(B), Cc):
            r = tile_rounds(A[i0:i0 + R], B[j0:j0 + Cc], limit, W)[0]
            tiles, total, most = tiles + 1, total + r, max(most, r)
    return tiles, total, most


def n_tiles(n_a, n_b, caps):
    return -(-n_a // caps["CMP_ROWS"]) * -(-n_b // caps["CMP_COLS"])


# ---- the cases: (A, B, claims) ----
def hand_case():
    """3 x 2 with an empty set; the expected matrices are written out per limit"""
    A = [u64([1, 3, 5, 7]), u64([]), u64([2, 3])]
    B = [u64([3, 4, 5]), u64([7])]
    want = {  # limit -> (shared, total)
        0: ([[2, 1], [0, 0], [1, 0]], [[5, 4], [3, 1], [4, 3]]),
        1: ([[0, 0], [0, 0], [0, 0]], [[1, 1], [1, 1], [1, 1]]),
        2: ([[1, 0], [0, 0], [1, 0]], [[2, 2], [2, 1], [2, 2]]),
        3: ([[1, 0], [0, 0], [1, 0]], [[3, 3], [3, 1], [3, 3]]),
        100: ([[2, 1], [0, 0], [1, 0]], [[5, 4], [3, 1], [4, 3]]),
    }
    return A, B, want


def window_edges(W, seed=11):
    """sizes 0, 1, W-1, W, W+1, 2W, 2W+1, 3W+5 from a pool of 4W values, all against all; the limits to run"""
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.choice(1 << 40, 4 * W, replace=False).astype(U64))
    sizes = [0, 1, W - 1, W, W + 1, 2 * W, 2 * W + 1, 3 * W + 5]
    A = [np.sort(rng.choice(pool, n, replace=False)) for n in sizes]
    B = [np.sort(rng.choice(pool, n, replace=False)) for n in sizes]
    limits = [0, 1, W - 1, W, W + 1, 2 * W + 1, 8 * W + 1]  # the last is beyond every union (a union holds at most the pool)
    return A, B, dict(sizes=sizes, limits=limits, pool=4 * W)


def tile_edges(R, Cc, seed=12):
    """(n_a, n_b) shapes around the tile, sets of about 20 values from a pool of 60"""
    rng = np.random.default_rng(seed)
    big = max(2 * R + 1, 2 * Cc + 1)
    sets = [np.sort(rng.choice(60, int(rng.integers(15, 26)), replace=False).astype(U64)) * U64(0x9E3779B97F4A7C15) for _ in range(2 * big)]
    sets = [np.sort(s) for s in sets]
    shapes = [(na, nb) for na in (1, R - 1, R, R + 1, 2 * R + 1) for nb in (1, Cc - 1, Cc, Cc + 1, 2 * Cc + 1)]
    return sets[:big], sets[big:], dict(shapes=shapes)


def extreme_values(W):
    """0 and 2^64-1 in both sets, in one, in neither; {2^64-1} alone; a set whose W-th and (W+1)-th values are 2^64-2 and 2^64-1"""
    mid = [5, 1 << 33, 1 << 63]
    edge = list(range(1000, 1000 + W - 1)) + [MAX - 1, MAX]  # W + 1 values: the window boundary falls between the last two
    sets = [u64([0] + mid + [MAX]), u64([0] + mid), u64(mid + [MAX]), u64(mid), u64([MAX]), u64([0]), u64([0, MAX]), u64(edge),
            u64(edge[:-1]), u64(list(range(1000, 1000 + W)) + [MAX])]
    return sets, sets, dict(edge_index=7, limits=[0, 1, 2, 4, W, W + 1])


def skew_cases(W):
    """name -> (A, B): one set races ahead of, or stalls behind, the others of its tile"""
    low = u64(range(1, 5 * W + 1))  # 5W values below everything else
    others = [u64(range(10 * W + i, 10 * W + i + 40)) for i in range(5)]
    gap = u64(range(20 * W, 23 * W))  # 3W values where the others hold nothing
    around = [u64(list(range(10 * W + i, 10 * W + i + 30)) + list(range(30 * W + i, 30 * W + i + 30))) for i in range(5)]
    dense = u64(range(0, 20 * W, 2))  # 10W values
    rng = np.random.default_rng(13)
    sparse = [np.sort(rng.choice(20 * W, 3, replace=False).astype(U64)) for _ in range(15)]
    return {
        "low": ([low] + others, others),
        "gap": ([gap] + around, around),
        "dense": ([dense], sparse),
        "dense_t": (sparse, [dense]),
    }


def limit_landings():
    """pairs with the limit on a shared value, on the value before one and on the value after one, at |union| and |union| + 1, identical
    sets below their size and disjoint sets: (a, b, limit, shared, total)"""
    a, b = u64([10, 20, 30, 40, 50]), u64([5, 20, 35, 40, 60])  # union 5 10 20 30 35 40 50 60, shared 20 40
    ident = u64(range(100, 140))
    return [
        (a, b, 3, 1, 3),   # the 3rd value of the union is the shared 20
        (a, b, 2, 0, 2),   # ... the 2nd, 10, is the value before it
        (a, b, 4, 1, 4),   # ... the 4th, 30, the value after it
        (a, b, 6, 2, 6),   # on the shared 40
        (a, b, 8, 2, 8),   # limit = |union|
        (a, b, 9, 2, 8),   # limit = |union| + 1
        (ident, ident, 7, 7, 7),
        (ident, ident, 39, 39, 39),
        (u64([1, 3, 5]), u64([2, 4, 6]), 4, 0, 4),
        (u64([1, 3, 5]), u64([2, 4, 6]), 0, 0, 6),
    ]


def mash_shape(seed=14):
    """40 sets of 1 000 values from a pool of 3 000, limit 1 000"""
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.choice(1 << 62, 3000, replace=False).astype(U64))
    sets = [np.sort(rng.choice(pool, 1000, replace=False)) for _ in range(40)]
    return sets, dict(limit=1000)


def small_pool_sets(n, seed=15):
    """n sets of 2-3 values from the pool 0 .. 63, and their bit masks (u64): what a vectorised reference works on"""
    rng = np.random.default_rng(seed)
    picks = rng.integers(0, 64, (n, 3))
    picks[:, 1] = (picks[:, 0] + 1 + rng.integers(0, 63, n)) % 64  # two distinct values ...
    two = rng.random(n) < 0.5
    picks[two, 2] = picks[two, 1]                                  # ... and for half of the sets no third
    masks = np.zeros(n, U64)
    for k in range(3):
        masks |= U64(1) << picks[:, k].astype(U64)
    sets = [np.array([k for k in range(64) if (int(m) >> k) & 1], U64) for m in masks]
    return sets, masks


def popcount(x):
    x = x.astype(U64)
    c = np.zeros(x.shape, U32)
    for k in range(64):
        c += ((x >> U64(k)) & U64(1)).astype(U32)
    return c


def mask_compare(ma, mb):
    """limit 0 on bit-mask sets: shared = popcount(a & b), total = popcount(a | b)"""
    return popcount(ma[:, None] & mb[None, :]), popcount(ma[:, None] | mb[None, :])


def bottom_sets(seed=16):
    """set sizes 0 .. 70 and 1 025"""
    rng = np.random.default_rng(seed)
    sizes = list(range(0, 71)) + [1025]
    return [np.sort(rng.choice(1 << 50, n, replace=False).astype(U64)) for n in sizes], sizes


def mutated_sequences(length=200_000, rates=(0.0, 0.01, 0.05), seed=17):
    """one random sequence, copies with substitutions at the given rates, and an unrelated one: list of ASCII byte strings"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    base = rng.integers(0, 4, length)
    seqs = [acgt[base].tobytes()]
    for rate in rates:
        m = base.copy()
        hit = rng.random(length) < rate
        m[hit] = (m[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        seqs.append(acgt[m].tobytes())
    seqs.append(acgt[rng.integers(0, 4, length)].tobytes())
    return seqs
