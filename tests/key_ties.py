"""Reads that put a crafted ACCIDENTAL 27-bit key tie (tests/golden/key_ties.json, scripts/make_key_ties.py) into every place a packed
window machine can meet it -- shared by tests/test_key_tie_fixtures.py (CPU: the fixtures hold, and every read below has teeth) and
tests/test_gpu_key_ties.py (GPU: every read bit-exact against the oracle's state machine).

A read is random flank + core + random flank, and it must have TEETH: the closed form over the packed keys (hash >> 37), ties broken
leftmost-first or rightmost-first, selects differently from the closed form over the 64-bit hashes -- a machine that ignores the low
37 bits fails that read.  Output positions are emitted when they CHANGE, so a wrong pick inside the pair shows only if the larger
element is never emitted by a window that holds it without the smaller one.  Minimizer reads get that by construction: a GUARD,
a k-mer with a smaller key, sits W positions beyond the smaller element's far side (at b - W when the right element is smaller,
at a + W when the left one is) -- in every window that holds the larger element alone, in none that holds both.  Its free bases are
the flank's next to the core, chosen by enumeration (scripts/make_key_ties.py keeps only cores that have guards for W - d <= 3);
at a read's edge no such window exists and no guard is needed.  The other flank bases are drawn until the pair is the minimum of a
window that holds both.  Everything is seeded: both test modules build the same reads.
"""
from __future__ import annotations

import json
import os
import random

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "key_ties.json")
KEY_SHIFT = 37
TRIES = 40           # flank draws per layout before it is given up (minimizer sets: none may be; test_key_tie_fixtures)
SYN_TRIES = 12       # ... for a syncmer layout (no guards: test_key_tie_fixtures asserts what every W keeps)
PLAIN_PER_TIE = 2    # plain random reads after every tie read: only some lanes of a unit see a tie
MIN_READS = 320      # batches are padded with plain reads to at least this many

_FIX = None


def fixtures():
    global _FIX
    if _FIX is None:
        with open(GOLDEN) as fh:
            _FIX = json.load(fh)
    return _FIX


def fixture(family, k, d, side):
    for e in fixtures()[family]:
        if e["k"] == k and e["d"] == d and e["smaller"] == side:
            return e
    return None


def syn_s(d):
    """the s of the syncmer fixture for s-mers d apart (s = 24: d <= 10, s = 11: d >= 11; scripts/make_key_ties.py)"""
    return 24 if d <= 10 else 11


# ---- closed forms over a hash array: the exact one and the two that look at the key only -----------------------------------------------
def _argmin(win, rule):
    if rule == "exact":
        return win.argmin(axis=1)
    keys = win >> np.uint64(KEY_SHIFT)
    if rule == "left":
        return keys.argmin(axis=1)
    return win.shape[1] - 1 - keys[:, ::-1].argmin(axis=1)  # "right": the rightmost of the equal keys


def _dedupe(pos):
    if len(pos) == 0:
        return pos
    keep = np.ones(len(pos), bool)
    keep[1:] = pos[1:] != pos[:-1]
    return pos[keep]


def minimizer_positions(h, w, rule="exact"):
    """leftmost argmin of every window of w hashes, emitted when it changes (NextMinimizer's closed form); rule 'left' / 'right': over
    h >> 37 with equal keys broken by position"""
    h = np.asarray(h, np.uint64)
    if len(h) < w:
        return np.zeros(0, np.int64)
    win = sliding_window_view(h, w)
    return _dedupe(np.arange(len(win)) + _argmin(win, rule))


def syncmer_positions(hs, k, s, n_bases, rule="exact"):
    """the window-bounded closed syncmer (oracle orc_syncmer_closed) over s-mer hashes hs: the 2w window at idx picks its leftmost
    minimum mI, the selected k-mer is mI (left half) or mI - w; emitted when it changes, dropped beyond the last idx"""
    hs = np.asarray(hs, np.uint64)
    w = k - s
    end = n_bases - 2 * k + s + 1
    if end < 0:
        return np.zeros(0, np.int64)
    win = sliding_window_view(hs, 2 * w)[:end + 1]
    idx = np.arange(end + 1)
    mi = idx + _argmin(win, rule)
    b = _dedupe(np.where(mi - idx < w, mi, mi - w))
    return b[b <= end]


# ---- layouts ----------------------------------------------------------------------------------------------------------------------
class TieRead:
    __slots__ = ("seq", "k", "w", "s", "d", "a", "side", "place")

    def __init__(self, seq, k, w, s, d, a, side, place):
        self.seq, self.k, self.w, self.s, self.d, self.a, self.side, self.place = seq, k, w, s, d, a, side, place


_ACGT = np.frombuffer(b"ACGT", np.uint8)


def rand_seq(rng, n):
    return _ACGT[np.frombuffer(rng.randbytes(n), np.uint8) & 3].tobytes().decode() if n > 0 else ""


def _has_teeth(O, seq, kind, k, w, s, a, d, side):
    if kind == "minimizer":
        h = O.nthash(seq, k)[0]
        ex = minimizer_positions(h, w)
        if (a if side == "left" else a + d) not in ex:  # the true minimum of the pair is selected
            return False
        return any(not np.array_equal(ex, minimizer_positions(h, w, r)) for r in ("left", "right"))
    hs = O.nthash(seq, s)[0]
    ex = syncmer_positions(hs, k, s, len(seq))
    return any(not np.array_equal(ex, syncmer_positions(hs, k, s, len(seq), r)) for r in ("left", "right"))


def _place(place, r, d, w, n, i):
    """start a of the pair among n elements (k-mers or s-mers): block offset r in the first block, an interior block or the last
    (partial) block; 'tile': across a multiple of 16 (every tile boundary is one)"""
    if place == "first":
        a = r
    elif place == "interior":
        a = w * max(1, (n // w) // 2) + r
    elif place == "last":
        a = ((n - 1 - d - r) // w) * w + r
    else:
        m = 1 + (i * 7) % max(1, (n - d) // 16 - 1)
        a = 16 * m - 1 - (i % d)
    return a if 0 <= a and a + d <= n - 1 else None


GUARD_ENUM = 3  # flank bases next to the core a guard is enumerated over (the fixtures guarantee one for W - d <= 3)


def _guard(O, rng, flank, core, k, d, t, key, top, side):
    """the flank with the bases next to the core set so that the guard's key is below `key` and the t - 1 k-mers between the guard
    and the pair are above `top` (the pair's larger hash: they share windows with the pair), or None.  side 'right' (the right
    element smaller): flank is the LEFT flank, the guard starts t bases before the core; 'left': flank is the RIGHT flank, the guard
    starts t positions after the right element (scripts/make_key_ties.py guard_ok: the same rule)"""
    e = min(t, GUARD_ENUM)
    opts = list(range(4 ** e))
    rng.shuffle(opts)
    for c in opts:
        x = "".join("ACGT"[(c >> (2 * j)) & 3] for j in range(e))
        if side == "right":
            f = flank[:len(flank) - e] + x
            g = f[len(f) - t:] + core[:k - 1]
        else:
            f = x + flank[e:]
            g = core[d + 1:d + k] + f[:t]
        h = O.nthash(g, k)[0]
        gi = 0 if side == "right" else len(h) - 1
        if int(h[gi]) >> KEY_SHIFT < key and all(int(v) > top for j, v in enumerate(h) if j != gi):
            return f
    return None


def build_minimizer_reads(O, k, w, length, seed, places=("first", "interior", "last")):
    """every d < w at every start residue mod w, both orientations, at every one of `places`; read length length(j mod w) for the j-th
    case of a placement, so that every placement sees every nk mod w.  -> (tie reads, number of layouts given up)"""
    rng = random.Random(seed)
    per_place = [(d, r, side) for d in range(1, w) for r in range(w) for side in ("left", "right")]
    cases = [(place, j, c) for place in places for j, c in enumerate(per_place)]
    out, lost = [], 0
    for i, (place, j, (d, r, side)) in enumerate(cases):
        e = fixture("minimizer", k, d, side)
        assert e is not None, (k, d, side)
        core = e["core"]
        n_bases = length(j % w)
        nk = n_bases - k + 1
        a = _place(place, r, d, w, nk, i)
        if a is None:
            lost += 1
            continue
        key, top = int(e["hash_a"]) >> KEY_SHIFT, max(int(e["hash_a"]), int(e["hash_b"]))
        t = w - d  # the guard is t positions beyond the smaller element: at a - t (right smaller) or b + t (left smaller)
        for _ in range(TRIES):
            left, right = rand_seq(rng, a), rand_seq(rng, n_bases - a - len(core))
            if side == "right" and a - t >= 0:
                left = _guard(O, rng, left, core, k, d, t, key, top, "right")
            elif side == "left" and a + d + t <= nk - 1:
                right = _guard(O, rng, right, core, k, d, t, key, top, "left")
            if left is None or right is None:
                continue
            seq = left + core + right
            if _has_teeth(O, seq, "minimizer", k, w, 0, a, d, side):
                out.append(TieRead(seq, k, w, 0, d, a, side, place))
                break
        else:
            lost += 1
    return out, lost


def syncmer_cases(w):
    """(d, residue, side): every d < w at every residue, and every d in [w, 2w) at residue d mod w.  Syncmer reads have no guards: a
    layout is kept when random flanks give it teeth -- every (d, side) with d < w keeps reads (test_key_tie_fixtures), the pairs d >= w
    apart (they meet only in a window's combination of its two halves) only some"""
    c = [(d, r, side) for d in range(1, w) for r in range(w) for side in ("left", "right")]
    c += [(d, d % w, side) for d in range(w, 2 * w) for side in ("left", "right")]
    return c


def build_syncmer_reads(O, w, seed, places=("first", "interior", "last")):
    """-> {s: tie reads}, layouts given up.  Read length s + 7w + 4 + (i mod w): windows enough for the fused and the staged kernels
    (a pair of reads selects ~9 rows of k_syncmer_pk's 23)"""
    rng = random.Random(seed)
    out, lost = {}, 0
    for i, (d, r, side) in enumerate(syncmer_cases(w)):
        s = syn_s(d)
        k = s + w
        e = fixture("syncmer", s, d, side)
        assert e is not None, (s, d, side)
        core = e["core"]
        place = places[i % len(places)]
        n_bases = s + 7 * w + 4 + (i // len(places)) % w
        ns = n_bases - s + 1
        a = _place(place, r, d, w, ns, i)
        if a is None:
            lost += 1
            continue
        for _ in range(SYN_TRIES):
            seq = rand_seq(rng, a) + core + rand_seq(rng, n_bases - a - len(core))
            if _has_teeth(O, seq, "syncmer", k, w, s, a, d, side):
                out.setdefault(s, []).append(TieRead(seq, k, w, s, d, a, side, place))
                break
        else:
            lost += 1
    return out, lost


def with_plain_reads(tie_reads, seed):
    """tie reads, each followed by PLAIN_PER_TIE random reads of its length, padded to MIN_READS -> (seqs, index of every tie read)"""
    rng = random.Random(seed)
    seqs, at = [], []
    for t in tie_reads:
        at.append(len(seqs))
        seqs.append(t.seq)
        seqs += [rand_seq(rng, len(t.seq)) for _ in range(PLAIN_PER_TIE)]
    while len(seqs) < MIN_READS:
        seqs.append(rand_seq(rng, len(tie_reads[len(seqs) % len(tie_reads)].seq)))
    return seqs, at


# ---- the GPU matrix ---------------------------------------------------------------------------------------------------------------
MIN_K = 21
# read sets: (W values, read length of e = 0..W-1, placements).  Cells that share a set run the same reads.
MIN_SETS = {
    "short": (range(2, 14), lambda e: 140 + e, ("first", "interior", "last")),      # ~150 bases
    "long": (range(2, 14), lambda e: 260 + e, ("first", "interior", "last")),       # beyond pk_minimizer_short_bases()
    "pkd": (range(2, 14), lambda e: 320 + 29 * e, ("first", "interior", "last")),   # 320..668 bases
    "tiles": (range(2, 14), lambda e: 300 + e, ("tile",)),                          # across tile boundaries
}
# (cell, env, read set, W values, plan substring with %d = W)
MIN_CELLS = [
    ("pk", {"BSK_NO_RING": "1", "BSK_NO_DENSE": "1"}, "short", range(2, 14), "k_minimizer_pk<%d,false>"),
    ("pk_long", {"BSK_NO_RING": "1", "BSK_NO_DENSE": "1"}, "long", range(2, 14), "k_minimizer_pk<%d,true>"),
    ("ring", {"BSK_RING": "1"}, "long", range(2, 14), "k_minimizer_ring<%d,"),
    ("pkd", {"BSK_NO_RING": "1"}, "pkd", range(2, 14), "k_minimizer_pkd<%d>"),
    ("tiles16", {"BSK_TILE_MIN": "40", "BSK_TILE_POS": "16"}, "tiles", (2, 4, 7, 10, 13), "(over tiles)"),
    ("tiles64", {"BSK_TILE_MIN": "40", "BSK_TILE_POS": "64"}, "tiles", (2, 4, 7, 10, 13), "(over tiles)"),
    ("pft", {"BSK_TILE_MIN": "40", "BSK_TILE_DENSE": "1"}, "tiles", range(4, 14), "k_minimizer_pft<%d>"),
]
# other k on the headline kernel: k = 15 and 31, and k = 40 > 32.  (k = 15 at small W only: its pairs d = 1, 2 apart have 16-17 free
# bases against 27 equations, so they cannot also be made small, and in a window of more than five k-mers they are seldom its minimum)
MIN_OTHER_K = [(15, (3, 5)), (31, (3, 11)), (40, (2, 9, 13))]
# (cell, env, W values, plan name of W); both cells run the same reads (build_syncmer_reads)
SYN_CELLS = [
    ("pf", {}, range(8, 25), lambda w: "k_syncmer_pf<%d>" % w if w <= 20 else "k_syncmer_pfl<%d>" % w),
    ("pk", {"BSK_NO_SYN_PF": "1"}, range(4, 25), lambda w: "k_syncmer_pk<%d>" % w if w <= 20 else "k_syncmer_pkl<%d>" % w),
]


def missing_classes(reads, w, ds=None):
    """the (d, side) classes, d < w (or d in ds), that no read covers"""
    have = {(t.d, t.side) for t in reads}
    return [(d, side) for d in (ds or range(1, w)) for side in ("left", "right") if (d, side) not in have]


def min_set_reads(O, name, w, k=MIN_K):
    ws, length, places = MIN_SETS[name]
    return build_minimizer_reads(O, k, w, length, seed=hash_seed(name, k, w), places=places)


def syn_reads(O, w):
    return build_syncmer_reads(O, w, seed=hash_seed("syncmer", w))


def hash_seed(*parts):
    v = 1469598103934665603
    for p in parts:
        for ch in str(p):
            v = ((v ^ ord(ch)) * 1099511628211) & ((1 << 64) - 1)
    return v
