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

Syncmer reads have no guards; a layout is kept when random flanks give it teeth.  Besides the reads of one length per W
(build_syncmer_reads, SYN_CELLS) there are three sets for the places such reads never reach (SYN_CELLS2):
  * SEAM reads (build_syncmer_seam_reads): the pair at a tile seam m tp.  syncmer_positions_tiled is a CPU model of the tiling rule --
    the header of kernels_tile.hpp restated, no kernel -- that takes a selection rule PER TILE; a seam read is labelled 'before' / 'after'
    when tile m - 1 / tile m ALONE selecting by key changes the stitched positions, and every (d < W, orientation, label) must be covered
    at every W (SEAM_LEFT_OUT names the classes left out, with the reason: none).  Default tiles report no size, so their reads
    (build_syncmer_default_tile_reads: 449 .. 1 500 bases, the pair across a multiple of 16) carry read-level teeth only;
  * LONG-PLAN reads (build_syncmer_long_reads): the same layouts at lengths the planner gives to k_syncmer_pkl<W> for W <= 20;
  * RAGGED reads (build_syncmer_ragged_reads, with_ragged_neighbours): the pair in the last two blocks, the neighbours in batch order
    3W .. 6W bases longer.
SYN_PLANS names the kernel every case must report, SYN_REACH the (kernel, W) pairs the cases reach with a tie read.
"""
from __future__ import annotations

import json
import os
import random

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from tests import plan_atlas as PA

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


def build_syncmer_reads(O, w, seed, places=("first", "interior", "last"), length=None, cases=None):
    """-> {s: tie reads}, layouts given up.  Read length s + 7w + 4 + (i mod w): windows enough for the fused and the staged kernels
    (a pair of reads selects ~9 rows of k_syncmer_pk's 23); or length(s, e), e = 0..w-1.  cases: syncmer_cases(w) unless given; a case
    (d, residue, side, e) names its e itself, and cases (d, residue, side, e, group) are alternatives: the first of a group that has
    teeth is kept, and a group counts as given up when none has"""
    rng = random.Random(seed)
    out, lost = {}, 0
    kept, failed = set(), set()   # groups of alternatives
    for i, (d, r, side, *opt) in enumerate(syncmer_cases(w) if cases is None else cases):
        group = opt[1] if len(opt) > 1 else None
        if group is not None and group in kept:
            continue
        s = syn_s(d)
        k = s + w
        e = fixture("syncmer", s, d, side)
        assert e is not None, (s, d, side)
        core = e["core"]
        place = places[i % len(places)]
        ei = opt[0] if opt else (i // len(places)) % w
        n_bases = s + 7 * w + 4 + ei if length is None else length(s, ei)
        ns = n_bases - s + 1
        a = _place(place, r, d, w, ns, i)
        for _ in range(SYN_TRIES if a is not None else 0):
            seq = rand_seq(rng, a) + core + rand_seq(rng, n_bases - a - len(core))
            if _has_teeth(O, seq, "syncmer", k, w, s, a, d, side):
                out.setdefault(s, []).append(TieRead(seq, k, w, s, d, a, side, place))
                if group is not None:
                    kept.add(group)
                break
        else:
            if group is None:
                lost += 1
            else:
                failed.add(group)
    return out, lost + len(failed - kept)


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


# ---- syncmers over tiles: a CPU model of the tiling rule (the header of kernels_tile.hpp, restated; no kernel) ------------------------
def _syncmer_b(hs, k, s, n_bases, rule):
    """b(idx), the k-mer the 2w window at idx selects, for idx = 0 .. end (before emit-when-changed)"""
    w = k - s
    npos = n_bases + s + 2 - 2 * k
    win = sliding_window_view(hs, 2 * w)[:npos]
    idx = np.arange(npos)
    mi = idx + _argmin(win, rule)
    return np.where(mi - idx < w, mi, mi - w)


def _tile_out(b, w, tp, j):
    """what tile j keeps of the selections b(idx): idx max(0, P0 - w + 1) .. P1 - 1, emitted when they change, positions in [P0, P1)"""
    p0 = j * tp
    p1 = min(p0 + tp, len(b))
    v = _dedupe(b[max(0, p0 - w + 1):p1])
    return v[(v >= p0) & (v < p1)]


def syncmer_positions_tiled(hs, k, s, n_bases, tp, rule_of_tile=lambda j: "exact"):
    """the closed syncmer of syncmer_positions, computed as the tile path does: tile j owns positions [j tp, min((j + 1) tp, npos)),
    npos = n_bases + s + 2 - 2k; it evaluates idx max(0, P0 - w + 1) .. P1 - 1 with the selection rule rule_of_tile(j) ('exact', 'left'
    or 'right': _argmin), emits a selection when it changes and keeps the positions of its own range; the tiles are concatenated"""
    hs = np.asarray(hs, np.uint64)
    w = k - s
    npos = n_bases + s + 2 - 2 * k
    if npos <= 0:
        return np.zeros(0, np.int64)
    bs, out = {}, []
    for j in range((npos + tp - 1) // tp):
        rule = rule_of_tile(j)
        if rule not in bs:
            bs[rule] = _syncmer_b(hs, k, s, n_bases, rule)
        out.append(_tile_out(bs[rule], w, tp, j))
    return np.concatenate(out)


def tile_teeth(hs, k, s, n_bases, tp, tiles):
    """those of `tiles` in which a key-only rule ('left' or 'right') selects otherwise than the exact one -- the tiles keep disjoint ranges,
    so that is where replacing the rule of that ONE tile changes the stitched positions (test_key_tie_fixtures shows it on the model)"""
    hs = np.asarray(hs, np.uint64)
    w = k - s
    b = {r: _syncmer_b(hs, k, s, n_bases, r) for r in ("exact", "left", "right")}
    nt = (len(b["exact"]) + tp - 1) // tp
    return [j for j in tiles if 0 <= j < nt and
            any(not np.array_equal(_tile_out(b["exact"], w, tp, j), _tile_out(b[r], w, tp, j)) for r in ("left", "right"))]


class SeamRead(TieRead):
    """a tie read whose pair lies at the seam m tp: labels 'before' (tile m - 1 has teeth) and / or 'after' (tile m has)"""
    __slots__ = ("tp", "m", "labels")


SEAM_DRAWS = 400  # seeded draws of (seam, offset, flanks) per (d, side) before a label is given up


def syn_seam_bases(k, tp):
    """length of a seam read: a dozen small tiles or five large ones, and room for the core at every seam inside"""
    return 12 * tp + 3 * k if tp <= 16 else 5 * tp + 3 * k + 40


def build_syncmer_seam_reads(O, w, tp, seed):
    """random flank + core + random flank with the core's left s-mer at m tp - x, 0 <= x <= w + d, for a seam m tp inside the read; every
    d < w, both orientations.  Kept per (d, side): the first read with teeth in tile m - 1 ('before') and the first with teeth in tile m
    ('after'; one read may be both).  -> (reads, [(d, side, label) not reached in SEAM_DRAWS draws])"""
    rng = random.Random(seed)
    out, lost = [], []
    for d in range(1, w):
        s = syn_s(d)
        k = s + w
        n_bases = syn_seam_bases(k, tp)
        ntiles = (n_bases + s + 2 - 2 * k + tp - 1) // tp
        for side in ("left", "right"):
            core = fixture("syncmer", s, d, side)["core"]
            have = {}
            for _ in range(SEAM_DRAWS):
                m, x = rng.randint(1, ntiles - 1), rng.randint(0, w + d)
                a = m * tp - x
                if a < 0 or a + len(core) > n_bases:
                    continue
                seq = rand_seq(rng, a) + core + rand_seq(rng, n_bases - a - len(core))
                got = tile_teeth(O.nthash(seq, s)[0], k, s, n_bases, tp, (m - 1, m))
                labels = tuple(lab for j, lab in ((m - 1, "before"), (m, "after")) if j in got)
                if any(lab not in have for lab in labels):
                    t = SeamRead(seq, k, w, s, d, a, side, "seam")
                    t.tp, t.m, t.labels = tp, m, labels
                    for lab in labels:
                        have.setdefault(lab, t)
                    if len(have) == 2:
                        break
            for lab in ("before", "after"):
                if lab not in have:
                    lost.append((d, side, lab))
                elif not any(have[lab] is t for t in out):
                    out.append(have[lab])
    return out, lost


def missing_seam_classes(reads, w):
    """the (d, side, label) classes, d < w, that no seam read covers"""
    have = {(t.d, t.side, lab) for t in reads for lab in t.labels}
    return [(d, side, lab) for d in range(1, w) for side in ("left", "right") for lab in ("before", "after") if (d, side, lab) not in have]


# ---- the long staged plan for W <= 20, and ragged ends ------------------------------------------------------------------------------
def syn_long_range(w, s):
    """(lo, hi): the read lengths make_plan_enc gives to k_syncmer_pkl<W>, W <= 20, at k = s + w -- more rows than the short column's 23,
    fewer than the long one's 58 (tests/plan_atlas.py restates the rule: syn_pk_fits; its row syn_pkl<W>)"""
    k, base = s + w, s + 7 * w + 4
    lo = PA._longest(lambda ln: PA.syn_pk_fits(k, s, ln, False), base, PA.SYN_SHORT_BASES) + 1
    return lo, PA._longest(lambda ln: PA.syn_pk_fits(k, s, ln, True), lo, PA.SYN_LONG_BASES)


def syn_short_top(w, s):
    """the longest read k_syncmer_pk<W> takes at k = s + w (k_syncmer_pf<W> takes it too: its rule is the wider one up to there)"""
    k = s + w
    return PA._longest(lambda ln: PA.syn_pk_fits(k, s, ln, False), s + 2 * w, PA.SYN_SHORT_BASES)


def syn_long_bases(w, s, e):
    lo, hi = syn_long_range(w, s)
    return (lo + hi) // 2 + e


def _last_block_cases(w, bases, ds, group):
    """'last' placements that can have teeth, as groups of alternatives for build_syncmer_reads.  Only the positions 0 .. end = ns - 2w
    are selectable, so of the 'last' placements, whose left s-mer is q = d + 1 .. d + w before the read's end, those with q < w have no
    teeth (the pair then lies in the right half of every window that holds it whole, and the k-mer of the larger element, w to the left of
    it, is selected either way or not at all).  For every e and orientation and every d of ds(e): q = w .. w + d in turn, from another
    one at every e; the block offset follows from q.  bases(s, e): the read length; group(d, side, e): what one read is wanted for"""
    cases = []
    for side in ("left", "right"):
        for e in range(w):
            for d in ds(e):
                ns = bases(syn_s(d), e) - syn_s(d) + 1
                cases += [(d, (ns - w - (e + j) % (d + 1)) % w, side, e, group(d, side, e)) for j in range(d + 1)]
    return cases


def build_syncmer_long_reads(O, w, seed):
    """the layouts of build_syncmer_reads at lengths around the middle of syn_long_range, + (i mod w); and, because few of its 'last'
    placements can have teeth (_last_block_cases), one more read per orientation and ns mod w with a pair d < w apart in the last blocks"""
    bases = lambda s, e: syn_long_bases(w, s, e)
    out, lost = build_syncmer_reads(O, w, seed, length=bases)
    ds = lambda e: [1 + (7 * e + j) % (w - 1) for j in range(w - 1)]
    more, lost2 = build_syncmer_reads(O, w, seed + 1, places=("last",), length=bases, cases=_last_block_cases(w, bases, ds, lambda d, side, e: (side, e)))
    for s, v in more.items():
        out.setdefault(s, []).extend(v)
    return out, lost + lost2


def syn_ragged_bases(w, s, e):
    """a ragged tie read: 5w + e bases below the plan's longest read, so that neighbours 3w .. 6w longer fit the same plan"""
    return syn_short_top(w, s) - 5 * w - e


def build_syncmer_ragged_reads(O, w, seed):
    """every d < w in both orientations, each at four read lengths a quarter of w apart (all of them at w = 4), so that the reads of
    every orientation meet every ns mod w; the pair in the read's last two blocks (_last_block_cases)"""
    bases = lambda s, e: syn_ragged_bases(w, s, e)
    ds = lambda e: [d for d in range(1, w) if any((d + j * max(1, w // 4)) % w == e for j in range(4))]
    return build_syncmer_reads(O, w, seed, places=("last",), length=bases, cases=_last_block_cases(w, bases, ds, lambda d, side, e: (d, side, e)))


def ragged_neighbour_range(t):
    """(lo, hi) lengths of a ragged tie read's plain neighbours: 3w .. 6w bases longer, within the short plan's longest read"""
    return len(t.seq) + 3 * t.w, min(len(t.seq) + 6 * t.w, syn_short_top(t.w, t.s))


def with_ragged_neighbours(tie_reads, seed):
    """tie reads (one s, one w), each followed by PLAIN_PER_TIE plain reads 3w .. 6w bases longer: the wavefront runs on to its longest
    read, so the tie read's lane overruns its end by three to six blocks.  In batch order.  -> (seqs, index of every tie read)"""
    rng = random.Random(seed)
    seqs, at = [], []
    for t in tie_reads:
        lo, hi = ragged_neighbour_range(t)
        at.append(len(seqs))
        seqs.append(t.seq)
        seqs += [rand_seq(rng, rng.randint(lo, hi)) for _ in range(PLAIN_PER_TIE)]
    while len(seqs) < MIN_READS:
        lo, hi = ragged_neighbour_range(tie_reads[len(seqs) % len(tie_reads)])
        seqs.append(rand_seq(rng, rng.randint(lo, hi)))
    return seqs, at


def chunks(reads, n):
    """reads in batches of at most n (a tie read and its two plain reads each: batches below the planner's length-binning threshold)"""
    return [reads[i:i + n] for i in range(0, len(reads), n)]


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


# ---- syncmer ties at tile seams, on the long staged plan and at ragged ends ----------------------------------------------------------
NO_SYN_PF = {"BSK_NO_SYN_PF": "1"}
SYN_TILE_MIN = {"BSK_TILE_MIN": "40"}
DEFAULT_TILE_BASES = (449, 1500)  # sequences the default planner cuts into tiles (longer than PlannerTable::syn_tile_min_bases)
BATCH_TIES = 330                  # tie reads per batch: 990 sequences, below the 1 024 from which the planner bins a ragged batch by length


def _by_w(**names):
    """{w: 'k_syncmer_<name><w>'} from name = the W values planned on it"""
    return {w: "k_syncmer_%s<%d>" % (n, w) for n, ws in names.items() for w in ws}


# The kernel the tiles of a cell are planned on, per W, for the run with the fused-emit kernels ('pf') and the run with BSK_NO_SYN_PF ('pk').
# A forced tile of tp positions is a read of at most tp + 3w + s + 12 bases with tp + w + 14 windows (tiles.hip), and make_plan_enc's rules
# (tests/plan_atlas.py: syn_pk_fits, syn_pf_fits; test_key_tie_fixtures holds this table against them) give: the short staged column
# takes tp + w + 14 <= 6.67 (w + 1) windows -- not W = 4 at tp = 16, not W < 13 at tp = 64 --, the long one 16.3 (w + 1) -- not W = 4 at
# tp = 64: those tiles run on the 64-bit machine k_syncmer_fast<4>, which no key tie can reach; the case stays for the tile path's sake and
# counts for nothing in SYN_REACH --, the fused kernel's short emit list 9.17 (w + 1) -- not W = 8 at tp = 64.  W >= 21 has long forms only.
# Default tiles are sized for the long plan's columns (tile_positions), so they run on k_syncmer_pfl<W>, W >= 8, and k_syncmer_pkl<W> below.
SYN_PLANS = {
    ("syn_tiles16", "pk"): _by_w(pkl=(4, 21, 22, 23, 24), pk=range(5, 21)),
    ("syn_tiles16", "pf"): _by_w(pkl=(4,), pk=(5, 6, 7), pf=range(8, 21), pfl=range(21, 25)),
    ("syn_tiles64", "pk"): _by_w(fast=(4,), pkl=tuple(range(5, 13)) + (21, 22, 23, 24), pk=range(13, 21)),
    ("syn_tiles64", "pf"): _by_w(fast=(4,), pkl=(5, 6, 7), pfl=(8, 21, 22, 23, 24), pf=range(9, 21)),
    ("syn_tiles_default", "pf"): _by_w(pkl=range(4, 8), pfl=range(8, 25)),
    ("syn_long", "pk"): _by_w(pkl=range(4, 21)),
    ("syn_ragged", "pk"): _by_w(pk=range(4, 21)),
    ("syn_ragged", "pf"): _by_w(pf=range(8, 21)),
}
SYN_TILE_WS = tuple(range(4, 25))  # forced tiles: every W (a W's seam reads are built in a tenth of a second)
# (cell, env without the fused / staged switch, suffix the plan string must end in, W values of the 'pf' run, W values of the 'pk' run)
SYN_CELLS2 = [
    ("syn_tiles16", dict(SYN_TILE_MIN, BSK_TILE_POS="16"), PA.TILES, SYN_TILE_WS, SYN_TILE_WS),
    ("syn_tiles64", dict(SYN_TILE_MIN, BSK_TILE_POS="64"), PA.TILES, SYN_TILE_WS, SYN_TILE_WS),
    ("syn_tiles_default", {}, PA.TILES, tuple(range(4, 25)), ()),
    ("syn_long", {}, "", (), tuple(range(4, 21))),
    ("syn_ragged", {}, "", tuple(range(8, 21)), tuple(range(4, 21))),
]
SYN_CASES2 = [(cell, mode, w) for cell, _, _, wf, wk in SYN_CELLS2 for mode, ws in (("pf", wf), ("pk", wk)) for w in ws]
# the (kernel, W) pairs the cells above run a tie read on: every packed syncmer instantiation of the build
SYN_REACH = ({("k_syncmer_pk", w) for w in range(4, 21)} | {("k_syncmer_pkl", w) for w in range(4, 25)} |
             {("k_syncmer_pf", w) for w in range(8, 21)} | {("k_syncmer_pfl", w) for w in range(8, 25)})
# packed instantiations the planner gives to no tie read with s in {24, 11}: {(kernel, W): reason}.  None: k_syncmer_pfl<W> for W <= 20,
# which whole reads reach only with k = 64 or BSK_PF_DENSITY (tests/plan_atlas.py), is what the default tiles of every W >= 8 run on.
SYN_NOT_REACHED = {}
# seam classes (W, tp, d, side, label) left out, with the reason: none
SEAM_LEFT_OUT = {}


def syn_cell_env(cell, mode):
    env = dict(next(c for c in SYN_CELLS2 if c[0] == cell)[1])
    if mode == "pk":
        env.update(NO_SYN_PF)
    return env


def syn_default_tile_bases(w, e):
    lo, hi = DEFAULT_TILE_BASES
    return lo + (hi - lo) * e // (w - 1)


def build_syncmer_default_tile_reads(O, w, seed):
    """sequences of 449 .. 1 500 bases with the pair across a multiple of 16 ('tile' placement: every default tile start is one); every
    d < 2w in both orientations, twice.  The library does not report its tile size: read-level teeth only"""
    cases = [(d, 0, side) for _ in range(2) for d in range(1, 2 * w) for side in ("left", "right")]
    return build_syncmer_reads(O, w, seed, places=("tile",), length=lambda s, e: syn_default_tile_bases(w, e), cases=cases)


def syn_cell_reads(O, cell, w):
    """-> {s: tie reads} of a cell of SYN_CELLS2 (the 'pf' and the 'pk' run of a cell share them)"""
    if cell.startswith("syn_tiles") and cell != "syn_tiles_default":
        reads, lost = build_syncmer_seam_reads(O, w, int(cell[len("syn_tiles"):]), hash_seed(cell, w))
        by_s = {}
        for t in reads:
            by_s.setdefault(t.s, []).append(t)
        return by_s, lost
    build = {"syn_tiles_default": build_syncmer_default_tile_reads, "syn_long": build_syncmer_long_reads, "syn_ragged": build_syncmer_ragged_reads}[cell]
    return build(O, w, hash_seed(cell, w))


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
