#!/usr/bin/env python3
"""Write tests/golden/key_ties.json: crafted ACCIDENTAL 27-bit key ties for the packed window machines.

The packed minimizer and syncmer machines (kernels_pk.hpp, kernels_ring.hpp, kernels_syncmer_pk.hpp) compare one 32-bit word per
element: the upper 27 bits of the canonical ntHash and a slot number.  That word gives the 64-bit leftmost minimum unless two elements
of a window share the minimal 27-bit key, which every min operation checks (tmin = min(a ^ b) < 32).  Each fixture here is a short
core string holding two k-mers (or s-mers) d positions apart with EQUAL upper 27 bits, DIFFERENT canonical hashes (so no real tie and
no first-window flag) and hashes smaller than every k-mer between them, in both orientations: the left element smaller, and the right.

How they are found.  ntHash is XOR-linear in its seeds.  Restrict base j of the core to a random pair of letters {P0_j, P1_j}: then
seed(x_j) = seed(P0_j) ^ u_j (seed(P0_j) ^ seed(P1_j)) and the forward (or reverse) hash of every k-mer of the core is an affine
function of the bits u over GF(2).  "Equal upper 27 bits" is 27 linear equations, "top z bits zero" z more (a small pair tends to be
the window's minimum); Gaussian elimination solves them, and each solution is checked against oracle.nthash (the canonical strand
must be the one the equations assumed).  Deterministic: the same seed writes the same file byte for byte.

    python scripts/make_key_ties.py            # writes tests/golden/key_ties.json
"""
from __future__ import annotations

import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "key_ties.json")
M64 = (1 << 64) - 1
KEY_SHIFT = 37  # the packed word keeps hash >> 37 (27 bits)

# what the GPU tests need: minimizer k with every d = 1..12 (W = 2..13), syncmer s with every d < 2W for W up to 24 (the s-mer
# window of the closed syncmer is 2W wide).  Overlapping s-mers of s = 11 hardly ever tie (4^(11+d) strings against 2^27 keys), so
# s = 24 covers d <= 10 by the linear system, and s = 11 covers d >= 11 = s: two whole s-mers from the 4^11 with the smallest equal keys.
MIN_SET = [(21, d) for d in range(1, 13)] + [(15, d) for d in range(1, 13)] + [(31, d) for d in range(1, 13)] + \
          [(40, d) for d in range(1, 13)]
SYN_SET = [(24, d) for d in range(1, 11)]
SYN_S, SYN_D = 11, range(11, 48)


def rol(v, n):
    n &= 63
    return ((v << n) | (v >> (64 - n))) & M64 if n else v


def seeds():
    L = O.lib()
    f = {c: int(L.orc_seed_fwd(ord(c))) for c in "ACGT"}
    r = {c: int(L.orc_seed_rev(ord(c))) for c in "ACGT"}
    return f, r


def solve(rows, n, rng):
    """rows: list of (mask over n unknowns, rhs).  A random solution (list of bits) or None."""
    piv = {}  # pivot column -> (mask, rhs); no pivot row holds another pivot's column
    for m, b in rows:
        for c, (pm, pb) in piv.items():
            if (m >> c) & 1:
                m ^= pm
                b ^= pb
        if m == 0:
            if b:
                return None
            continue
        c = m.bit_length() - 1
        for pc, (pm, pb) in list(piv.items()):
            if (pm >> c) & 1:
                piv[pc] = (pm ^ m, pb ^ b)
        piv[c] = (m, b)
    u = [0 if j in piv else rng.getrandbits(1) for j in range(n)]
    for c, (m, b) in piv.items():  # u_c = rhs ^ the free variables of its row
        v = b
        mm = m & ~(1 << c)
        while mm:
            j = (mm & -mm).bit_length() - 1
            v ^= u[j]
            mm &= mm - 1
        u[c] = v
    return u


def affine(f, r, P0, P1, start, k, strand):
    """hash of the k-mer at core offset `start` as  const ^ XOR_j u_j col_j : (const, {j: col})"""
    const, cols = 0, {}
    for t in range(k):
        j = start + t
        s0 = f[P0[j]] if strand == 0 else r[P0[j]]
        s1 = f[P1[j]] if strand == 0 else r[P1[j]]
        rot = k - 1 - t if strand == 0 else t
        const ^= rol(s0, rot)
        cols[j] = rol(s0 ^ s1, rot)
    return const, cols


def attempt(f, r, k, d, z, rng):
    n = k + d
    P0, P1 = [], []
    for _ in range(n):
        a, b = rng.sample("ACGT", 2)
        P0.append(a)
        P1.append(b)
    sa, sb = rng.getrandbits(1), rng.getrandbits(1)
    ca, cola = affine(f, r, P0, P1, 0, k, sa)
    cb, colb = affine(f, r, P0, P1, d, k, sb)
    rows = []
    for bit in range(KEY_SHIFT, 64):          # equal keys: bit of hA ^ hB is 0
        m = 0
        for j in range(n):
            if ((cola.get(j, 0) ^ colb.get(j, 0)) >> bit) & 1:
                m |= 1 << j
        rows.append((m, ((ca ^ cb) >> bit) & 1))
    for bit in range(64 - z, 64):             # small keys: bit of hA is 0
        m = 0
        for j in range(n):
            if (cola.get(j, 0) >> bit) & 1:
                m |= 1 << j
        rows.append((m, (ca >> bit) & 1))
    u = solve(rows, n, rng)
    if u is None:
        return None
    core = "".join(P1[j] if u[j] else P0[j] for j in range(n))
    h, st = O.nthash(core, k)
    h = [int(x) for x in h]
    ha, hb = h[0], h[d]
    if (ha >> KEY_SHIFT) != (hb >> KEY_SHIFT) or ha == hb:
        return None                           # the canonical strand was not the one solved for
    if any(x <= max(ha, hb) for x in h[1:d]):
        return None
    return core, ha, hb


GUARD_T = 3            # a minimizer pair must have guards for t = 1..GUARD_T free bases (tests/key_ties.py enumerates that many)
BAND_LO = 1 << 56      # ... and its larger hash at least this: small, but a flank can still undercut it


def has_guards(core, k, d, side):
    """tests/key_ties.py hides the larger element of the pair from every window that does not hold both: a GUARD, a k-mer with a
    smaller key t = W - d positions beyond the smaller element's far side (before the core when the right element is smaller, after
    it when the left one is), whose t free bases are the flank's next to the core.  For W - d = t <= GUARD_T such a k-mer must exist
    among the 4^t choices, with the k-mers between it and the pair above the pair (guard_ok) -- a property of the core, checked here"""
    h = [int(v) for v in O.nthash(core, k)[0]]
    key, top = h[0] >> KEY_SHIFT, max(h[0], h[d])
    for t in range(1, GUARD_T + 1):
        ok = False
        for c in range(4 ** t):
            x = "".join("ACGT"[(c >> (2 * j)) & 3] for j in range(t))
            if guard_ok(x + core[:k - 1] if side == "right" else core[d + 1:d + k] + x, k, key, top, side):
                ok = True
                break
        if not ok:
            return False
    return True


def guard_ok(g, k, key, top, side):
    """g: the t k-mers from the guard to the core (side 'right': guard first) or from the core to the guard ('left': guard last).
    The guard's key is below the pair's; the t - 1 k-mers between it and the pair are above both of the pair's hashes (they share
    windows with the pair).  (tests/key_ties.py holds the same rule)"""
    h = [int(v) for v in O.nthash(g, k)[0]]
    gi = 0 if side == "right" else len(h) - 1
    return h[gi] >> KEY_SHIFT < key and all(v > top for j, v in enumerate(h) if j != gi)


def search(f, r, k, d, rng, want, tries=30000, z_max=4, guards=False):
    """both orientations for (k, d): {'left': entry, 'right': entry}, trying fewer zero bits as a z runs out of tries.  guards:
    minimizer pairs, whose larger hash must lie in [BAND_LO, ...) and which must have guards (has_guards)"""
    got = {}
    # (unknowns k + d against 27 + z equations: fewer zero bits where there are few unknowns.  At most z_max: a pair that is small but
    # not tiny lets a random flank hold an element below the larger of the two, which hides it -- without one, a machine that picked
    # the wrong one of the pair would emit the same positions, only at other windows)
    z0 = max(0, min(z_max, k + d - 17))
    for z in list(range(z0, 0, -2)) + [0]:
        for _ in range(tries * (10 if z == 0 else 1)):  # (the last resort searches longer)
            a = attempt(f, r, k, d, z, rng)
            if a is None:
                continue
            core, ha, hb = a
            side = "left" if ha < hb else "right"
            if side in got:
                continue
            if guards and (max(ha, hb) < BAND_LO or not has_guards(core, k, d, side)):
                continue
            got[side] = dict(k=k, d=d, core=core, a=0, b=d, smaller=side, z=z, hash_a=str(ha), hash_b=str(hb))
            if len(got) == 2:
                return got
    return got


def smer_pairs(f, r, s, count):
    """the `count` pairs of different canonical s-mers with equal keys and the smallest such keys: [(x, y, hx, hy)], hx < hy"""
    n = 4 ** s
    codes = np.arange(n, dtype=np.uint64)
    F = np.array([f[c] for c in "ACGT"], np.uint64)
    R = np.array([r[c] for c in "ACGT"], np.uint64)
    fh = np.zeros(n, np.uint64)
    rh = np.zeros(n, np.uint64)
    for j in range(s):
        b = (codes >> np.uint64(2 * (s - 1 - j))) & np.uint64(3)
        for arr, tab, rot in ((fh, F, s - 1 - j), (rh, R, j)):
            v = tab[b]
            if rot % 64:
                v = (v << np.uint64(rot % 64)) | (v >> np.uint64(64 - rot % 64))
            arr ^= v
    h = np.minimum(fh, rh)
    keys = h >> np.uint64(KEY_SHIFT)
    o = np.argsort(h, kind="stable")
    hk, kk = h[o], keys[o]
    pairs, seen = [], set()
    for i in np.nonzero((kk[1:] == kk[:-1]) & (hk[1:] != hk[:-1]))[0]:
        hx, hy = int(hk[i]), int(hk[i + 1])
        if (hx, hy) in seen:
            continue
        seen.add((hx, hy))
        x = "".join("ACGT"[(int(o[i]) >> (2 * (s - 1 - j))) & 3] for j in range(s))
        y = "".join("ACGT"[(int(o[i + 1]) >> (2 * (s - 1 - j))) & 3] for j in range(s))
        assert int(O.nthash(x, s)[0][0]) == hx and int(O.nthash(y, s)[0][0]) == hy
        pairs.append((x, y, hx, hy))
        if len(pairs) == count:
            break
    return pairs


def far_pair(pairs, s, d, side, rng):
    """core = x + filler + y with the pair d >= s apart; the smaller one on `side`"""
    for t in range(1000):
        x, y, hx, hy = pairs[(2 * d + (side == "right") + t) % len(pairs)]
        if side == "right":
            x, y, hx, hy = y, x, hy, hx
        core = x + "".join(rng.choice("ACGT") for _ in range(d - s)) + y
        h = [int(v) for v in O.nthash(core, s)[0]]
        if h[0] == hx and h[d] == hy and all(v > max(hx, hy) for v in h[1:d]):
            return dict(k=s, d=d, core=core, a=0, b=d, smaller=side, z=64 - max(hx, hy).bit_length(), hash_a=str(hx), hash_b=str(hy))
    raise RuntimeError("no filler for s=%d d=%d" % (s, d))


def main(argv):
    out = argv[1] if len(argv) > 1 else OUT
    f, r = seeds()
    entries = {"minimizer": [], "syncmer": []}
    missing = []
    for fam, todo in (("minimizer", MIN_SET), ("syncmer", SYN_SET)):
        for k, d in todo:
            rng = random.Random(0x6B7E5 * 1000003 + 1009 * k + d + (0 if fam == "minimizer" else 7777))
            got = search(f, r, k, d, rng, 2, z_max=4 if fam == "minimizer" else 8, guards=fam == "minimizer")
            for side in ("left", "right"):
                if side in got:
                    entries[fam].append(got[side])
                else:
                    missing.append((fam, k, d, side))
            print(fam, k, d, sorted(got), file=sys.stderr)
    pairs = smer_pairs(f, r, SYN_S, 64)
    rng = random.Random(0x6B7E5 + SYN_S)
    for d in SYN_D:
        for side in ("left", "right"):
            entries["syncmer"].append(far_pair(pairs, SYN_S, d, side, rng))
    doc = {
        "about": "accidental 27-bit key ties (scripts/make_key_ties.py): core[a:a+k] and core[b:b+k] have equal canonical ntHash >> 37, "
                 "different 64-bit hashes, and hashes below every k-mer between them; k is the s of an s-mer for syncmer entries",
        "key_shift": KEY_SHIFT,
        "minimizer": entries["minimizer"],
        "syncmer": entries["syncmer"],
        "missing": [dict(family=a, k=b, d=c, smaller=e) for a, b, c, e in missing],
    }
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote %s: %d minimizer, %d syncmer entries, %d missing" % (out, len(entries["minimizer"]), len(entries["syncmer"]), len(missing)),
          file=sys.stderr)


if __name__ == "__main__":
    main(sys.argv)
