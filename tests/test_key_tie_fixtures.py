"""The crafted key-tie fixtures (tests/golden/key_ties.json) hold, and every read tests/test_gpu_key_ties.py builds from them has teeth.

The packed window machines compare hash >> 37 (27 bits) plus a slot number and trust that only where no two elements of a window share
the minimal key; every min operation checks for such a pair (kernels_pk.hpp header).  These tests keep the evidence for that check
honest without a GPU: each fixture is re-derived from oracle.nthash, and each GPU read is shown to select differently under a machine
that ignores the low 37 bits (leftmost-first or rightmost-first among equal keys) -- so a missing check fails the GPU test somewhere.
For the syncmer reads at tile seams the machine that ignores them is ONE TILE of a CPU model of the tiling rule
(KT.syncmer_positions_tiled, itself held against the oracle): every seam read has teeth in the tile its label names, and every
(d < W, orientation, tile before / after the seam) is covered.  The long-plan and ragged reads are held against the planner's rule for
their lengths (tests/plan_atlas.py), and the table of kernels the GPU cases must report against that rule at a tile's length.
"""
import random

import numpy as np
import pytest

from tests import key_ties as KT


def test_fixtures_are_accidental_key_ties(oracle):
    fx = KT.fixtures()
    assert fx["key_shift"] == KT.KEY_SHIFT
    for fam in ("minimizer", "syncmer"):
        for e in fx[fam]:
            k, d, core = e["k"], e["d"], e["core"]
            h = [int(v) for v in oracle.nthash(core, k)[0]]
            assert len(core) == k + d and e["a"] == 0 and e["b"] == d, e
            ha, hb = h[0], h[d]
            assert (str(ha), str(hb)) == (e["hash_a"], e["hash_b"]), e
            assert ha >> KT.KEY_SHIFT == hb >> KT.KEY_SHIFT and ha != hb, e        # a key tie, not a 64-bit tie
            assert e["smaller"] == ("left" if ha < hb else "right"), e
            assert all(v > max(ha, hb) for v in h[1:d]), e                         # below every element between them


def test_fixtures_cover_every_distance_in_both_orientations():
    have = {(fam, e["k"], e["d"], e["smaller"]) for fam in ("minimizer", "syncmer") for e in KT.fixtures()[fam]}
    for k in (21, 15, 31, 40):
        for d in range(1, 13):
            for side in ("left", "right"):
                assert ("minimizer", k, d, side) in have, (k, d, side)
    for d in range(1, 48):   # d < 2W for W up to 24
        for side in ("left", "right"):
            assert ("syncmer", KT.syn_s(d), d, side) in have, (d, side)


@pytest.mark.parametrize("k,w", [(21, 2), (21, 11), (15, 5), (40, 13), (5, 3)])
def test_closed_minimizer_equals_oracle(oracle, k, w):
    rng = random.Random(k * 31 + w)
    seqs = [KT.rand_seq(rng, rng.randint(k + w - 1, 400)) for _ in range(150)] + ["A" * 80, "AC" * 60]
    for q in seqs:
        h = oracle.nthash(q, k)[0]
        eh, ep, es, fl = oracle.minimizer(q, k, w, closed=True)
        assert np.array_equal(KT.minimizer_positions(h, w), ep), (k, w, q)


@pytest.mark.parametrize("k,s", [(15, 11), (35, 11), (28, 24), (48, 24), (31, 16)])
def test_closed_syncmer_equals_oracle(oracle, k, s):
    rng = random.Random(k * 37 + s)
    seqs = [KT.rand_seq(rng, rng.randint(2 * k - s - 1, 400)) for _ in range(150)] + ["A" * 120, "AC" * 70]
    for q in seqs:
        hs = oracle.nthash(q, s)[0]
        eh, ep, es, fl = oracle.syncmer(q, k, s, closed=True)
        assert np.array_equal(KT.syncmer_positions(hs, k, s, len(q)), ep), (k, s, q)


def _check_teeth(oracle, t, kind):
    """the read's true selection is the oracle's, and a key-only machine (either tie-break) selects differently"""
    q = t.seq
    if kind == "minimizer":
        h = oracle.nthash(q, t.k)[0]
        ep = oracle.minimizer(q, t.k, t.w, closed=True)[1]
        mp = oracle.minimizer(q, t.k, t.w)[1]
        assert np.array_equal(KT.minimizer_positions(h, t.w), ep) and np.array_equal(mp, ep)
        assert any(not np.array_equal(ep, KT.minimizer_positions(h, t.w, r)) for r in ("left", "right")), (t.w, t.d, t.a, t.side)
    else:
        hs = oracle.nthash(q, t.s)[0]
        ep = oracle.syncmer(q, t.k, t.s, closed=True)[1]
        mp = oracle.syncmer(q, t.k, t.s)[1]
        assert np.array_equal(KT.syncmer_positions(hs, t.k, t.s, len(q)), ep) and np.array_equal(mp, ep)
        assert any(not np.array_equal(ep, KT.syncmer_positions(hs, t.k, t.s, len(q), r)) for r in ("left", "right")), (t.w, t.d, t.a)


@pytest.mark.parametrize("name", sorted(KT.MIN_SETS))
def test_every_minimizer_tie_read_has_teeth(oracle, name):
    """k = 21: EVERY layout (d < W, start residue, orientation, placement) is built -- the guard makes the teeth -- and the last
    (ragged) block is met at every nk mod W"""
    for w in KT.MIN_SETS[name][0]:
        reads, lost = KT.min_set_reads(oracle, name, w)
        assert lost == 0 and len(reads) == 2 * w * (w - 1) * len(KT.MIN_SETS[name][2]), (name, w, lost, len(reads))
        ends = {(t.place, (len(t.seq) - KT.MIN_K + 1) % w) for t in reads}
        for place in KT.MIN_SETS[name][2]:
            if place == "last":   # the ragged last block at every nk mod W
                assert {e for p, e in ends if p == place} == set(range(w)), (name, w)
        for t in reads:
            _check_teeth(oracle, t, "minimizer")


def test_every_other_k_tie_read_has_teeth(oracle):
    for k, ws in KT.MIN_OTHER_K:
        for w in ws:
            reads, _ = KT.min_set_reads(oracle, "short", w, k=k)
            assert not KT.missing_classes(reads, w), (k, w, KT.missing_classes(reads, w))
            for t in reads:
                _check_teeth(oracle, t, "minimizer")


def test_every_syncmer_tie_read_has_teeth(oracle):
    """syncmer reads have no guards: every (d, side) with d < W keeps reads; of the pairs W..2W-1 apart (they meet only where a 2W
    window's two halves are combined) some do, at every W"""
    for w in range(4, 25):
        by_s, _ = KT.syn_reads(oracle, w)
        reads = [t for v in by_s.values() for t in v]
        assert not KT.missing_classes(reads, w), (w, KT.missing_classes(reads, w))
        assert any(t.d >= w for t in reads), w
        for t in reads:
            _check_teeth(oracle, t, "syncmer")


# ---- syncmer ties at tile seams, on the long staged plan and at ragged ends (KT.SYN_CELLS2) --------------------------------------------
@pytest.mark.parametrize("k,s", [(15, 11), (35, 11), (28, 24), (48, 24), (31, 16)])
def test_tiled_syncmer_model_equals_oracle(oracle, k, s):
    """the tiling rule of kernels_tile.hpp's header, with the exact selection in every tile, is the closed form and the state machine"""
    rng = random.Random(k * 41 + s)
    seqs = [KT.rand_seq(rng, rng.randint(2 * k - s - 1, 400)) for _ in range(150)] + ["A" * 120, "AC" * 70]
    for q in seqs:
        hs = oracle.nthash(q, s)[0]
        ep = oracle.syncmer(q, k, s, closed=True)[1]
        assert np.array_equal(oracle.syncmer(q, k, s)[1], ep), (k, s, q)
        for tp in (16, 64, 224):
            assert np.array_equal(KT.syncmer_positions_tiled(hs, k, s, len(q), tp), ep), (k, s, tp, q)


PA_TILE_MIN = KT.PA.SYN_TILE_MIN   # PlannerTable::syn_tile_min_bases


def _seam_cells():
    return [(c[0], int(c[1]["BSK_TILE_POS"])) for c in KT.SYN_CELLS2 if "BSK_TILE_POS" in c[1]]


@pytest.mark.parametrize("cell,tp", _seam_cells())
def test_every_seam_read_has_teeth_in_its_tile(oracle, cell, tp):
    """a seam read labelled 'before' / 'after' changes the stitched positions when tile m - 1 / m ALONE selects by key (shown on the tiled
    model, tile by tile), and not when its label does not claim it; every (d < W, orientation, label) is covered at every W of the cell"""
    assert KT.SEAM_LEFT_OUT == {}
    ws = {w for c in KT.SYN_CELLS2 if c[0] == cell for w in c[3] + c[4]}
    assert ws == set(KT.SYN_TILE_WS) and {4, 8, 13, 20, 21, 24} <= ws
    for w in sorted(ws):
        by_s, lost = KT.syn_cell_reads(oracle, cell, w)
        reads = [t for v in by_s.values() for t in v]
        assert lost == [] and KT.missing_seam_classes(reads, w) == [], (cell, w, lost)
        for t in reads:
            q, n = t.seq, len(t.seq)
            assert n == KT.syn_seam_bases(t.k, tp) and t.tp == tp and 0 <= t.m * tp - t.a <= w + t.d and t.labels, (cell, w, t.d, t.a)
            assert q[t.a:t.a + t.s + t.d] == KT.fixture("syncmer", t.s, t.d, t.side)["core"]
            hs = oracle.nthash(q, t.s)[0]
            ep = oracle.syncmer(q, t.k, t.s, closed=True)[1]
            assert t.m * tp < len(hs) - 2 * w + 1                                    # the seam lies inside the read: tile m exists
            assert np.array_equal(oracle.syncmer(q, t.k, t.s)[1], ep) and np.array_equal(KT.syncmer_positions_tiled(hs, t.k, t.s, n, tp), ep)
            for j, lab in ((t.m - 1, "before"), (t.m, "after")):
                bites = any(not np.array_equal(ep, KT.syncmer_positions_tiled(hs, t.k, t.s, n, tp, lambda i, j=j, r=r: r if i == j else "exact"))
                            for r in ("left", "right"))
                assert bites == (lab in t.labels), (cell, w, t.d, t.side, t.a, t.m, lab)


def test_seam_cell_plans_follow_the_planner_rule():
    """KT.SYN_PLANS for the forced tiles = make_plan_enc's rules (plan_atlas: syn_pk_fits, syn_pf_fits) at a tile's length bound
    tp + 3k - 2s + 12 (tiles.hip), the same for both s of a W; the cells name a kernel for every W they run, and SYN_REACH is their union"""
    PA = KT.PA

    def planned(k, s, ln, fused):
        for ok, lng, name in ((fused and PA.syn_pf_fits(k, s, ln, False), 0, "pf"), (fused and PA.syn_pf_fits(k, s, ln, True), 1, "pfl"),
                              (PA.syn_pk_fits(k, s, ln, False), 0, "pk"), (PA.syn_pk_fits(k, s, ln, True), 1, "pkl")):
            if ok:
                return name
        return "fast"
    for cell, tp in _seam_cells():
        for mode in ("pf", "pk"):
            for w in KT.SYN_TILE_WS:
                for s in (24, 11):
                    k = s + w
                    ln = min(tp + 3 * k - 2 * s + 12, KT.syn_seam_bases(k, tp))
                    assert KT.SYN_PLANS[cell, mode][w] == "k_syncmer_%s<%d>" % (planned(k, s, ln, mode == "pf"), w), (cell, mode, w, s)
    reach = set()
    for cell, mode, w in KT.SYN_CASES2:
        name = KT.SYN_PLANS[cell, mode][w]
        if not name.startswith("k_syncmer_fast"):
            reach.add((name.split("<")[0], w))
    assert reach == KT.SYN_REACH
    packed = {("k_syncmer_pk", w) for w in range(4, 21)} | {("k_syncmer_pkl", w) for w in range(4, 25)}
    packed |= {("k_syncmer_pf", w) for w in range(8, 21)} | {("k_syncmer_pfl", w) for w in range(8, 25)}   # (pk / pf_syncmer_supported)
    assert KT.SYN_REACH | set(KT.SYN_NOT_REACHED) == packed and not KT.SYN_REACH & set(KT.SYN_NOT_REACHED)
    assert KT.SYN_NOT_REACHED == {}


def test_every_default_tile_read_has_teeth(oracle):
    """sequences the default planner tiles (449 .. 1 500 bases), the pair across a multiple of 16: read-level teeth, every d < W both ways"""
    for w in range(4, 25):
        by_s, _ = KT.syn_cell_reads(oracle, "syn_tiles_default", w)
        reads = [t for v in by_s.values() for t in v]
        assert not KT.missing_classes(reads, w), (w, KT.missing_classes(reads, w))
        assert any(t.d >= w for t in reads), w
        for t in reads:
            assert KT.DEFAULT_TILE_BASES[0] <= len(t.seq) <= KT.DEFAULT_TILE_BASES[1] and PA_TILE_MIN < len(t.seq)
            assert t.a // 16 < (t.a + t.d) // 16, (w, t.d, t.a)
            _check_teeth(oracle, t, "syncmer")


def test_every_long_plan_tie_read_has_teeth(oracle):
    """W <= 20 at lengths the planner gives to k_syncmer_pkl<W>: too many rows for the short column, few enough for the long one, both
    for the longest read of the batch; every (d, side), some d >= W, and the last block at every ns mod W"""
    for w in range(4, 21):
        by_s, _ = KT.syn_cell_reads(oracle, "syn_long", w)
        reads = [t for v in by_s.values() for t in v]
        assert not KT.missing_classes(reads, w), (w, KT.missing_classes(reads, w))
        assert any(t.d >= w for t in reads), w
        assert {t.place for t in reads} == {"first", "interior", "last"}, w
        assert {(len(t.seq) - t.s + 1) % w for t in reads if t.place == "last"} == set(range(w)), w
        for s, v in by_s.items():
            lo, hi = KT.syn_long_range(w, s)
            top = max(len(t.seq) for t in v)
            assert not KT.PA.syn_pk_fits(s + w, s, lo, False) and KT.PA.syn_pk_fits(s + w, s, lo - 1, False) and KT.PA.syn_pk_fits(s + w, s, hi, True)
            assert all(lo <= len(t.seq) <= hi for t in v) and hi <= PA_TILE_MIN, (w, s, lo, hi)
            assert not KT.PA.syn_pk_fits(s + w, s, top, False) and KT.PA.syn_pk_fits(s + w, s, top, True), (w, s, top)
        for t in reads:
            _check_teeth(oracle, t, "syncmer")


def test_every_ragged_tie_read_has_teeth(oracle):
    """the pair within the last 2W s-mers of its read, the neighbours 3W .. 6W bases longer and still on the short plan; every (d, side),
    and every ns mod W in both orientations"""
    for w in range(4, 21):
        by_s, lost = KT.syn_cell_reads(oracle, "syn_ragged", w)
        reads = [t for v in by_s.values() for t in v]
        assert lost == 0 and not KT.missing_classes(reads, w), (w, lost, KT.missing_classes(reads, w))
        for side in ("left", "right"):
            assert {(len(t.seq) - t.s + 1) % w for t in reads if t.side == side} == set(range(w)), (w, side)
        for t in reads:
            ns = len(t.seq) - t.s + 1
            assert t.d < w and ns - 2 * w <= t.a and t.a + t.d <= ns - 1, (w, t.d, t.a, ns)
            lo, hi = KT.ragged_neighbour_range(t)
            assert lo == len(t.seq) + 3 * w and lo <= hi and KT.PA.syn_pk_fits(t.k, t.s, hi, False), (w, t.d, lo, hi)
            assert w < 8 or KT.PA.syn_pf_fits(t.k, t.s, hi, False), (w, t.d, hi)
            _check_teeth(oracle, t, "syncmer")
        for s, v in by_s.items():
            for part in KT.chunks(v, KT.BATCH_TIES):
                seqs, at = KT.with_ragged_neighbours(part, 1)
                assert len(seqs) < 1024 and [seqs[i] for i in at] == [t.seq for t in part]
                assert all(min(len(seqs[i + 1]), len(seqs[i + 2])) >= len(seqs[i]) + 3 * w for i in at), (w, s)
