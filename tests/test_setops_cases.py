"""CPU: every claim tests/setops_cases.py makes about its crafted inputs, re-derived from the sets alone -- a pair's t against the caps
read from setops.hip, the merged ranks of a shared value's two copies against the tile boundaries, which members of a group hold a
value -- and the reference itself on inputs whose answer is known by construction."""
import numpy as np
import pytest

from tests import setops_cases as SC

U64 = np.uint64
CAPS = SC.read_caps()
GROUP_CAP, WAVE_CAP, TILE = CAPS["SO_GROUP_CAP"], CAPS["SO_WAVE_CAP"], CAPS["SO_TILE"]


def strictly_ascending(x):
    return x.dtype == U64 and bool(np.all(x[1:] > x[:-1]))


def test_caps_read_from_the_source():
    assert 16 <= GROUP_CAP < WAVE_CAP and TILE == WAVE_CAP
    assert WAVE_CAP * 8 <= 8192  # one wavefront's LDS share: both sets of a pair, 8 bytes a value
    for k in ("SO_GROUP_BLOCKS_PER_CU", "SO_WAVE_BLOCKS_PER_CU", "SO_TILE_BLOCKS_PER_CU", "SO_WAVES"):
        assert CAPS[k] >= 1, k


def test_reference_on_known_answers():
    a, b = np.array([1, 3, 5, 7], U64), np.array([3, 4, 7, 9], U64)
    want = {SC.UNION: [1, 3, 4, 5, 7, 9], SC.INTERSECT: [3, 7], SC.DIFF: [1, 5], SC.SYMDIFF: [1, 4, 5, 9]}
    for op, w in want.items():
        o, v = SC.ref_op(SC.collection([a, a]), SC.collection([b]), op)  # broadcast
        assert o.tolist() == [0, len(w), 2 * len(w)] and v.tolist() == w * 2 and v.dtype == U64
    s = SC.collection([a, b, np.array([7], U64)])
    go = np.array([0, 0, 3, 3], U64)
    assert [x.tolist() for x in SC.split(*SC.ref_reduce(s, go, 1))] == [[], [1, 3, 4, 5, 7, 9], []]
    assert [x.tolist() for x in SC.split(*SC.ref_reduce(s, go, 2))] == [[], [3, 7], []]
    assert [x.tolist() for x in SC.split(*SC.ref_reduce(s, go, SC.MEMBERS_ALL))] == [[], [7], []]
    assert [x.tolist() for x in SC.split(*SC.ref_reduce(s, go, 4))] == [[], [], []]


def test_degenerate_pairs_are_what_their_names_say():
    d = SC.degenerate_pairs()
    for name, (a, b) in d.items():
        assert strictly_ascending(a) and strictly_ascending(b), name
    assert len(d["both empty"][0]) == 0 and len(d["both empty"][1]) == 0
    assert len(d["a empty"][0]) == 0 and len(d["a empty"][1]) > 0 and len(d["b empty"][1]) == 0 and len(d["b empty"][0]) > 0
    assert np.array_equal(*d["identical"])
    a, b = d["disjoint interleaved"]
    v, from_a = SC.merged(a, b)
    assert len(np.intersect1d(a, b)) == 0 and np.all(from_a[::2]) and not np.any(from_a[1::2])
    assert d["a below b"][0].max() < d["a below b"][1].min() and d["b below a"][1].max() < d["b below a"][0].min()
    a, b = d["extremes on both sides"]
    assert a[0] == 0 and b[0] == 0 and a[-1] == SC.MAX64 and b[-1] == SC.MAX64
    a, b = d["extremes split"]
    assert a[0] == 0 and b[-1] == SC.MAX64 and a[-1] == b[0]
    assert max(len(a) + len(b) for a, b in d.values()) <= GROUP_CAP  # all of them on the group path


@pytest.mark.parametrize("cap", [GROUP_CAP, WAVE_CAP])
def test_class_edges(cap):
    edges = SC.class_edges(cap, np.random.default_rng(5))
    assert sorted({t for _, _, t, _ in edges}) == [cap - 1, cap, cap + 1]
    for a, b, t, na in edges:
        assert strictly_ascending(a) and strictly_ascending(b)
        assert len(a) == na and len(a) + len(b) == t
        assert len(np.intersect1d(a, b)) == min(na, t - na) // 2
        want = [1, 0, 0] if t <= GROUP_CAP else [0, 1, 0] if t <= WAVE_CAP else [0, 0, 1]
        assert SC.path_counts(*[SC.collection([x])[0] for x in (a, b)], CAPS) == want
    for t in (cap - 1, cap, cap + 1):
        assert sorted(na for _, _, tt, na in edges if tt == t) == sorted([0, 1, t // 2, t - 1])


def test_tile_cases_put_the_copies_where_they_claim():
    t = 3 * TILE + 5
    cases = SC.tile_cases(TILE, np.random.default_rng(9))
    for name, (a, b, at) in cases.items():
        assert strictly_ascending(a) and strictly_ascending(b), name
        assert len(a) + len(b) == t, name
        v, from_a = SC.merged(a, b)
        dup = np.flatnonzero(v[1:] == v[:-1])  # rank of the first copy of every shared value
        assert dup.tolist() == sorted(at), name
        assert np.all(from_a[dup]) and not np.any(from_a[dup + 1]), name  # a's copy first
        assert len(np.intersect1d(a, b)) == len(at), name
    at = cases["straddles the boundary after tile 0"][2]
    assert at == [TILE - 1] and (at[0] // TILE, (at[0] + 1) // TILE) == (0, 1)  # merged ranks 1 023 and 1 024 at the recommended tile
    at = cases["straddles the boundary after tile 1"][2]
    assert (at[0] // TILE, (at[0] + 1) // TILE) == (1, 2)
    assert [(r // TILE, (r + 1) // TILE) for r in cases["straddles both boundaries"][2]] == [(0, 1), (1, 2)]
    r = cases["last ranks of tile 0, not straddling"][2][0]
    assert (r + 1) % TILE == TILE - 1 and r // TILE == (r + 1) // TILE == 0
    r = cases["first ranks of tile 1"][2][0]
    assert r % TILE == 0 and r // TILE == (r + 1) // TILE == 1
    at = cases["every value shared but the first (every boundary straddled)"][2]
    a, b, _ = cases["every value shared but the first (every boundary straddled)"]
    more, less = (a, b) if len(a) > len(b) else (b, a)  # the first rank's value is in one of them only
    assert len(more) == len(less) + 1 and np.array_equal(more[1:], less)
    assert {TILE - 1, 2 * TILE - 1, 3 * TILE - 1} <= set(at)
    a, b, at = cases["no value shared"]
    assert at == [] and len(np.intersect1d(a, b)) == 0
    assert (t + TILE - 1) // TILE == 4  # three full tiles and one of five ranks


def test_shifted_pairs_and_their_reference():
    rng = np.random.default_rng(3)
    n = 600
    a, b, base, shift = SC.shifted_pairs(n, 0, 40, rng, n_base=37)
    assert len(a[0]) == n + 1 and len(b[0]) == n + 1
    sa, sb = SC.split(*a), SC.split(*b)
    for p in (0, 1, 36, 37, 38, 599):
        assert np.array_equal(sa[p], base[p % 37][0] + shift[p]) and np.array_equal(sb[p], base[p % 37][1] + shift[p])
        assert strictly_ascending(sa[p]) and strictly_ascending(sb[p])
    t = SC.pair_t(a[0], b[0])
    assert t.min() >= 0 and t.max() <= 40
    assert max(int(x.max()) if len(x) else 0 for x, _ in base) < 1 << 40 and int(shift[1]) == 1 << 41
    for op in SC.OPS:  # the shift commutes with the op: the short cut equals NumPy pair by pair
        o, v = SC.ref_shifted(base, shift, op)
        o2, v2 = SC.ref_op(a, b, op)
        assert np.array_equal(o, o2) and np.array_equal(v, v2)


def test_reduce_groups_hold_what_they_claim():
    (offs, vals), go = SC.reduce_groups(np.random.default_rng(7))
    sets = SC.split(offs, vals)
    assert go[0] == 0 and go[-1] == len(sets) and np.all(np.diff(go.astype(np.int64)) >= 0)
    sizes = np.diff(go.astype(np.int64)).tolist()
    assert sizes == [0, 1, 2, 0, 64, 3, 2, 2, 0]
    for s in sets:
        assert strictly_ascending(s) or len(s) <= 1
    g1, g2 = sets[int(go[1]):int(go[2])], sets[int(go[2]):int(go[3])]
    assert g1[0][-1] == g2[0][0] == 1000 and 1000 not in g2[1].tolist()  # the run of 1000 reaches two only across the border
    big = sets[int(go[4]):int(go[5])]
    held = {x: sum(int(x in s.tolist()) for s in big) for x in (7, 8, 9, 10)}
    assert held == {7: 64, 8: 63, 9: 2, 10: 1}
    g5 = sets[int(go[5]):int(go[6])]
    assert [len(s) for s in g5] == [2, 0, 2]
    assert all(len(s) == 0 for s in sets[int(go[6]):int(go[7])])
    # and the reference draws the lines there
    for m, want in ((1, [7, 8, 9, 10]), (2, [7, 8, 9]), (3, [7, 8]), (63, [7, 8]), (64, [7]), (SC.MEMBERS_ALL, [7])):
        got = SC.split(*SC.ref_reduce((offs, vals), go, m))[4]
        assert [x for x in got.tolist() if x < 100] == want, m
    r1, r2, rall = (SC.split(*SC.ref_reduce((offs, vals), go, m)) for m in (1, 2, SC.MEMBERS_ALL))
    assert r1[1].tolist() == [1, 5, 1000] and r1[2].tolist() == [1000, 1500, 2000]
    assert r2[1].tolist() == [] and r2[2].tolist() == [2000]  # 1000 is NOT counted across the border
    assert rall[1].tolist() == [1, 5, 1000] and rall[5].tolist() == [] and r2[5].tolist() == [4] and rall[7].tolist() == [0, SC.MAX64]
