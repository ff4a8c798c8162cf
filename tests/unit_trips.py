"""The cases of tests/test_gpu_unit_trips.py: every planned sketch kernel's unit loop through several tickets a wave (BSK_UNIT_GRID;
DESIGN.md "Switches" and section 7), and the list of reads a packed kernel leaves to the exact machine at the edge of its segment.
tests/test_unit_trips.py holds all of it against the sources -- no GPU.

THE TRIP SHAPE.  A planned sketch kernel is a grid of persistent waves that pull tickets of `own` units of 64 reads (launch.hip:
4 for k_minimizer_pkd / _dense / k_prot_minimizer_fast, 8 for the others that take KArgs::tk; the stream kernels' fixed 8 or 4, one unit for
the general kernels), and launch.hip shrinks the ticket to one per wave while nunits < waves x own.  On 256 CUs that is every batch of the
other suites.  BSK_UNIT_GRID=G gives the launch min(G, its own grid) waves; the rows here hold N_TRIP = 82 x 64 + 37 reads -- 83 units,
the last one partial; 83 = 10 x 8 + 3 = 20 x 4 + 3: the last ticket is partial for both sizes; 83 >= G x own for G in CAPS, so `tk` stays
the kernel's own -- which are 11 or 21 tickets for one or three waves: some wave takes four or more.

ROWS.  Copies of plan-atlas rows (tests/plan_atlas.py: same seeded generator, every tenth read low-complexity) with n = N_TRIP, picked by
`selected`: of every kernel family (the plan name before '<') and combination of its non-numeric template arguments the rows with the
smallest and the largest leading numeric argument (k_nthash_fast's argument is a mode: every mode); not the fallback rows, and not the rows over tiles or length-binned units, whose shapes have
cases of their own below.  A batch of 1 024 ragged reads or more is length-binned by itself (bin_gran_for, planner.hip): the rows keep the
atlas's plan names with BSK_NO_BIN.

THE FULL SEGMENT.  list_append (kernels_generic.hpp) gives every workgroup one segment of syn_pk_fixcap(n, grid) / grid entries and
raises a flag at the first entry beyond it; the host then runs the batch on the 64-bit kernel.  EDGES: batches of nothing but exact-tie
reads (homopolymers and short-period repeats: equal hashes inside every window, so every read is listed and the count is known), at one
workgroup exactly the segment (the packed kernel's name stays) and one read more (the call ends on k_minimizer_fast / k_syncmer_fast), and
at three workgroups three segments and one read (some segment takes one too many, whoever draws which ticket).
"""
from __future__ import annotations

import copy
import os
import random
import re

from tests import plan_atlas as A

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bio_amd", "csrc")
N_TRIP = 82 * 64 + 37
UNITS = (N_TRIP + 63) // 64
CAPS = (1, 3)
NO_BIN = {"BSK_NO_BIN": "1"}

# plan-name family -> (the planner's name for it: Which in host_internal.hpp, where its own ticket size stands, the text that says it, units)
FAMILIES = {
    "k_minimizer_pk": ("K_MIN_PK", "kernels_pk.hpp", "#define PK_TICKET 8u", 8),
    "k_minimizer_ring": ("K_MIN_RING", "kernels_ring.hpp", "#define RG_TICKET 8u", 8),
    "k_minimizer_pkd": ("K_MIN_PKD", "kernels_pkd.hpp", "const u32 tku = a.tk ? a.tk : 4u;", 4),
    "k_minimizer_dense": ("K_MIN_DENSE", "kernels_fast.hpp", "const u32 TK = ASC ? 1u : (a.tk ? a.tk : 4u);", 4),
    "k_minimizer_fast": ("K_MIN_FAST", "kernels_fast.hpp", "const u32 tku = a.tk ? a.tk : 8u;", 8),
    "k_syncmer_pk": ("K_SYN_PK", "kernels_syncmer_pk.hpp", "const u32 tku = a.tk ? a.tk : 8u;", 8),
    "k_syncmer_pkl": ("K_SYN_PK", "kernels_syncmer_pk.hpp", "const u32 tku = a.tk ? a.tk : 8u;", 8),
    "k_syncmer_pf": ("K_SYN_PK", "kernels_syncmer_pf.hpp", "const u32 tku = a.tk ? a.tk : 8u;", 8),
    "k_syncmer_pfl": ("K_SYN_PK", "kernels_syncmer_pf.hpp", "const u32 tku = a.tk ? a.tk : 8u;", 8),
    "k_syncmer_fast": ("K_SYN_FAST", "kernels_syncmer.hpp", "const u32 TK = ASC ? 1u : (a.tk ? a.tk : 8u);", 8),
    "k_prot_minimizer_fast": ("K_PROT_MIN_FAST", "kernels_protein.hpp", "const u32 tku = a.tk ? a.tk : 4u;", 4),
    "k_prot_hash_fast": ("K_PROT_HASH_FAST", "kernels_protein.hpp", "const u32 u0 = next_ticket(a.ticket, lane) * 4u;", 4),
    "k_nthash_fast": ("K_NT_FAST", "kernels_fast.hpp", "const u32 u0 = next_ticket(a.ticket, lane) * 8u;", 8),
    "k_simhash_fast": ("K_SIM_FAST", "kernels_simhash.hpp", "const u32 u0 = next_ticket(a.ticket, lane) * 8u;", 8),
    # the general per-lane kernels: a ticket is one unit
    "k_minimizer_generic": ("K_MIN_GEN_P", "kernels_generic.hpp", "const u32 unit = next_ticket(a.ticket, lane);", 1),
    "k_nthash_stream": ("K_NT_P", "kernels_generic.hpp", "const u32 unit = next_ticket(a.ticket, lane);", 1),
    "k_syncmer": ("K_SYN_P", "kernels_more.hpp", "const u32 unit = next_ticket(a.ticket, lane);", 1),
    "k_kmer": ("K_KMER_P", "kernels_more.hpp", "const u32 unit = next_ticket(a.ticket, lane);", 1),
    "k_simhash": ("K_SIM_P", "kernels_more.hpp", "const u32 unit = next_ticket(a.ticket, lane);", 1),
    "k_prot_hash": ("K_PROT_HASH", "kernels_more.hpp", "const u32 unit = next_ticket(a.ticket, lane);", 1),
    "k_prot_minimizer": ("K_PROT_MIN", "kernels_more.hpp", "const u32 unit = next_ticket(a.ticket, lane);", 1),
}
# the kernels that take their units from eight ticket heads and look back over them: BSK_UNIT_GRID must not reach their launches
HEAD_TICKET_KERNELS = ("k_translate", "k_compact_flags", "k_tile_stitch", "k_minimizer_pft")


def source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def family(name):
    return name.split("<")[0]


def template_args(name):
    return name.split("<", 1)[1].rstrip(">,").split(",") if "<" in name else []


MODE_FAMILIES = ("k_nthash_fast",)  # the template argument is a MODE (ntHash one strand / canonical, k-mer codes canonical / two strands / forward), not a size: every mode is a group


def group_of(row):
    """(family, its non-numeric template arguments), and the leading numeric argument (None: the name has none)"""
    args = template_args(row.name)
    if family(row.name) in MODE_FAMILIES:
        return (family(row.name), tuple(args)), None
    nums = [int(a) for a in args if a.isdigit()]
    return (family(row.name), tuple(a for a in args if not a.isdigit())), (nums[0] if nums else None)


def eligible(row):
    return "fallback" not in row.id and A.TILES not in row.suffixes and A.BINNED not in row.suffixes


def selected(rows=None):
    """the atlas rows the trip shape runs: per group the rows with the smallest and the largest leading numeric argument, in atlas order"""
    rows = [r for r in (A.ROWS if rows is None else rows) if eligible(r)]
    ends = {}
    for r in rows:
        g, num = group_of(r)
        if num is not None:
            lo, hi = ends.get(g, (num, num))
            ends[g] = (min(lo, num), max(hi, num))
    return [r for r in rows if group_of(r)[1] is None or group_of(r)[1] in ends[group_of(r)[0]]]


TIE_EXTRA = 150  # homopolymers appended to the rows below
# Rows of the kernels that list reads where the atlas's low-complexity reads (period 1-6 over a random share of the read) tie inside a
# window in only 50-150 of the 528: windows of two k-mers, or of eight s-mers of a hundred bases -- too few for 65 in one of three segments
TIE_ROWS = ("min_pk<2,false>", "min_pk<2,true>", "min_ring<2,false>", "min_ring<2,true>", "min_pkd<2>", "syn_pk_224<4>", "syn_pk_225<4>", "syn_pkl_480<4>")


def lists_reads(name):
    """the planned kernel leaves reads to the exact machine through list_append (launch.hip: `lists`)"""
    return FAMILIES[family(name)][0] in ("K_MIN_PK", "K_MIN_RING", "K_MIN_PKD", "K_SYN_PK")


# Rows whose atlas lengths make k_minimizer_pk list MOST reads at 83 units -- a pair of reads shares a staging column of BSK_PK_ROWS = 58
# rows, and both go to the list when their tuples fill it: at w = 2 (two tuples in three windows) every pair of 100-base reads does, at
# w = 13 the pairs of 260-base reads -- so that the call abandons the kernel (160 reads never fill a segment; 5 285 do).  Shorter plain
# reads; the `limits` reads, which decide the kernel's LONG argument, stay.
TRIP_LENS = {"min_pk<2,false>": (36, 44, 52), "min_pk<2,true>": (36, 44, 52), "min_pk<13,true>": (150, 200)}


def trip_row(row):
    """the atlas row with N_TRIP reads in all (its `extra` reads included).  The TIE_ROWS end in TIE_EXTRA homopolymers of the row's
    lengths: a homopolymer ties in every window there is."""
    t = copy.copy(row)
    t.lens = TRIP_LENS.get(row.id, row.lens)
    if row.id in TIE_ROWS:
        lens = sorted(t.lens)
        t.extra = tuple(row.extra) + tuple("ACGT"[j % 4] * (lens[j % len(lens)] - (j // 4) % 8) for j in range(TIE_EXTRA))
    t.n = N_TRIP - len(t.extra)
    t.env = dict(row.env, **NO_BIN)
    return t


ROWS = [trip_row(r) for r in selected()]
BY_ID = {r.id: r for r in ROWS}


# ---- launch.hip's ticket rule and planner.hip's list segments, as the sources state them ----
def launch_rules():
    """-> dict(own4: the planner's kernels whose own ticket is 4 units (the others': 8), shrink: the kernels whose ticket launch.hip
    shrinks, lists: the kernels with a list of reads).  Raises AssertionError when launch.hip / planner.hip no longer say it this way."""
    src = source("launch.hip")
    m = re.search(r"const u32 own = \(([^;]*?)\) \? 4u : 8u;\s*const u64 waves = \(u64\)std::max\(pl\.grid, 1\);\s*a\.tk = 0;\s*if \(\(([^;]*?)\) && \(u64\)pl\.nunits < waves \* own\)\s*"
                  r"a\.tk = \(u32\)std::max<u64>\(1, \(\(u64\)pl\.nunits \+ waves - 1\) / waves\);", src)
    assert m, "launch.hip: the units-per-ticket rule (own, waves, tk) is not where tests/unit_trips.py reads it"
    names = lambda text: set(re.findall(r"pl\.which == (K_\w+)", text))
    tail = re.search(r"if \(pl\.which == K_MIN_PK && !a\.tk && ctx->opt\.pk_tail\) \{[^}]*?const u64 region = std::min<u64>\(\(u64\)ctx->opt\.pk_tail \* waves \* own, pl\.nunits\);\s*"
                     r"a\.tk_t0 = \(u32\)\(\(\(u64\)pl\.nunits - region\) / own\);\s*a\.tk_small = ctx->opt\.pk_small;", src)
    assert tail, "launch.hip: k_minimizer_pk's tail rule (tk_t0, tk_small) is not where tests/unit_trips.py reads it"
    lists = re.search(r"const bool lists = ([^;]*);\s*const u64 fixcap = lists \? syn_pk_fixcap\(b->n, pl\.grid\) : 0;", src)
    assert lists, "launch.hip: the list of reads (lists, fixcap) is not where tests/unit_trips.py reads it"
    assert "a.list_grid = (u32)pl.grid;" in src and "a.fixcap = (u32)fixcap;" in src
    fix = "u64 syn_pk_fixcap(u64 n, int grid) { return std::max<u64>((u64)grid * 1024, (n / 4 + (u64)grid) / (u64)grid * (u64)grid); }"
    assert fix in source("planner.hip"), "planner.hip: syn_pk_fixcap is not the expression tests/unit_trips.py restates"
    gen = source("kernels_generic.hpp")
    assert "if (at < seg) list[a.list_grid + blockIdx.x * seg + at] = (u32)r;" in gen and "else atomicOr(&a.ticket[1], 2u);" in gen
    bio = source("biosketch.hip")
    assert 'pk_tail = env_u32("BSK_PK_TAIL", 1);' in bio and 'pk_small = std::min(std::max(env_u32("BSK_PK_SMALL", 3), 3u), 8u);' in bio
    return dict(own4=names(m.group(1)), shrink=names(m.group(2)), lists=names(lists.group(1)), pk_tail=1, pk_small=3)


def listed_bounds(oracle, row, seqs, consts):
    """-> (must, may): the reads of a batch in batch order (no length bins) the planned kernel of `row` must list -- an exact hash tie inside
    a window -- and an upper bound of what it lists, by the kernel's own rule for reads it cannot finish (consts: read off the headers by
    tests/test_unit_trips.py).  k_minimizer_pk / k_syncmer_pk / _pkl: lanes l and l ^ 32 of a unit share a column of PR rows, both are listed
    when their tuples reach it; k_syncmer_pf / _pfl: the lanes of a unit beyond TCAP tuples; k_minimizer_pkd: a read beyond its slab;
    k_minimizer_ring: a read beyond the unit's rows, and the lanes that outrun the ring -- up to 4 % of the reads (launch.hip's figure)."""
    from tests.test_plan_atlas import _has_equal_pair_in_a_window, _oracle_call
    fam, p = family(row.name), row.p
    tied, cnt = [], []
    for q in seqs:
        tied.append(_has_equal_pair_in_a_window(oracle, row, q))
        try:
            cnt.append(len(_oracle_call(oracle, row, q)[0]))
        except oracle.OracleError:
            cnt.append(0)
    n = len(seqs)
    listed = list(tied)
    longest = max(len(q) for q in seqs)
    if fam in ("k_minimizer_pk", "k_syncmer_pk", "k_syncmer_pkl"):
        pr = consts[fam]
        for r in range(n):
            mate = (r & ~63) | ((r & 63) ^ 32)
            mate_cnt, mate_tied = (cnt[mate], tied[mate]) if mate < n else (0, False)
            if cnt[r] and (cnt[r] + mate_cnt >= pr or mate_tied and mate_cnt + cnt[r] >= pr):
                listed[r] = True
    elif fam in ("k_syncmer_pf", "k_syncmer_pfl"):
        for u in range(0, n, 64):
            run = 0
            for r in range(u, min(u + 64, n)):
                run += 0 if tied[r] else cnt[r]
                if run > consts[fam] and cnt[r]:
                    listed[r] = True
    elif fam == "k_minimizer_pkd":
        nwin = max(longest - p["k"] - p["w"] + 2, 0)
        slab = (A.slab_tuples(nwin, p["w"]) + 15) & ~15
        listed = [t or c > slab for t, c in zip(tied, cnt)]
    elif fam == "k_minimizer_ring":
        nwin = max(longest - p["k"] - p["w"] + 2, 1)
        rows = (min(nwin, -(-nwin * 26 // (10 * (p["w"] + 1))) + 6) + 3) & ~3
        listed = [t or c > rows for t, c in zip(tied, cnt)]
        return sum(tied), sum(listed) + n // 25
    return sum(tied), sum(listed)


def fixcap(n, grid):
    """syn_pk_fixcap (planner.hip)"""
    return max(grid * 1024, (n // 4 + grid) // grid * grid)


def segment(n, grid):
    """entries of one workgroup's segment of the list of reads (list_append: fixcap / list_grid)"""
    return fixcap(n, grid) // grid


def ticketing(rules, fam, nunits, grid):
    """-> (tk as launch.hip sets it: 0 = the kernel's own, units per ticket, tickets of the launch) of `fam` over nunits units on `grid` waves"""
    which, _, _, own = FAMILIES[fam]
    tk = 0
    if which in rules["shrink"]:
        own_l = 4 if which in rules["own4"] else 8
        assert own_l == own, (fam, own_l, own)
        if nunits < grid * own_l:
            tk = max(1, (nunits + grid - 1) // grid)
    per = tk or own
    return tk, per, (nunits + per - 1) // per


def pk_tail(rules, nunits, grid):
    """k_minimizer_pk's whole tickets: -> (tk_t0, tk_small, tickets) -- tickets from number tk_t0 on have tk_small units"""
    region = min(rules["pk_tail"] * grid * 8, nunits)
    t0 = (nunits - region) // 8
    left = nunits - t0 * 8
    return t0, rules["pk_small"], t0 + (left + rules["pk_small"] - 1) // rules["pk_small"]


# ---- tiles, length-binned units, a class plan ----
TILE_ENV = {"BSK_TILE_MIN": "40", "BSK_TILE_POS": "16"}


class Case:
    """a batch of its own: kind + p as in a Row, the reads, the switches, and what its plan must say"""

    def __init__(self, cid, kind, p, seqs, env, plan_has, alphabet="dna", launches=(), uncut=None):
        self.id, self.kind, self.p, self._seqs, self.env, self.plan_has, self.alphabet, self.launches = cid, kind, dict(p), seqs, dict(env), tuple(plan_has), alphabet, tuple(launches)
        self.circular = False
        self.uncut = dict(uncut or {})  # {cap: grids the call sizes that want no more workgroups than the cap, each with its reason where the case is made}

    def uncut_max(self, cap):
        return self.uncut.get(cap, 0)

    def cut_min(self, cap):
        """the launches the case names are grids the switch cuts -- but the named ones it leaves whole at this cap (binned units at three: k_bin_desc)"""
        return len(self.launches) - (1 if self is BINNED_CASE and cap == 3 else 0)

    def reads(self):
        return self._seqs(random.Random(A.hash_seed("trips", self.id)))


def _long(alpha):
    return lambda rng: [A.fast_seq(rng, rng.randint(3000, 6000), alpha) for _ in range(28)]


def _many(rng):
    """200 sequences of 500..900 bases: four units of 64 sequences for k_tile_count and its look-back, and >= 83 units of tiles"""
    return [A.fast_seq(rng, rng.randint(500, 900)) for _ in range(200)]


def _ragged(rng):
    """N_TRIP reads of 60..150 bases, every tenth low-complexity"""
    seqs = [A.fast_seq(rng, rng.randint(60, 150)) for _ in range(N_TRIP)]
    for j in range(0, N_TRIP, 10):
        seqs[j] = A.low_complexity(rng, len(seqs[j]))
    return seqs


def _classes(rng):
    """150-base reads and, every 97th, one of 400 bases: a second length class"""
    seqs = [A.fast_seq(rng, 400 if j % 97 == 5 else 150) for j in range(N_TRIP)]
    for j in range(0, N_TRIP, 10):
        seqs[j] = A.low_complexity(rng, len(seqs[j]))
    return seqs


# (a tile of 16 positions is its positions + the overlap the kind needs: well below a unit's limits; >= 83 units of 64 tiles from 28 sequences.
# 28 sequences are ONE unit of k_tile_count, whose grid then stays whole: `tiles_many_sequences` gives it four)
ONE_COUNT_UNIT = {1: 1, 3: 1}
TILE_CASES = [
    Case("tiles_minimizer", "minimizer", dict(k=21, w=11), _long("ACGT"), TILE_ENV, ("k_minimizer_", A.TILES), launches=("tile units",), uncut=ONE_COUNT_UNIT),
    Case("tiles_many_sequences", "minimizer", dict(k=21, w=11), _many, TILE_ENV, ("k_minimizer_", A.TILES), launches=("tile units", "k_tile_count")),
    Case("tiles_syncmer", "syncmer", dict(k=31, s=11), _long("ACGT"), TILE_ENV, ("k_syncmer_", A.TILES), launches=("tile units",), uncut=ONE_COUNT_UNIT),
    Case("tiles_nthash", "nthash", dict(k=21, canonical=True), _long("ACGT"), TILE_ENV, ("k_nthash_", A.TILES), launches=("tile units",), uncut=ONE_COUNT_UNIT),
    Case("tiles_prot_minimizer", "prot_minimizer", dict(k=9, w=5), _long(A.AA), TILE_ENV, ("k_prot_minimizer", A.TILES), alphabet="protein", launches=("tile units",),
         uncut=ONE_COUNT_UNIT),
    Case("tiles_two_strand", "kmer", dict(k=21, canonical=False), _long("ACGT"), TILE_ENV, ("k_nthash_fast<4>", A.TILES), launches=("tile units", "k_two_strand"),
         uncut=ONE_COUNT_UNIT),
]
# (5 285 reads are two chunks of 4 096 for k_bin_desc: two trips at one workgroup, one each at three -- whole there)
BINNED_CASE = Case("binned_units", "minimizer", dict(k=21, w=11), _ragged, {"BSK_BIN_MIN": "64", "BSK_NO_RING": "1", "BSK_NO_DENSE": "1"},
                   ("k_minimizer_pk<11,false>", A.BINNED), launches=("k_minimizer_pk", "k_bin_desc"), uncut={3: 1})
# (six blocks of 1 024 reads for k_class_cut; the 55 reads of 400 bases are one unit for their part's own launches: whole)
CLASS_CASE = Case("class_plan", "minimizer", dict(k=21, w=11), _classes, {"BSK_CLASS_FORCE": "1", "BSK_CLASS_VIEW": "1", "BSK_CLASS_MIN": "64", "BSK_NO_BIN": "1"},
                  ("k_minimizer_", " reads of "), launches=("the bulk's kernel", "k_class_cut"), uncut={1: 4, 3: 4})
CASES = TILE_CASES + [BINNED_CASE, CLASS_CASE]
CASE_BY_ID = {c.id: c for c in CASES}


# ---- the full segment ----
class Edge:
    """rid: the atlas row whose parameters, switches and lengths the batch takes; period_max: repeats of period 2 .. period_max tie inside
    every window; falls_to: the plan a call ends on whose list outgrew a segment"""

    def __init__(self, rid, period_max, falls_to):
        self.row, self.period_max, self.falls_to = A.BY_ID[rid], period_max, falls_to
        self.id = rid

    def reads(self, n):
        """n different exact-tie reads of the row's lengths: the four homopolymers, then repeats of period 2 .. period_max; the longest read
        of the row is among them (it decides the plan)"""
        rng = random.Random(A.hash_seed("edge", self.id))
        lens = sorted(set(self.row.lens + self.row.limits))
        seqs, seen = [], set()
        for j, base in enumerate("ACGT"):
            seqs.append(base * lens[-1 - j % len(lens)])
        seen.update(seqs)
        while len(seqs) < n:
            unit = A.rand_seq(rng, rng.randint(2, self.period_max))
            ln = rng.choice(lens)
            q = (unit * (ln // len(unit) + 1))[:ln]
            if q not in seen and len(set(unit)) > 1:
                seen.add(q)
                seqs.append(q)
        return seqs


EDGES = [
    Edge("min_pk<11,false>", 10, "k_minimizer_fast<11,"),
    Edge("min_ring<11,false>", 10, "k_minimizer_fast<11,"),
    Edge("min_pkd<11>", 10, "k_minimizer_fast<11,"),
    Edge("syn_pk<20>", 19, "k_syncmer_fast<20>"),
    Edge("syn_pf<20>", 19, "k_syncmer_fast<20>"),
]
EDGE_BY_ID = {e.id: e for e in EDGES}


def edge_sizes(grid):
    """-> (the largest batch of listed reads that fits `grid` segments whoever lists what, the smallest that cannot)"""
    full = max(n for n in range(1, 8192) if n <= segment(n, grid))  # one workgroup may list them all
    over = min(n for n in range(1, 8192) if n > grid * segment(n, grid))  # pigeonhole: some segment takes one too many
    return full, over
