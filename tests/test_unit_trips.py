"""The unit-trip cases (tests/unit_trips.py) keep their shape -- no GPU.

Held against the sources, the way tests/test_sets_cases.py holds its thresholds: launch.hip's units-per-ticket rule, planner.hip's
syn_pk_fixcap and every kernel's own ticket size are READ there, and must still give, for N_TRIP reads at BSK_UNIT_GRID 1 and 3, several
tickets per wave with `tk` left alone, and between 65 listed reads and a full segment in one workgroup's piece of the list.  The rows are the
selection rule applied to the plan atlas: a family the atlas gains fails here by name until a trip row runs it.  And no kernel that takes
its units from eight ticket heads is launched through the helper behind the switch (host_types.hpp: unit_grid).
"""
import os
import re

import pytest

from tests import plan_atlas as A
from tests import unit_trips as T
from tests.test_plan_atlas import _has_equal_pair_in_a_window

CSRC = T.CSRC


def _code(name):
    """a source file without its // comments"""
    return re.sub(r"//[^\n]*", "", T.source(name))


@pytest.fixture(scope="module")
def rules():
    return T.launch_rules()


# ---- the shape ----
def test_batch_is_83_units_and_the_last_ticket_is_partial_for_both_sizes():
    assert T.N_TRIP == 82 * 64 + 37 == 5285 and T.UNITS == 83 and T.N_TRIP % 64 == 37
    assert T.UNITS % 8 == 3 and T.UNITS % 4 == 3 and T.CAPS == (1, 3)
    assert all(8 % g or g == 1 for g in T.CAPS) and 8 % 3 and 4 % 3  # three waves divide neither a ticket nor the eight XCDs


def test_every_family_states_its_own_ticket_where_the_table_says(rules):
    plan_names = T.source("planner.hip")
    for fam, (which, fn, text, own) in T.FAMILIES.items():
        assert text in T.source(fn), (fam, fn, text)
        sizes = re.findall(r"(\d+)u\b", text)
        assert own == (int(sizes[-1]) if sizes else 1), (fam, text, own)  # (no figure: the ticket IS the unit)
        m = re.search(r"case %s:\s*snprintf\(b, sizeof b, ([^;]*);" % which, plan_names)
        assert m and ('"%s<' % fam in m.group(1) or '"%s"' % fam in m.group(1)), (fam, which)  # plan_name spells this family for this Which
        if which in rules["shrink"]:
            assert (4 if which in rules["own4"] else 8) == own, (fam, which, own)
    assert rules["own4"] <= rules["shrink"] and rules["lists"] - {"K_SYN_SEL"} <= rules["shrink"]
    assert {w for f, (w, _, _, _) in T.FAMILIES.items() if T.lists_reads(f + "<")} == rules["lists"] - {"K_SYN_SEL"}  # (K_SYN_SEL: make EXPERIMENTS=1 only)


@pytest.mark.parametrize("grid", T.CAPS)
def test_several_tickets_per_wave_and_tk_untouched(rules, grid):
    for fam in T.FAMILIES:
        tk, per, tickets = T.ticketing(rules, fam, T.UNITS, grid)
        assert tk == 0, (fam, grid, tk)  # launch.hip leaves the kernel's own ticket: 83 >= grid x own
        assert per == T.FAMILIES[fam][3] and T.UNITS >= grid * per
        assert -(-tickets // grid) >= 4, (fam, grid, tickets)  # pigeonhole: some wave takes four tickets or more
        assert per == 1 or T.UNITS % per, (fam, per)  # ... and the last ticket is partial
        # with the switch unset the same batch is one unit per wave and ticket: the other ticketing the digests are compared with
        tk_unset, per_unset, n_unset = T.ticketing(rules, fam, T.UNITS, T.UNITS)
        assert (tk_unset, per_unset, n_unset) == ((1, 1, T.UNITS) if T.FAMILIES[fam][0] in rules["shrink"] else (0, per, tickets)), fam
    t0, small, tickets = T.pk_tail(rules, T.UNITS, grid)
    assert (t0, small) == ({1: 9, 3: 7}[grid], 3) and 0 < t0 < tickets  # k_minimizer_pk walks from eight-unit into three-unit tickets
    assert ((T.UNITS - 8 * t0) % small != 0) == (grid == 1)  # (27 units in nine whole small tickets at three waves, 11 in four at one: the last partial)
    assert -(-tickets // grid) >= 4


# ---- the rows ----
def test_rows_are_the_selection_rule_over_the_atlas():
    want = [r.id for r in T.selected()]
    assert [r.id for r in T.ROWS] == want and len(want) == len(set(want))
    groups = {}
    for r in A.ROWS:
        if T.eligible(r):
            g, num = T.group_of(r)
            groups.setdefault(g, []).append((num, r.id))
    have = set(want)
    for g, members in groups.items():
        assert g[0] in T.FAMILIES, "kernel family %s of the plan atlas has no entry in tests/unit_trips.py FAMILIES (its own ticket size) and no trip row" % g[0]
        nums = [n for n, _ in members if n is not None]
        for num, rid in members:
            ends = num is None or num in (min(nums), max(nums))
            assert (rid in have) == ends, (g, rid, num)
    # a family that only has fallback / tile / binned rows would be left out silently: name it
    for r in A.ROWS:
        assert T.family(r.name) in {T.family(x.name) for x in T.ROWS} | {"k_minimizer_pft"}, "kernel family %s has no trip row" % T.family(r.name)
    names = {x.name for x in T.ROWS}
    for must in ("k_minimizer_pk<2,false>", "k_minimizer_pk<13,true>", "k_minimizer_ring<2,false>", "k_minimizer_ring<13,true>", "k_minimizer_pkd<2>", "k_minimizer_pkd<13>",
                 "k_minimizer_dense<1>", "k_minimizer_dense<16>", "k_minimizer_fast<2,", "k_minimizer_fast<32,", "k_syncmer_pk<4>", "k_syncmer_pk<20>", "k_syncmer_pkl<4>",
                 "k_syncmer_pkl<24>", "k_syncmer_pf<8>", "k_syncmer_pf<20>", "k_syncmer_pfl<8>", "k_syncmer_pfl<24>", "k_syncmer_fast<2>", "k_syncmer_fast<32>",
                 "k_nthash_fast<0>", "k_nthash_fast<1>", "k_nthash_fast<2>", "k_nthash_fast<3>", "k_simhash_fast<5,12>", "k_simhash_fast<5,20>", "k_simhash_fast<5,34>",
                 "k_simhash_fast<6,12>", "k_simhash_fast<6,20>", "k_simhash_fast<6,34>", "k_prot_hash_fast<4,false>", "k_prot_hash_fast<16,true>",
                 "k_prot_minimizer_fast<2,4,false>", "k_prot_minimizer_fast<8,16,true>", "k_minimizer_generic<0>", "k_minimizer_generic<1>", "k_nthash_stream<0>",
                 "k_nthash_stream<1>", "k_syncmer<0>", "k_syncmer<1>", "k_kmer<0>", "k_kmer<1>", "k_simhash<0>", "k_simhash<1>", "k_prot_hash", "k_prot_minimizer"):
        assert must in names, must
    assert any(A.SIDE in x.suffixes and x.name.startswith("k_minimizer_dense<") for x in T.ROWS)  # the ASCII side launch and its side_grid
    assert any(A.SIDE in x.suffixes and x.name.startswith("k_syncmer_fast<") for x in T.ROWS)
    # k_nthash_fast<4> and k_minimizer_pft only exist over tiles: the first runs in the tile cases, the second keeps its own grid (below)
    assert any("k_nthash_fast<4>" in c.plan_has for c in T.TILE_CASES)


def test_rows_hold_n_trip_reads_of_the_atlas_generator():
    for t in T.ROWS:
        row = A.BY_ID[t.id]
        seqs = t.reads()
        assert len(seqs) == T.N_TRIP and t.n + len(t.extra) == T.N_TRIP, t.id
        longest = max(len(q) for q in seqs)
        assert longest == max(t.lens + t.limits), t.id  # the longest read decides the plan ...
        if t.id in T.TRIP_LENS:  # ... shorter plain reads (k_minimizer_pk's columns): on the same side of the kernel's LONG limit, the limits' reads themselves kept
            assert T.family(t.name) == "k_minimizer_pk" and max(t.lens) < max(row.lens) and t.limits == row.limits
            assert (longest > A.PK_SHORT_BASES) == (max(row.lens + row.limits) > A.PK_SHORT_BASES) and min(t.lens) >= row.min_len(), t.id
        else:
            assert t.lens == row.lens and longest == max(row.lens + row.limits), t.id
        assert seqs[3] == "" and len(set(seqs[1])) == 1 and [len(seqs[i]) for i in t.limit_indices()] == list(row.limits), t.id
        assert t.env == dict(row.env, BSK_NO_BIN="1") and t.name == row.name and t.suffixes == row.suffixes and t.p == row.p
        assert len(row.extra) <= len(t.extra) <= len(row.extra) + T.TIE_EXTRA


@pytest.mark.parametrize("rid", [r.id for r in T.ROWS if T.lists_reads(r.name)])
def test_listed_reads_fill_a_segment_past_one_chunk_and_not_to_its_end(oracle, rules, rid):
    """exact ties inside a window are what the packed machines must list (27-bit key ties on top of them are a read in ten million
    windows; k_minimizer_ring also lists the lanes that outran its ring -- up to 4 % of the reads, launch.hip's own figure)"""
    t = T.BY_ID[rid]
    assert T.FAMILIES[T.family(t.name)][0] in rules["lists"]
    pk_rows = int(re.search(r"#define BSK_PK_ROWS (\d+)", T.source("kernels_pk.hpp")).group(1))
    assert "u64 bad = __builtin_amdgcn_ballot_w64(cnt_pair >= (u32)LY::PR);" in T.source("kernels_pk.hpp") and "static constexpr int PR = BSK_PK_ROWS;" in T.source("kernels_pk.hpp")
    consts = {"k_minimizer_pk": pk_rows, "k_syncmer_pk": A.SYN_PAIR_ROWS[False], "k_syncmer_pkl": A.SYN_PAIR_ROWS[True], "k_syncmer_pf": A.SYN_PF_TUPLES[False],
              "k_syncmer_pfl": A.SYN_PF_TUPLES[True]}  # (tests/test_plan_atlas.py holds the syncmer figures against the headers)
    must, may = T.listed_bounds(oracle, t, t.reads(), consts)
    assert must <= may and (t.id in T.TIE_ROWS) == (len(t.extra) > len(A.BY_ID[t.id].extra))
    for grid in T.CAPS:
        seg = T.segment(T.N_TRIP, grid)
        assert seg == {1: 1322, 3: 1024}[grid]
        assert -(-must // grid) >= 65, (rid, grid, must)  # some workgroup's segment holds more than one chunk of 64 for the list pass
        assert may + 16 <= seg, (rid, grid, must, may, seg)  # ... and none can fill up, whoever draws which ticket: no fall-back here


# ---- the full segment ----
def test_edge_sizes_come_from_syn_pk_fixcap(rules):
    assert T.fixcap(1024, 1) == 1024 and T.fixcap(1025, 1) == 1024 and T.fixcap(T.N_TRIP, 1) == 1322 and T.fixcap(T.N_TRIP, 3) == 3072
    assert T.edge_sizes(1) == (1024, 1025) and T.edge_sizes(3) == (1024, 3 * 1024 + 1)
    for e in T.EDGES:
        fam = T.family(e.row.name)
        assert T.FAMILIES[fam][0] in rules["lists"], e.id
        for n, grid in ((1024, 1), (1025, 1), (3073, 3)):
            units = (n + 63) // 64
            assert T.ticketing(rules, fam, units, grid)[0] == 0, (e.id, n, grid)  # whole tickets here too: 16, 17 and 49 units


@pytest.mark.parametrize("eid", [e.id for e in T.EDGES])
def test_edge_reads_are_all_different_and_all_tie(oracle, eid):
    e = T.EDGE_BY_ID[eid]
    p = e.row.p
    span = p["w"] if e.row.kind == "minimizer" else 2 * (p["k"] - p["s"])
    assert e.period_max < (p["w"] if e.row.kind == "minimizer" else p["k"] - p["s"]) and e.period_max < span
    seqs = e.reads(3073)
    assert len(set(seqs)) == 3073 and e.reads(1025) == seqs[:1025] and e.reads(1024) == seqs[:1024]
    assert max(len(q) for q in seqs[:1024]) == max(e.row.lens + e.row.limits) and min(len(q) for q in seqs) >= e.row.min_len()
    assert [q for q in seqs[:4]] == [b * len(q) for b, q in zip("ACGT", seqs[:4])]
    assert all(_has_equal_pair_in_a_window(oracle, e.row, q) for q in seqs)


# ---- the switch stays off the kernels that wait for units nobody may have taken ----
def _kernel_bodies():
    """{kernel: body} of every __global__ function in the kernel headers"""
    out = {}
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith(".hpp"):
            continue
        src = _code(fn)
        for m in re.finditer(r"__global__[^;{]*?\bvoid (\w+)\(", src):
            start = src.index("{", m.end())
            depth, i = 0, start
            while True:
                depth += {"{": 1, "}": -1}.get(src[i], 0)
                if depth == 0:
                    break
                i += 1
            out[m.group(1)] = src[start:i]
    return out


def _statement_with(src, at):
    """the statement around position `at`, and the definitions of the identifiers it sizes its grid with (`x = ...;` above it)"""
    begin = max(src.rfind(";", 0, at), src.rfind("{", 0, at), src.rfind("}", 0, at)) + 1
    end = src.index(";", at)
    stmt = src[begin:end]
    defs = []
    for ident in set(re.findall(r"\b(\w*grid\w*)\b", stmt)) - {"unit_grid", "capped_grid", "dim3"}:
        defs += re.findall(r"[^;{}]*\b%s = [^;]*;" % ident, src[:begin])[-2:]
    return stmt + "\n" + "\n".join(defs)


def test_no_kernel_on_eight_ticket_heads_is_launched_through_the_helper():
    bodies = _kernel_bodies()
    heads = {name for name, body in bodies.items() if "HeadTickets" in body or "xcc_id()" in body}
    assert heads == set(T.HEAD_TICKET_KERNELS), "kernels that take units from the eight ticket heads: %s (tests/unit_trips.py HEAD_TICKET_KERNELS)" % sorted(heads)
    launchers = {"k_minimizer_pft": "pft_minimizer_launch"}
    seen = set()
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith((".hip", ".hpp", ".cpp")):
            continue
        src = _code(fn)
        for k in heads:
            for m in re.finditer(r"hipLaunchKernelGGL\(\(?%s\b|(?<!void )\b%s\(" % (k, launchers.get(k, k + "_no_launcher")), src):
                text = _statement_with(src, m.start())
                seen.add(k)
                assert "unit_grid" not in text, "%s: %s is sized through unit_grid (BSK_UNIT_GRID): it takes units from eight heads and would wait for a unit nobody took\n%s" % (fn, k, text)
    assert seen == heads, sorted(heads - seen)


def test_the_helper_sizes_the_grids_the_switch_is_for():
    planner, tiles, classes = _code("planner.hip"), _code("tiles.hip"), _code("classes.hip")
    assert "pl.grid = (int)unit_grid(ctx," in planner and planner.count("pl.side_grid = (int)unit_grid(ctx,") == 2
    assert planner.index("if (ctx->opt.waves_per_cu) per_cu") < planner.index("pl.grid = (int)unit_grid(ctx,") < planner.index("pl.ring_entries = (size_t)pl.grid")
    assert "const unsigned bin_grid = unit_grid(ctx," in planner and planner.count("dim3(bin_grid)") == 2
    assert "hipLaunchKernelGGL(k_tile_count, dim3(unit_grid(ctx," in tiles and "hipLaunchKernelGGL(k_two_strand, dim3(unit_grid(ctx," in tiles
    assert "hipLaunchKernelGGL(k_class_cut, dim3(unit_grid(ctx," in classes
    n_calls = sum(len(re.findall(r"\bunit_grid\(ctx,", _code(fn))) for fn in os.listdir(CSRC) if fn.endswith((".hip", ".cpp")))
    assert n_calls == 7, n_calls  # pl.grid, two side grids, k_bin_desc, k_tile_count, k_two_strand, k_class_cut: a new call site is read for waiting loops first
    # everything else follows pl.grid by itself
    launch = _code("launch.hip")
    for text in ("syn_pk_fixcap(b->n, pl.grid)", "a.list_grid = (u32)pl.grid;", "const u64 waves = (u64)std::max(pl.grid, 1);", "std::min(pl.grid, ctx->cus * 8)"):
        assert text in launch, text
    assert "pl.side_grid = sd.grid;" in planner and "pl.ring_entries = (size_t)pl.grid * pl.ring_w * 64;" in planner
