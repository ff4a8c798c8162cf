"""CPU: what tests/sketch_programs.py claims about the campaign tests/test_gpu_sketch_programs.py runs -- 6 blocks of 16 seeded programs.

The generator is deterministic and every program stays inside the header's contract (a checker walks it); the model's records equal
a plain second implementation written here (per-read oracle calls, the fetch ranges, the narrow packing, the reference-word
decoding, the digest formula and the sets by hand, in Python integers, sets and Counters); every block and the whole campaign reach
the states the programs exist for (the thresholds below are caps that keep the campaign from hiding a failure: when a block misses
one, the generator's weights change, not the threshold); and every model of SP.SABOTAGES -- one piece of state left stale, named
after the host mistake it stands for -- is caught by the same comparison (SP.same) the GPU test uses, in every block."""
import collections
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import sketch_programs as SP

U64, U32, U16, U8 = np.uint64, np.uint32, np.uint16, np.uint8
MASK64 = (1 << 64) - 1


@functools.lru_cache(None)
def block(b):
    """the programs of a block with the model's records, and per sabotage the seeds at which SP.same tells it from the model"""
    O.build()
    progs, caught = [], collections.defaultdict(list)
    for seed in SP.seeds(b):
        prog, recs = SP.program_and_records(seed, O)
        progs.append((prog, recs))
        for sab in SP.SABOTAGES:  # (right after the program: its reads are still in the oracle cache)
            if SP.same(recs, SP.run(prog, sab(O))):
                caught[sab.name].append(seed)
    SP.clear_cache()
    return progs, caught


def campaign():
    return [pr for b in range(SP.BLOCKS) for pr in block(b)[0]]


# ---- the generator ----
def test_the_campaign_is_96_seeds_and_a_program_is_its_seed():
    all_seeds = [s for b in range(SP.BLOCKS) for s in SP.seeds(b)]
    assert all_seeds == list(range(SP.BASE, SP.BASE + 96)) and SP.BLOCKS * SP.PER_BLOCK == 96 and len(SP.THEMES) == SP.PER_BLOCK
    for seed in SP.seeds(0)[2:6] + SP.seeds(4)[8:14]:
        one, two = SP.program(seed, O), SP.program(seed, O)
        assert SP.describe(one) == SP.describe(two) and len(one) == len(two)
        assert SP.describe(one) != SP.describe(SP.program(seed + SP.PER_BLOCK, O))
    assert "python -m tests.sketch_programs" in SP.message(SP.BASE, 5, SP.program(SP.BASE, O), ["x"])


@pytest.mark.parametrize("b", range(SP.BLOCKS))
def test_every_program_stays_inside_the_contract(b):
    for prog, recs in block(b)[0]:
        assert 12 <= len(prog) <= 20 and len(recs) == len(prog) + 1, len(prog)
        assert SP.contract_violations(prog) == [], SP.describe(prog)


def test_the_checker_sees_a_program_that_leaves_the_contract():
    prog = [dict(s) for s in block(0)[0][8][0]]  # the re-filled batch
    at = next(i for i, s in enumerate(prog) if s["kind"] == "refill")
    sized = next(s for s in prog[:at] if s["kind"] == "sketch")
    late = dict(kind="timed", res=sized["res"], batch=sized["batch"], sketch=sized["sketch"], p=sized["p"], warmup=0, iters=1)
    assert SP.contract_violations(prog[:at] + [late]) == []
    assert any("timed re-run" in v for v in SP.contract_violations(prog[:at + 1] + [late]))  # after the refill
    fetches = [dict(s) for s in block(0)[0][5][0]]
    second = [i for i, s in enumerate(fetches) if s["kind"] == "compact_read"][1]
    assert any("compact" in v for v in SP.contract_violations(fetches[:second] + [fetches[second]] * 2))
    assert any("outside the allowed" in v for v in SP.contract_violations([dict(kind="switch", env={"BSK_NO_PK": "1"})]))
    assert any("released" in v for v in SP.contract_violations([dict(kind="read", res="r9", how="info")]))
    bare = [{k: v for k, v in s.items() if k != "recheck"} for s in prog]
    assert any("no other live result is fetched again" in v for v in SP.contract_violations(bare))


def test_same_reports_what_differs():
    a = dict(n=3, v=np.array([1, 2, 3], U64), c=None, sub={"x": (np.zeros(2, U32), np.ones(2, U8))})
    assert SP.same(a, dict(a)) == []
    for change in (dict(n=4), dict(v=np.array([1, 2, 4], U64)), dict(v=np.array([1, 2, 3], np.int64)), dict(v=np.array([1, 2], U64)), dict(c=np.zeros(0, U32)), dict(sub={"y": 1})):
        assert len(SP.same(a, {**a, **change})) == 1, change


# ---- the model against a plain second implementation ----
def plain_read(kind, p, protein, q):
    """(code, flags, hashes, positions, strands) of one read: a per-read oracle call, nothing shared with SP.oracle_read"""
    k, circ = p["k"], bool(p.get("circular"))
    non_acgt = any(c not in b"ACGTacgt" for c in q)
    try:
        if kind == "minimizer":
            h, ps, st, fl = O.minimizer(q, k, p["w"], circ, closed=True)
            return 0, (fl & 0x10) | (0x20 * non_acgt), list(map(int, h)), list(map(int, ps)), list(map(int, st))
        if kind == "syncmer":
            h, ps, st, fl = O.syncmer(q, k, p["s"], circ, closed=True)
            return 0, (fl & 0x10) | (0x20 * non_acgt), list(map(int, h)), list(map(int, ps)), list(map(int, st))
        if kind == "nthash":
            return 0, 0x20 * non_acgt, list(map(int, O.nthash(q, k, p["canonical"], circ)[0])), None, None
        if kind == "kmer":
            return 0, 0, list(map(int, O.kmer_codes(q, k, p["canonical"], circ, 0))), None, None
        if kind == "simhash":
            return 0, 0x20 * non_acgt, list(map(int, O.simhash(q, k, p["m"], p["scale"], True))), None, None
        if kind == "prot_hash":
            h = O.protein_hashes(q, k) if protein else O.protein_hashes_nt(q, k, p["codon_table"], p["frame"])
            return 0, 0, list(map(int, h)), None, None
        h, ps, fl = O.protein_minimizer(q, k, p["w"], closed=True) if protein else O.protein_minimizer_nt(q, k, p["w"], p["codon_table"], p["frame"])
        return 0, fl & 0x10, list(map(int, h)), list(map(int, ps)), [0] * len(h)
    except O.OracleError as e:
        assert e.name == "ErrShortSeq", e.name
        return 1, 0, [], ([] if kind in SP.POSITIONAL else None), ([] if kind in SP.POSITIONAL else None)


def arr(xs, dt):
    return np.array(list(xs), dt)


def plain_fetch(reads, first, count, has_pos, narrow=False):
    rs = reads[first:first + count]
    offs, at = [0], 0
    for r in rs:
        at += len(r[2])
        offs.append(at)
    pos = None
    if has_pos:
        pos = [p | (s << (15 if narrow else 31)) for r in rs for p, s in zip(r[3], r[4])]
    return dict(offsets=arr(offs, U32 if narrow else U64), code=arr((r[0] for r in rs), U8), flags=arr((r[1] for r in rs), U8), hash=arr((h for r in rs for h in r[2]), U64),
                pos=None if pos is None else arr(pos, U16 if narrow else U32))


def plain_sets(reads, whole, scale, counted):
    maxhash = MASK64 // scale if scale > 1 else MASK64
    scopes = [[h for r in reads for h in r[2]]] if whole else [r[2] for r in reads]
    offs, vals, cnts = [0], [], []
    for sc in scopes:
        c = collections.Counter(h for h in sc if h <= maxhash)
        vals += sorted(c)
        cnts += [c[v] for v in sorted(c)]
        offs.append(len(vals))
    return dict(offsets=arr(offs, U64), values=arr(vals, U64), counts=arr(cnts, U32) if counted else None)


def plain_record(s, reads, has_pos):
    """what a read step of result `reads` yields, by hand (None: not restated here)"""
    how, n = s["how"], len(reads)
    T = sum(len(r[2]) for r in reads)
    if how == "info":
        return dict(n_reads=n, n_tuples=T, has_pos=has_pos)
    if how == "fetch":
        return plain_fetch(reads, s["first"], s["count"], has_pos)
    if how == "narrow":
        if has_pos and any(p >= 32768 for r in reads[s["first"]:s["first"] + s["count"]] for p in r[3]):
            return dict(refused="BSK_ERR_UNSUPPORTED")
        return plain_fetch(reads, s["first"], s["count"], has_pos, narrow=True)
    if how == "status":
        f = plain_fetch(reads, s["first"], s["count"], has_pos)
        return dict(code=f["code"], flags=f["flags"])
    if how == "digest":
        ck = 0
        for r in reads:
            for j, h in enumerate(r[2]):
                ck = (ck + h * (2 * (r[3][j] if has_pos else j) + 1)) & MASK64
        return dict(checksum=ck, n_tuples=T, short=sum(r[0] == 1 for r in reads), illegal=0)
    if how in ("sets", "counted"):
        return plain_sets(reads, s["whole"], s["scale"], how == "counted")
    if how == "device":
        rec = plain_fetch(reads, 0, n, has_pos)
        rec["layout_ok"] = True
        return rec
    return None


@pytest.mark.parametrize("b", range(SP.BLOCKS))
def test_the_model_agrees_with_a_plain_second_implementation(b):
    done = collections.Counter()
    for seed, (prog, recs) in zip(SP.seeds(b), block(b)[0]):
        batches, results, compact, classed, owner = {}, {}, None, set(), None  # (owner: the result whose class plan the context's lists describe)
        for s, both in zip(prog, recs):
            rec = both["step"] if s.get("recheck") is not None else both
            k = s["kind"]
            for x in ([s["a"], s["b"]] if k == "make2" else [s] if k in ("make", "refill") else []):
                batches[x["slot"]] = (list(x["seqs"]), x["protein"])
            if k == "translate":
                batches[s["slot"]] = ([O.translate(q, s["table"], s["frame"]).encode("latin-1") if len(q) >= 3 else b"" for q in batches[s["src"]][0]], True)
                want = b"".join(batches[s["slot"]][0])
                assert rec["bytes"].tobytes() == want and rec["n_bases"] == len(want), SP.message(seed, prog.index(s), prog, "translate")
                done["translate"] += 1
            elif k == "destroy":
                del batches[s["slot"]]
            elif k == "sketch":
                seqs, protein = batches[s["batch"]]
                results[s["res"]] = ([plain_read(s["sketch"], s["p"], protein, q) for q in seqs], s["sketch"] in SP.POSITIONAL)
                want = plain_record(dict(how="info"), *results[s["res"]])
                assert SP.same(want, rec) == [], SP.message(seed, prog.index(s), prog, "sketch")
                classed = (classed | {s["res"]}) if s["classed"] else classed - {s["res"]}
                owner = s["res"] if s["classed"] else owner
            elif k == "release":
                del results[s["res"]]
                owner = None if owner == s["res"] else owner
            elif k in ("read", "timed", "compact_read"):
                if k == "read" and s["how"] == "compact":
                    reads, has_pos = results[s["res"]]
                    compact = dict(plain_fetch(reads, 0, len(reads), has_pos), n_tuples=sum(len(r[2]) for r in reads))
                    del compact["code"], compact["flags"]
                    continue
                want = compact if k == "compact_read" else plain_record(s, *results[s["res"]]) if k == "read" else \
                    dict(info=plain_record(dict(how="info"), *results[s["res"]]), all=plain_fetch(results[s["res"]][0], 0, len(results[s["res"]][0]), results[s["res"]][1]))
                if k == "timed" and s["res"] in classed and owner != s["res"]:  # the documented refusal: the result as it was
                    want = dict(refused="BSK_ERR_ARG", all=want["all"])
                    done["timed refused"] += 1
                assert SP.same(want, rec) == [], SP.message(seed, prog.index(s), prog, SP.same(want, rec))
                done[s.get("how", k)] += 1
            if s.get("recheck") is not None:
                reads, has_pos = results[s["recheck"]]
                assert SP.same(plain_fetch(reads, 0, len(reads), has_pos), both["recheck"]) == [], SP.message(seed, prog.index(s), prog, "the re-read of %s" % s["recheck"])
        end = recs[-1]
        assert set(end["results"]) == set(results) and set(end["batches"]) == set(batches)
        for i, (reads, has_pos) in results.items():
            assert SP.same(plain_fetch(reads, 0, len(reads), has_pos), end["results"][i]) == [], i
        for i, (seqs, _) in batches.items():
            assert end["batches"][i]["bytes"].tobytes() == b"".join(seqs) and list(np.diff(end["batches"][i]["offsets"])) == [len(q) for q in seqs], i
    assert all(done[h] >= 1 for h in SP.READS if h != "compact") and done["compact_read"] >= 2 and done["timed"] >= 1 and done["timed refused"] == 2 and done["translate"] >= 3, done


def test_the_decoder_reads_rows_and_dense_results():
    """SP.decode_refs / tuple_index (what the GPU test decodes bsk_result_device with) on hand-made reference words"""
    refs = arr([(5 << 24) | 3, (1 << 63) | (100 << 24) | 2, (1 << 63) | (101 << 24) | 0, (200 << 24) | 1], U64)
    first, count, stride = SP.decode_refs(refs)
    assert first.tolist() == [5, 100, 101, 200] and count.tolist() == [3, 2, 0, 1] and stride.tolist() == [1, 64, 64, 1]
    assert SP.tuple_index(first, count, stride).tolist() == [5, 6, 7, 100, 164, 200]
    r = SP.result_of("minimizer", dict(k=21, w=11), [(0, 0, arr([7, 8, 9], U64), arr([1, 5, 1 << 31], U32)), (1, 0, np.zeros(0, U64), np.zeros(0, U32))] * 40)
    raw = SP.raw_layout(r)
    f, c, st = SP.decode_refs(raw[0])
    assert set(st.tolist()) == {64} and np.array_equal(raw[1][SP.tuple_index(f, c, st)], r["hash"]) and np.array_equal(raw[2][SP.tuple_index(f, c, st)], r["pos"])


# ---- what the campaign reaches ----
ORDERS = {(a, b) for a in ("pure", "flagged", "fixed", "ragged", "empty") for b in ("pure", "flagged", "fixed", "ragged", "empty") if a != b}


@pytest.mark.parametrize("b", range(SP.BLOCKS))
def test_what_a_block_reaches(b):
    f = SP.figures(block(b)[0])
    assert f["kinds"] == set(SP.KINDS), set(SP.KINDS) - f["kinds"]
    assert f["kind_changes"] >= 10, f["kind_changes"]
    assert f["pos_to_stream"] >= 3 and f["stream_to_pos"] >= 3 and f["grows"] >= 3 and f["layout_changes"] >= 3, f
    assert f["refill_orders"] >= ORDERS, ORDERS - f["refill_orders"]
    assert f["both_refills"] >= 1, "no object re-filled through both entries"
    assert f["tiled_sets_tiled"] >= 1 and f["fetch_narrow_fetch"] >= 1 and f["compact_later"] >= 1 and f["class_pairs_timed"] >= 1 and f["table_aba"] >= 1, f
    assert f["reserve_pairs"] >= 3, f["reserve_pairs"]
    assert f["reads"] == set(SP.READS), set(SP.READS) - f["reads"]
    assert max(f["bases"]) <= SP.BASES_BUDGET * 1.25, f["bases"]
    assert 20 * f["refused"] <= f["steps"], (f["refused"], f["steps"])


def test_what_the_campaign_reaches():
    f = SP.figures(campaign())
    assert f["tables"] == set(SP.genetic_codes(O)) and f["frames"] == set(SP.FRAMES), (set(SP.genetic_codes(O)) - f["tables"], f["frames"])
    assert f["entries"] == {"bsk_batch_from_ascii", "bsk_batch_from_packed", "bsk_batch_refill_ascii", "bsk_batch_refill_packed", "bsk_sketch_timed"}, f["entries"]
    assert f["switches"] == set(SP.SWITCHES), set(SP.SWITCHES) - f["switches"]
    assert f["refused"] >= 1, "no narrow fetch of a read of 32 768 bases or more"
    shapes, fixed = collections.Counter(), set()
    for prog, _ in campaign():
        for s in prog:
            for x in ([s["a"], s["b"]] if s["kind"] == "make2" else [s] if s["kind"] in ("make", "refill") else []):
                lens = [len(q) for q in x["seqs"]]
                shapes["empty"] += not lens
                shapes["protein"] += x["protein"]
                shapes["5000"] += 5000 in lens
                shapes["32768+"] += max(lens, default=0) >= SP.NARROW_LIMIT
                shapes["all too short"] += bool(lens) and max(lens) < 9
                shapes["every read flagged"] += bool(lens) and not x["protein"] and all(SP.flagged(q) for q in x["seqs"])
                if set(lens) == {150}:
                    fixed.add(len(lens))
    assert all(shapes[k] >= 1 for k in ("empty", "protein", "5000", "32768+", "all too short", "every read flagged")), shapes
    assert fixed >= set(SP.UNIT_EDGES) and any(1100 <= n <= 2200 for n in fixed), sorted(fixed)


# ---- the campaign sees the host mistakes these entries can make ----
@pytest.mark.parametrize("b", range(SP.BLOCKS))
def test_every_sabotaged_model_is_caught_in_every_block(b):
    caught = block(b)[1]
    print({name.split()[0]: len(seeds) for name, seeds in caught.items()})
    for sab in SP.SABOTAGES:
        assert caught[sab.name], "block %d: nothing tells `%s` from the model" % (b, sab.name)
