"""CPU: what tests/index_programs.py claims about the campaign tests/test_gpu_index_fuzz.py runs -- 8 blocks of 20 seeded programs over the
long-lived indexes, the window sets and the weighted and folded hits, beside the 12 blocks of tests/algebra_programs.py and the 8 of
tests/graph_programs.py, which stay what they were (both pinned below).

The generator is deterministic; its records are run_model's; the model agrees with brute force written here with Python sets, dicts and
integers (windows cut tuple by tuple, searches pair by pair, folds hit by hit, the formulas in Python floats); the campaign reaches the
states the fuzz exists for -- the floors below are conditions, not measurements: when the campaign misses one, the generator changes, not the
floor --; and every sabotaged model of IP.SABOTAGES is caught by the same comparison (AP.same) the GPU test uses.

Wall time of this module on the build machine: 29 s, 13 to 19 s of it the two older campaigns generated again for their pins, beside 17 s of
tests/test_graph_programs.py."""
import collections
import functools
import math
import zlib

import numpy as np
import pytest

from tests import algebra_programs as AP
from tests import graph_programs as GP
from tests import index_programs as IP
from tests import search_cases as SR
from tests import search_counted_cases as SW
from tests import setops_cases as SO
from tests import window_cases as WN
from tests.test_algebra_programs import as_counters, as_sets, brute_step as brute_sets_step
from tests.test_graph_programs import brute_step as brute_graph_step

U64, U32, I64 = np.uint64, np.uint32, np.int64
MAX64 = (1 << 64) - 1
AP_CRC = 0x85BE8B09  # of AP.describe(AP.program(seed)) over AP's 240 seeds (pinned in tests/test_graph_programs.py as well)
GP_CRC = 0xD065E092  # of GP.describe(GP.program(seed)) over GP's 160 seeds, taken before this campaign was written
SMALL = 4000         # brute force takes the steps whose operands hold at most so many values
PAIRS_WORK = 150_000


@functools.lru_cache(None)
def block(b):
    """the programs of a block with the model's records"""
    return [IP.program_and_records(seed) for seed in IP.seeds(b)]


@functools.lru_cache(None)
def campaign():
    return [pr for b in range(IP.BLOCKS) for pr in block(b)]


# ---- the generator ----
def test_the_older_campaigns_are_what_they_were():
    for mod, crc_want, n in ((AP, AP_CRC, 240), (GP, GP_CRC, 160)):
        crc = 0
        for b in range(mod.BLOCKS):
            for seed in mod.seeds(b):
                crc = zlib.crc32(mod.describe(mod.program(seed)).encode(), crc)
        assert mod.BLOCKS * mod.PER_BLOCK == n and crc == crc_want, (mod.__name__, "%08X" % crc)


def test_the_campaign_is_160_seeds_and_a_program_is_its_seed():
    all_seeds = [s for b in range(IP.BLOCKS) for s in IP.seeds(b)]
    assert all_seeds == list(range(IP.BASE, IP.BASE + 160))
    assert not set(all_seeds) & (set(range(AP.BASE, AP.BASE + 240)) | set(range(GP.BASE, GP.BASE + 160)))
    for seed in IP.seeds(0)[:5] + IP.seeds(5)[:5]:
        one, two = IP.program(seed), IP.program(seed)
        assert IP.describe(one) == IP.describe(two) and len(one) == len(two)
        assert IP.describe(one) != IP.describe(IP.program(seed + 1))
        steps = [s for s in one if s["kind"] not in ("load", "sketch")]
        assert 10 <= len(steps) <= 16 and len(one) - len(steps) == 4
        assert [s["kind"] for s in one[:4]].count("sketch") == 1  # the window sets need a result with positions
        sources = [s["counted"] if s["kind"] == "sketch" else s["counts"] is not None for s in one[:4]]
        assert any(sources) and not all(sources), sources
    assert "python -m tests.index_programs" in IP.message(IP.BASE, 5, IP.program(IP.BASE), ["x"])
    from tests.test_gpu_fold import RULES
    assert IP.RULES == RULES and len(IP.SABOTAGES) >= 10 and 0.0 in IP.COVERS and 1.0 in IP.COVERS


def test_the_generator_s_records_are_run_model_s():
    for prog, recs in block(2)[:10]:
        again = IP.run_model(prog)
        assert len(again) == len(recs) == len(prog) + 1
        for i, (x, y) in enumerate(zip(recs, again)):
            assert AP.same(x, y) == [], i
        assert IP.first_difference(prog, recs, IP.Model()) is None
        replayed = IP.Model()
        replayed.kinds = ()  # every step replayed from its record: the state at the end is the same
        assert IP.first_difference(prog, recs, replayed) is None


def test_run_model_takes_the_device_s_tuples():
    """other tuples for the sketch step: the sets of the sketch and the window sets follow them"""
    prog, recs = block(0)[0]
    sk = [s for s in prog if s["kind"] == "sketch"][0]
    o, h, p = IP.standin_tuples(sk)
    again = IP.run_model(prog, tuples=(o, h ^ U64(1), p))
    i = prog.index(sk)
    assert AP.same(recs[i], again[i]) != [] and AP.same(recs[0 if i else 1], again[0 if i else 1]) == []


# ---- the model against brute force ----
def py(t):
    """sets (offsets, values, counts or None) -> per set a dict value -> count (1 without counts)"""
    return [dict(c) for c in as_counters(t)]


def brute_windows(tuples, s):
    """the window sets tuple by tuple -> (group_offsets, offsets, values, counts)"""
    offs, hash_, pos = tuples
    maxhash = MAX64 // s["scale"] if s["scale"] > 1 else MAX64
    go, sets = [0], []
    for i in range(len(offs) - 1):
        a, b = int(offs[i]), int(offs[i + 1])
        ps = [(int(pos[j]) & 0x7FFFFFFF) if pos is not None else j - a for j in range(a, b)]
        wins = []
        if ps:
            last = ps[-1]
            if s.get("count"):
                W = S = max(1, -(-(last + 1) // s["count"]))
            else:
                W, S = s["window"], s.get("step") or s["window"]
            wins = [dict() for _ in range((0 if last < W else (last - W) // S + 1) + 1)]
            for j, p in zip(range(a, b), ps):
                hv = int(hash_[j])
                for w in range(len(wins)):
                    if w * S <= p < w * S + W and hv <= maxhash:
                        wins[w][hv] = wins[w].get(hv, 0) + 1
        sets += wins
        go.append(len(sets))
    o, v = SO.collection([np.array(sorted(d), U64) for d in sets])
    return np.array(go, U64), o, v, np.array([d[k] for d in sets for k in sorted(d)], U32)


def brute_index(t, cnt):
    sets = [dict(zip(v.tolist(), (np.ones(len(v), I64) if cnt is None else c).tolist())) for v, c in zip(SO.split(t[0], t[1]), SO.split(t[0], t[1] if cnt is None else cnt))]
    distinct = {v for d in sets for v in d}
    bits = max(len(distinct).bit_length() - 1, 0)
    buckets = collections.Counter(int(k) >> (64 - bits) if bits else 0 for k in SR.mix64(np.array(sorted(distinct), U64)))
    return dict(counted=cnt is not None, n_targets=len(sets), n_postings=sum(len(d) for d in sets), n_distinct=len(distinct), max_bucket=max(buckets.values(), default=0),
                sumsq=np.array([min(sum(c * c for c in d.values()), MAX64) for d in sets], U64), totals=np.array([sum(d.values()) for d in sets], U64),
                target_sizes=np.array([len(d) for d in sets], U64))


def brute_search(tsets, qsets, step, weighted):
    """every (query, target) pair intersected as two dicts"""
    offs, tgt, sh, dot, ms = [0], [], [], [], []
    for q in qsets:
        for j, t in enumerate(tsets):
            both = [v for v in q if v in t]
            s = len(both)
            if s >= max(step["min_shared"], 1) and float(s) >= step["min_query_cov"] * float(len(q)) and float(s) >= step["min_target_cov"] * float(len(t)):
                tgt.append(j), sh.append(s)
                dot.append(min(sum(q[v] * t[v] for v in both), MAX64)), ms.append(sum(min(q[v], t[v]) for v in both))
        offs.append(len(tgt))
    out = dict(n_queries=len(qsets), n_hits=len(tgt), offsets=np.array(offs, U64), target=np.array(tgt, U32), shared=np.array(sh, U32), has_total=False, has_members=False,
               has_weights=weighted, total=None, members=None, dot=None, min_sum=None)
    if weighted:
        out.update(dot=np.array(dot, U64), min_sum=np.array(ms, U64))
    return out


def brute_fold(h, go, rule):
    go = [int(x) for x in go]
    o, ot, os_, om = [0], [], [], []
    for q in range(h["n_queries"]):
        acc = collections.OrderedDict()
        for i in range(int(h["offsets"][q]), int(h["offsets"][q + 1])):
            t = int(h["target"][i])
            g = max(k for k in range(len(go) - 1) if go[k] <= t < go[k + 1])
            acc.setdefault(g, [0, set()])
            acc[g][0] += int(h["shared"][i])
            acc[g][1].add(t)
        for g in sorted(acc):
            s, ts = acc[g]
            frac = rule.get("frac")
            if len(ts) >= max(rule.get("min_members", 1), 1) and (frac is None or len(ts) * frac[1] >= frac[0] * (go[g + 1] - go[g])):
                ot.append(g), os_.append(min(s, 0xFFFFFFFF)), om.append(len(ts))
        o.append(len(ot))
    return dict(n_queries=h["n_queries"], n_hits=len(ot), offsets=np.array(o, U64), target=np.array(ot, U32), shared=np.array(os_, U32), members=np.array(om, U32),
                has_members=True, has_total=False, has_weights=False, total=None, dot=None, min_sum=None, n_large_queries=0)


def brute_formulas(h, qa, qb, ta, tb, plain_targets):
    """the weighted formulas hit by hit in Python floats (acos aside, whose last bit may differ between two libraries: compared to 1e-15)"""
    out = {k: [] for k in IP.FORMULAS}
    rows = IP.rows_of(h["offsets"])
    for i, j, d, m in zip(rows.tolist(), h["target"].tolist(), h["dot"].tolist(), h["min_sum"].tolist()):
        den = math.sqrt(float(qa[i])) * math.sqrt(float(qb[j]))
        cos = float("nan") if MAX64 in (d, qa[i], qb[j]) else float(d) / den if den else 0.0
        out["cosine"].append(cos)
        out["angular_similarity"].append(cos if cos != cos else 1.0 - 2.0 * math.acos(min(cos, 1.0)) / math.pi)
        den = float(ta[i]) + float(tb[j]) - float(m)
        out["weighted_jaccard"].append(float(m) / den if den else 0.0)
        den = float(ta[i]) + float(tb[j])
        out["bray_curtis"].append(1.0 - 2.0 * float(m) / den if den else 0.0)
        out["weighted_containment"].append(float("nan") if d == MAX64 else float(d) / float(ta[i]) if ta[i] else 0.0)
    if not plain_targets:
        del out["weighted_containment"]
    return {k: np.array(v, np.float64) for k, v in out.items()}


def norms(t):
    sets = py(t)
    return [min(sum(c * c for c in d.values()), MAX64) for d in sets], [sum(d.values()) for d in sets]


def test_the_model_agrees_with_brute_force():
    """every step of three blocks' programs whose operands hold at most SMALL values (a search: whose pairs walk at most PAIRS_WORK values), and
    the formulas at the end of the hits that small"""
    done = collections.Counter()
    for (prog, recs), seed in [x for b in (0, 3, 6) for x in zip(block(b), IP.seeds(b))]:
        objs, fsets, hits, version, wscale = {}, {}, {}, collections.Counter(), {}
        cores, handles, bound = {}, {}, {}  # index: (targets, counts); handle -> index; hits -> what its formulas are bound to
        tuples = None
        for i, (step, rec) in enumerate(zip(IP.run_concrete(prog)[1], recs)):  # (the steps with their group offsets spelled out)
            k = step["kind"]
            where = IP.message(seed, i, prog, k)
            pool = lambda x: objs[x] if x in objs else fsets[x]  # noqa: E731
            if k == "sketch":
                tuples = IP.standin_tuples(step)
            ids = [step[x] for x in ("a", "b", "q") if step.get(x) is not None]
            small = sum(AP.n_values(pool(x)) for x in ids) <= SMALL
            if k in ("search", "search_counted"):
                t = cores[handles[step["x"]]][0]
                small = small and AP.n_values(t) <= SMALL and AP.n_values(pool(step["q"])) * AP.n_sets(t) <= PAIRS_WORK
            want = None
            if k in ("load", "refused", "close_sets"):
                pass
            elif k == "windows":
                if len(tuples[1]) <= SMALL:
                    go, o, v, c = brute_windows(tuples, step)
                    want = dict(group_offsets=go, offsets=o, values=v, counts=c if step["counted"] else None)
            elif k in GP.SETS_KINDS and small:
                want = brute_sets_step(step, objs, IP.values_of(tuples) if tuples else None)
                if step.get("own_groups"):  # a window object reduced by its own group_offsets: the per-sequence sets of the result
                    o, v = WN.sets_per_sequence(tuples[0], tuples[1], wscale[step["a"]])
                    assert np.array_equal(rec["offsets"], o) and np.array_equal(rec["values"], v), where
                    done["own"] += 1
            elif k == "copy":
                want = dict(offsets=objs[step["a"]][0], values=objs[step["a"]][1], counts=objs[step["a"]][2])
            elif k == "index" and small:
                t = objs[step["a"]]
                want = brute_index(t, t[2] if step["counted"] else None)
            elif k in ("attach", "close_index") and AP.n_values(cores[handles[step["x"]]][0]) <= 8 * SMALL:
                want = brute_index(*cores[handles[step["x"]]])
                if k == "close_index":
                    sib = [x for x, c in handles.items() if c == handles[step["x"]] and x != step["x"]]
                    assert sorted(rec["siblings"]) == sorted(sib) and sib, where
                    want, rec = dict(want), dict(rec["siblings"][sib[0]])
            elif k in ("search", "search_counted") and small:
                t, cnt = cores[handles[step["x"]]]
                want = brute_search(py((t[0], t[1], cnt)), py(pool(step["q"])), step, k == "search_counted")
                holders = collections.Counter(v for d in py((t[0], t[1], None)) for v in d)
                sums = [sum(holders[v] for v in q) for q in py(pool(step["q"]))]
                want["n_large_queries"] = sum(x > SR.SR_CAP for x in sums)
                if k == "search_counted":
                    want["plan_tail"] = SW.plan_tail(np.array(sums, I64), pool(step["q"])[0], want["offsets"])
            elif k == "fold" and hits[step["hits"]]["n_hits"] <= SMALL:
                want = brute_fold(hits[step["hits"]], step["groups"], step["rule"])
                assert rec["figures"][0] == len(step["groups"]) - 1 and rec["figures"][2] == want["n_hits"], where
            elif k in ("top", "hits_load", "neighbors", "neighbors_counted") and small:
                want = dict(brute_graph_step(step, rec, objs, hits), has_members=False, members=None)
            if want is not None:
                assert AP.same(want, {key: rec[key] for key in want}) == [], where
                done[k] += 1
            # the state, from the records
            if "out" in step and k in IP.SETS_KINDS:
                if step.get("into"):
                    version[step["out"]] += 1
                if step.get("keep", True):
                    objs[step["out"]] = (rec["offsets"], rec["values"], rec["counts"])
                    wscale[step["out"]] = step["scale"] if k == "windows" else None
                else:
                    objs.pop(step["out"], None)
                    version[step["out"]] += 1
            elif k == "copy":
                fsets[step["out"]] = objs[step["a"]]
            elif k == "close_sets":
                objs.pop(step["a"], None), fsets.pop(step["a"], None)
                version[step["a"]] += 1
            elif k == "index":
                t = objs[step["a"]]
                cores[step["out"]], handles[step["out"]] = ((t[0], t[1]), t[2] if step["counted"] else None), step["out"]
            elif k == "attach":
                handles[step["out"]] = handles[step["x"]]
            elif k == "close_index":
                del handles[step["x"]]
            elif k in IP.HITS_KINDS:
                hits[step["slot"]] = recs[i]
                bound.pop(step["slot"], None)
                if k == "search_counted":
                    t, cnt = cores[handles[step["x"]]]
                    bound[step["slot"]] = ([(step["q"], pool(step["q"]), version[step["q"]])], (t[0], t[1], cnt), 0, cnt is None, step["x"])
                elif k == "neighbors_counted":
                    bound[step["slot"]] = ([(step[x], objs[step[x]], version[step[x]]) for x in ("a", "b")], None, step["limit"], False, None)
        for slot, h in recs[-1]["hits"].items():  # the late formulas
            if not h["has_weights"]:
                assert h["weighted"] is None
                continue
            sets, ix, limit, plain_targets, handle = bound[slot]
            if any(version[sid] != v for sid, _, v in sets):
                assert h["weighted"] == "stale", (hex(seed), slot)
                done["stale"] += 1
            elif handle is not None and handle not in handles:
                assert h["weighted"] == "closed", (hex(seed), slot)
                done["closed"] += 1
            elif limit:
                assert h["weighted"] == "limit", (hex(seed), slot)
            elif sum(AP.n_values(t) for _, t, _ in sets) + (AP.n_values(ix) if ix else 0) <= SMALL:
                (qa, ta), (qb, tb) = norms(sets[0][1]), norms(ix if ix else sets[1][1])
                for name, want in brute_formulas(h, qa, qb, ta, tb, plain_targets).items():
                    got = h["weighted"][name].view(np.float64)
                    ok = np.allclose(got, want, rtol=0, atol=1e-15, equal_nan=True) if name == "angular_similarity" else np.array_equal(got, want, equal_nan=True)
                    assert ok, (hex(seed), slot, name)
                assert plain_targets or h["weighted"]["weighted_containment"] == "undefined"
                done["formulas"] += 1
    print(dict(done))
    for k in ("windows", "own", "index", "attach", "close_index", "search", "search_counted", "fold", "top", "copy", "neighbors_counted", "formulas", "stale"):
        assert done[k] >= 3, (k, done)


# ---- what the campaign reaches ----
def test_what_the_campaign_reaches():
    f = IP.figures(campaign())
    print("%d programs, %d calls after the sources, %d checked objects" % (len(campaign()), f["steps"], f["checked"]))
    print({k: v for k, v in f.items() if not isinstance(v, set)})
    assert f["chunk_calls"] >= 20, f["chunk_calls"]                      # search_counted calls in which k_sw_chunk ran
    assert f["row_calls"] >= 20, f["row_calls"]                          # ... in which k_sw_row ran
    assert f["large"] >= 10, f["large"]                                  # searches with n_large_queries > 0
    assert f["stale_queries"] >= 15, f["stale_queries"]                  # search_counted whose queries have stale counts
    assert f["stale_builds"] >= 15, f["stale_builds"]                    # index_counted built from stale-counts sets
    assert f["source_gone"] >= 20, f["source_gone"]                      # searches of an index whose source was overwritten or closed before
    assert f["attached"] >= 20, f["attached"]                            # searches through an attached handle on the other engine
    assert f["attached_first_closed"] >= 8, f["attached_first_closed"]   # ... of those, after the first handle was closed
    assert f["window_folds"] >= 20, f["window_folds"]                    # folds by a window object's group_offsets of hits against its index
    assert f["weighted_folds"] >= 10, f["weighted_folds"]                # folds of weighted hits
    assert f["folded_tops"] >= 10, f["folded_tops"]                      # top of folded hits
    assert len(f["transitions"]) == 12 and min(f["transitions"].values()) >= 3, f["transitions"]  # none / totals / weights / members on a re-used object
    assert set(f["refusals"]) == set(IP.REFUSALS) and min(f["refusals"].values()) >= 5, f["refusals"]
    assert f["late_formulas"] >= 20, f["late_formulas"]                  # weighted hits whose formulas are asked after an operand was written or closed
    assert f["covers"] >= 25, f["covers"]                                # search steps with a non-zero cover
    assert f["closed_formulas"] >= 3, f["closed_formulas"]                # ... after the handle of the search was closed
    assert f["asked_formulas"] >= 20 and f["own_reduces"] >= 5 and f["most_sets"] >= 300, f  # and: formulas that do answer, window objects reduced, of several hundred sets
    assert f["window_algebra"] >= 10, f["window_algebra"]                # set algebra with a window object as an operand
    assert f["kinds"] >= (set(IP.KINDS) - {"window_algebra"}) | {"refused", "load", "sketch"} and len(f["rules"]) == 4 and len(f["windows"]) == len(IP.WINDOWS), f
    for prog, recs in campaign():  # AP's and GP's work budgets
        assert sum(r.get("n_values", 0) for r in recs[:-1]) <= 3 * AP.VALUE_BUDGET
        for s, r in zip(prog, recs):
            if s["kind"] in ("neighbors", "neighbors_counted"):
                assert r["n_queries"] * len(r["operands"][s["b"]][0]) <= 41 * 41


# ---- the campaign sees the mistakes these entries can make ----
@pytest.mark.parametrize("sabotage", IP.SABOTAGES, ids=[s.name.split()[0] for s in IP.SABOTAGES])
def test_every_sabotaged_model_is_caught(sabotage):
    """programs of the campaign at which AP.same tells the sabotaged model from the true one"""
    caught = [seed for b in range(IP.BLOCKS) for seed, (prog, recs) in zip(IP.seeds(b), block(b))
              if (sabotage.kinds == ("end",) or any(s["kind"] in sabotage.kinds for s in prog)) and IP.first_difference(prog, recs, sabotage()) is not None]
    print("%s: caught by %d programs of %d" % (sabotage.name, len(caught), IP.BLOCKS * IP.PER_BLOCK))
    assert len(caught) >= 2, sabotage.name
