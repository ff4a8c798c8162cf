"""CPU: what tests/graph_programs.py claims about the campaign tests/test_gpu_graph_fuzz.py runs -- 8 blocks of 20 seeded programs over
the compare, hits and clusters objects, beside the 12 blocks of tests/algebra_programs.py, which stay what they were (pinned below).

The generator is deterministic; its model agrees with brute force (neighbor_cases.walk_neighbors, a Counter walk in Python integers for
the weights, a union-find and a sequential greedy loop written here); every block and the whole campaign reach the states the fuzz
exists for -- the conditions below keep the campaign from hiding a failure: when a block misses one, the generator's weights change, not
the condition, and the ones marked (!) are why this campaign exists --; and every sabotaged model of GP.SABOTAGES is caught by the same
comparison (AP.same) the GPU test uses."""
import collections
import functools
import zlib

import numpy as np
import pytest

from tests import algebra_programs as AP
from tests import cluster_cases as CL
from tests import graph_programs as GP
from tests import neighbor_cases as NC
from tests import setops_cases as SO
from tests.test_algebra_programs import as_sets, brute_step as brute_sets_step
from tests.test_compare_cases import brute as brute_compare
from tests.test_search_cases import _brute as brute_search

U64, U32 = np.uint64, np.uint32
MAX64 = (1 << 64) - 1
NEW_KINDS = ("compare", "compare_counted", "neighbors", "neighbors_counted", "search", "top", "hits_load", "cluster")
OLD_CAMPAIGN_CRC = 0x85BE8B09  # of AP.describe(AP.program(seed)) over AP's 240 seeds, taken before this campaign was written


@functools.lru_cache(None)
def block(b):
    """the programs of a block with the model's records"""
    return [GP.program_and_records(seed) for seed in GP.seeds(b)]


@functools.lru_cache(None)
def campaign():
    return [pr for b in range(GP.BLOCKS) for pr in block(b)]


# ---- the generator ----
def test_the_old_campaign_is_what_it_was():
    crc = 0
    for b in range(AP.BLOCKS):
        for seed in AP.seeds(b):
            crc = zlib.crc32(AP.describe(AP.program(seed)).encode(), crc)
    assert AP.BLOCKS * AP.PER_BLOCK == 240 and crc == OLD_CAMPAIGN_CRC, "%08x" % crc


def test_the_campaign_is_160_seeds_and_a_program_is_its_seed():
    all_seeds = [s for b in range(GP.BLOCKS) for s in GP.seeds(b)]
    assert all_seeds == list(range(GP.BASE, GP.BASE + 160)) and not set(all_seeds) & set(range(AP.BASE, AP.BASE + 240))
    for seed in GP.seeds(0)[:5] + GP.seeds(6)[:5]:
        one, two = GP.program(seed), GP.program(seed)
        assert GP.describe(one) == GP.describe(two) and len(one) == len(two)
        assert GP.describe(one) != GP.describe(GP.program(seed + 1))
        steps = [s for s in one if s["kind"] not in ("load", "sketch")]
        assert 10 <= len(steps) <= 16 and len(one) - len(steps) == 4
        sources = [s["counted"] if s["kind"] == "sketch" else s["counts"] is not None for s in one[:4]]
        assert any(sources) and not all(sources), sources
    assert "python -m tests.graph_programs" in GP.message(GP.BASE, 5, GP.program(GP.BASE), ["x"])
    assert len(GP.SABOTAGES) >= 12 and set(GP.NS) >= {17, 33, 40}


def test_the_generator_s_records_are_run_model_s():
    for prog, recs in block(1)[:8]:
        again = GP.run_model(prog)
        assert len(again) == len(recs) == len(prog) + 1
        for i, (x, y) in enumerate(zip(recs, again)):
            assert AP.same(x, y) == [], i
        assert GP.first_difference(prog, recs, GP.Model()) is None


# ---- the model against brute force ----
def counters(t):
    c = np.ones(len(t[1]), U32) if t[2] is None else t[2]
    return [collections.Counter({int(v): int(n) for v, n in zip(s, cs)}) for s, cs in zip(SO.split(t[0], t[1]), SO.split(t[0], c))]


def brute_weights(x, y, limit):
    """(dot, min_sum) of two Counters: over the first `limit` keys of their union (0: all) that both hold"""
    walked = sorted(set(x) | set(y))
    walked = walked[:limit] if limit else walked
    both = [v for v in walked if v in x and v in y]
    return min(sum(x[v] * y[v] for v in both), MAX64), sum(min(x[v], y[v]) for v in both)


def union_find(n, edges):
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v

    for u, v in edges:
        parent[find(u)] = find(v)
    return [find(v) for v in range(n)]


def brute_cluster(h, method, score):
    """-> (the representative of every node, the clusters as sets) by a plain union-find / the sequential greedy loop"""
    n = h["n_queries"]
    o, t = [int(x) for x in h["offsets"]], [int(x) for x in h["target"]]
    edges = {(min(i, j), max(i, j)) for i in range(n) for j in t[o[i]:o[i + 1]] if i != j}
    better = (lambda v: v) if score is None else (lambda v: (-int(score[v]), v))  # the smaller, the better
    if method == "components":
        root = union_find(n, edges)
        rep = [min((u for u in range(n) if root[u] == root[v]), key=better) for v in range(n)]
    else:
        rep, reps = [None] * n, set()
        for v in sorted(range(n), key=better):
            near = [u for u in reps if (min(u, v), max(u, v)) in edges]
            rep[v] = min(near, key=better) if near else v
            if not near:
                reps.add(v)
    return rep


def brute_step(step, rec, objs, hits):
    """what a step of a new kind yields, by brute force -> the record's fields it can speak about"""
    k = step["kind"]
    if k in ("compare", "compare_counted", "neighbors", "neighbors_counted"):
        a, b = objs[step["a"]], objs[step["b"]]
        A, B = SO.split(a[0], a[1]), SO.split(b[0], b[1])
        if k in GP.CMP_ENTRY:
            sh, tt = brute_compare(A, B, step["limit"])
            out = dict(shared=sh, total=tt, weighted=k == "compare_counted", dot=None, min_sum=None)
            if k == "compare_counted":
                w = [[brute_weights(x, y, step["limit"]) for y in counters(b)] for x in counters(a)]
                out.update(dot=np.array([[c[0] for c in row] for row in w], U64).reshape(sh.shape), min_sum=np.array([[c[1] for c in row] for row in w], U64).reshape(sh.shape))
            return out
        o, t, s, tot = NC.walk_neighbors(A, B, step["limit"], **GP.rule_of(step))
        out = dict(n_queries=len(A), n_hits=len(t), offsets=o, target=t, shared=s, has_total=True, total=tot, has_weights=k == "neighbors_counted", dot=None, min_sum=None)
        if k == "neighbors_counted":
            ca, cb = counters(a), counters(b)
            rows = np.repeat(np.arange(len(A)), np.diff(o).astype(np.int64))
            w = [brute_weights(ca[i], cb[int(j)], step["limit"]) for i, j in zip(rows, t)]
            out.update(dot=np.array([c[0] for c in w], U64), min_sum=np.array([c[1] for c in w], U64))
        return out
    if k == "search":
        o, t, s = brute_search(as_sets(objs[step["a"]]), as_sets(objs[step["q"]]), step["min_shared"], 0.0, 0.0)
        return dict(offsets=o, target=t, shared=s, has_total=False, has_weights=False, total=None, dot=None, min_sum=None)
    if k == "top":
        h = hits[step["hits"]]
        o, t, s = [int(x) for x in h["offsets"]], h["target"], h["shared"]
        best = [sorted(zip(t[o[q]:o[q + 1]], s[o[q]:o[q + 1]]), key=lambda x: (-int(x[1]), int(x[0])))[:step["n"]] for q in range(len(o) - 1)]
        return dict(n_queries=h["n_queries"], offsets=np.concatenate([[0], np.cumsum([len(x) for x in best])]).astype(U64), target=np.array([x[0] for r in best for x in r], U32),
                    shared=np.array([x[1] for r in best for x in r], U32), has_total=False, has_weights=False, total=None, dot=None, min_sum=None)
    if k == "hits_load":
        return dict(n_queries=step["n"], n_hits=len(step["target"]), offsets=step["offsets"], target=step["target"], shared=step["shared"], has_total=step["total"] is not None,
                    total=step["total"], has_weights=False)
    assert k == "cluster", k
    h = hits[step["hits"]]
    rep_of = brute_cluster(h, step["method"], step["score"])
    reps = sorted(set(rep_of))
    members = [[v for v in range(len(rep_of)) if rep_of[v] == r] for r in reps]
    lay, rounds = CL.ROUND_MODELS[step["method"]](h["n_queries"], h["offsets"], h["target"], step["score"])
    assert CL.same(lay, (rec["label"], rec["rep"], rec["offsets"], rec["members"], rec["largest"])), "the round scheme and the definition disagree"
    assert rec["figures"] == (rounds, len([1 for i in range(h["n_queries"]) for j in h["target"][int(h["offsets"][i]):int(h["offsets"][i + 1])] if int(j) != i]))
    return dict(n_items=len(rep_of), n_clusters=len(reps), largest=max(len(m) for m in members), rep=np.array(reps, U32), label=np.array([reps.index(r) for r in rep_of], U32),
                members=np.array([v for m in members for v in m], U32), offsets=np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(U64))


@pytest.mark.parametrize("b", [0, 3, 7])
def test_the_model_agrees_with_brute_force(b):
    """every step of the block's programs whose operands hold at most 4 000 values"""
    done = collections.Counter()
    for (prog, recs), seed in zip(block(b), GP.seeds(b)):
        objs, hits, values = {}, {}, None
        for i, (step, rec) in enumerate(zip(prog, recs)):
            k = step["kind"]
            if k == "sketch":
                values = AP.standin_values(step)
            ids = [step[x] for x in ("a", "b", "q") if step.get(x) is not None]
            if k not in ("load", "refused") and sum(AP.n_values(objs[x]) for x in ids) <= 4000:
                want = brute_step(step, rec, objs, hits) if k in NEW_KINDS else brute_sets_step(step, objs, values)
                if k in GP.SETS_KINDS:
                    want["sumsq"] = np.array([min(sum(n * n for n in c.values()), MAX64) for c in counters((rec["offsets"], rec["values"], rec["counts"]))], U64)
                assert AP.same(want, {key: rec[key] for key in want}) == [], GP.message(seed, i, prog, k)
                done[k] += 1
            if "out" in step:
                objs[step["out"]] = (rec["offsets"], rec["values"], rec["counts"])
            if k in GP.HITS_ENTRY:
                hits[step["slot"]] = rec
    assert all(done[k] >= 5 for k in NEW_KINDS), done


# ---- what the campaign reaches ----
@pytest.mark.parametrize("b", range(GP.BLOCKS))
def test_what_a_block_reaches(b):
    f = GP.figures(block(b))
    assert f["entries"] == set(GP.ENTRIES), set(GP.ENTRIES) ^ f["entries"]
    assert 4 * f["no_pair"] <= f["neighbour_steps"], ("neighbour steps that keep no pair", f["no_pair"], f["neighbour_steps"])
    assert f["into_other"] >= 5, ("neighbour or search steps into hits another entry made", f["into_other"])
    assert min(f["totals_to_none"], f["weights_to_none"], f["none_to_weights"]) >= 2, f   # (!) the payload flags of a re-used bsk_hits
    assert min(f["weighted_to_plain"], f["plain_to_weighted"]) >= 2, f                    # (!) the weighted flag of a re-used bsk_compare
    assert f["stale_weighted"] >= 3, f                                                    # (!) weighted kernels on operands with stale counts
    assert f["top_clusters"] >= 3, f                                                      # (!) clusters of a one-directional k-nearest graph
    assert f["search_clusters"] >= 1 and f["skipping"] >= 2, f
    for prog, recs in block(b):
        cells = max([r["n_a"] * r["n_b"] for r in recs[:-1] if "n_a" in r], default=0)
        assert sum(r.get("n_values", 0) for r in recs[:-1]) <= 2 * AP.VALUE_BUDGET and cells <= 1600, cells


def test_what_the_campaign_reaches():
    f = GP.figures(campaign())
    print("%d programs, %d calls after the sources, %d checked objects" % (len(campaign()), f["steps"], f["checked"]))
    print({k: v for k, v in f.items() if not isinstance(v, set)})
    assert f["jaccards"] == set(GP.MIN_JACCARD) and f["sizes"] >= set(CL.SIZES) and f["methods"] == set(CL.METHODS), f
    assert f["score_kinds"] == set(GP.SCORE_KINDS) and f["refusals"] == set(GP.REFUSALS), f
    assert f["saturated_dot"] >= 1 and f["saturated_sumsq"] >= 1 and f["cut_unions"] >= 1 and f["methods_differ"] >= 1 and f["long_greedy"] >= 1, f


# ---- the campaign sees the mistakes these entries can make ----
@pytest.mark.parametrize("sabotage", GP.SABOTAGES, ids=[s.name.split()[0] for s in GP.SABOTAGES])
def test_every_sabotaged_model_is_caught(sabotage):
    """programs of the campaign at which AP.same tells the sabotaged model from the true one"""
    caught = [seed for b in range(GP.BLOCKS) for seed, (prog, recs) in zip(GP.seeds(b), block(b))
              if any(s["kind"] in sabotage.kinds for s in prog) and GP.first_difference(prog, recs, sabotage()) is not None]
    print("%s: caught by %d programs of %d" % (sabotage.name, len(caught), GP.BLOCKS * GP.PER_BLOCK))
    assert caught, sabotage.name
