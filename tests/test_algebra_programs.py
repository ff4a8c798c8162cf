"""CPU: what tests/algebra_programs.py claims about the campaign tests/test_gpu_algebra_fuzz.py runs -- 12 blocks of 20 seeded programs.

The generator is deterministic; its model agrees with brute-force Python sets and Counters (the ones of test_compare_cases.py,
test_search_cases.py and test_counts_cases.py, and their like for the algebra); every block and the whole campaign reach the states
the fuzz exists for (the thresholds below are caps that keep the campaign from hiding a failure: when a block misses one, the
generator's weights change, not the threshold); and every sabotaged model of AP.SABOTAGES -- one small wrong variant of a reference,
named after the kernel mistake it stands for -- is caught by the same comparison (AP.same) the GPU test uses."""
import collections
import functools

import numpy as np
import pytest

from tests import algebra_programs as AP
from tests import counts_cases as CN
from tests import setops_cases as SO
from tests.test_compare_cases import brute as brute_compare
from tests.test_counts_cases import plain_count
from tests.test_search_cases import _brute as brute_search

U64, U32 = np.uint64, np.uint32


@functools.lru_cache(None)
def block(b):
    """the programs of a block with the model's records"""
    return [AP.program_and_records(seed) for seed in AP.seeds(b)]


@functools.lru_cache(None)
def campaign():
    return [pr for b in range(AP.BLOCKS) for pr in block(b)]


# ---- the generator ----
def test_the_campaign_is_240_seeds_and_a_program_is_its_seed():
    all_seeds = [s for b in range(AP.BLOCKS) for s in AP.seeds(b)]
    assert all_seeds == list(range(AP.BASE, AP.BASE + 240))
    for seed in AP.seeds(0)[:5] + AP.seeds(7)[:5]:
        one, two = AP.program(seed), AP.program(seed)
        assert AP.describe(one) == AP.describe(two) and len(one) == len(two)
        assert AP.describe(one) != AP.describe(AP.program(seed + 1))
        steps = [s for s in one if s["kind"] not in ("load", "sketch")]
        assert 8 <= len(steps) <= 14 and len(one) - len(steps) == 4
    assert "python -m tests.algebra_programs" in AP.message(AP.BASE, 5, AP.program(AP.BASE), ["x"])


def test_size_classes_sit_on_the_thresholds_read_from_the_sources():
    c = AP.size_classes()
    assert c == [(0, 0), (1, 20), (25, 40), (60, 70), (120, 136), (500, 530), (1000, 1100), (2040, 2060)]
    assert c[3][0] < AP.CAPS["SO_GROUP_CAP"] < c[3][1] and c[4][0] < AP.CMP["CMP_WINDOW"] < c[4][1]
    assert c[6][0] < AP.CAPS["SO_WAVE_CAP"] == AP.CAPS["SO_TILE"] < c[6][1] and c[7][0] < AP.CNT_CHUNK == AP.CAPS["RD_CHUNK"] < c[7][1]
    assert set(AP.NS) >= {AP.CMP["CMP_ROWS"], AP.CMP["CMP_ROWS"] + 1, 2 * AP.CMP["CMP_COLS"] + 1}


def test_the_generator_s_records_are_run_model_s():
    for prog, recs in block(2)[:8]:
        again = AP.run_model(prog)
        assert len(again) == len(recs) == len(prog) + 1
        for i, (x, y) in enumerate(zip(recs, again)):
            assert AP.same(x, y) == [], i
        assert AP.first_difference(prog, recs, AP.Model()) is None


def test_same_reports_what_differs():
    a = dict(n=3, v=np.array([1, 2, 3], U64), c=None, sub={"x": (np.zeros(2, U32), np.ones((2, 2), U32))})
    b = dict(n=3, v=np.array([1, 2, 3], U64), c=None, sub={"x": (np.zeros(2, U32), np.ones((2, 2), U32))})
    assert AP.same(a, b) == []
    for change in (dict(n=4), dict(v=np.array([1, 2, 4], U64)), dict(v=np.array([1, 2, 3], np.int64)), dict(v=np.array([1, 2], U64)), dict(c=np.zeros(0, U32)),
                   dict(sub={"x": (np.zeros(2, U32), np.eye(2, dtype=U32))}), dict(sub={"y": 1})):
        assert len(AP.same(a, {**b, **change})) == 1, change
    assert len(AP.same(a, {k: v for k, v in b.items() if k != "c"})) == 1


# ---- the model against brute force ----
def as_sets(t):
    return [set(int(v) for v in s) for s in SO.split(t[0], t[1])]


def as_counters(t):
    c = CN.ones(t[0]) if t[2] is None else t[2]
    return [collections.Counter({int(v): int(n) for v, n in zip(s, cs)}) for s, cs in zip(SO.split(t[0], t[1]), SO.split(t[0], c))]


def from_sets(sets):
    o, v = SO.collection([np.array(sorted(s), U64) for s in sets])
    return o, v, None


def from_counters(cs):
    o, v = SO.collection([np.array(sorted(c), U64) for c in cs])
    return o, v, np.array([c[k] for c in cs for k in sorted(c)], U32)


def paired(x, y):
    return zip(x * (len(y) if len(x) == 1 else 1), y * (len(x) if len(y) == 1 else 1)) if len(x) != len(y) else zip(x, y)


def brute_step(step, objs, values):
    """what a step yields, by Python sets and Counters -> the record's fields it can speak about"""
    k = step["kind"]
    if k in ("sketch", "result_sets"):
        o, v, c = plain_count(values, step["scale"], step["whole"])
        return dict(offsets=o, values=v, counts=c if step["counted"] else None)
    a = objs[step["a"]]
    if k == "op":
        f = {SO.UNION: set.union, SO.INTERSECT: set.intersection, SO.DIFF: set.difference, SO.SYMDIFF: set.symmetric_difference}[step["op"]]
        o, v, c = from_sets([f(x, y) for x, y in paired(as_sets(a), as_sets(objs[step["b"]]))])
    elif k == "op_counted":
        out = []
        for x, y in paired(as_counters(a), as_counters(objs[step["b"]])):
            if step["op"] == CN.ADD:
                out.append(collections.Counter({v: min(x[v] + y[v], AP.SAT) for v in set(x) | set(y)}))
            else:
                out.append(collections.Counter({v: n for v, n in x.items() if (v in y) == (step["op"] == CN.KEEP)}))
        o, v, c = from_counters(out)
    elif k == "reduce":
        sets, go, out = as_sets(a), [int(g) for g in step["groups"]], []
        for g in range(len(go) - 1):
            members = sets[go[g]:go[g + 1]]
            held = collections.Counter(v for m in members for v in m)
            need = len(members) if step["m"] == AP.MEMBERS_ALL else step["m"]
            out.append({v for v, n in held.items() if n >= need and members})
        o, v, c = from_sets(out)
    elif k == "filter":
        hi = AP.SAT if step["hi"] is None else step["hi"]
        o, v, c = from_counters([collections.Counter({v: n for v, n in x.items() if step["lo"] <= n <= hi}) for x in as_counters(a)])
    elif k == "bottom":
        cut = [collections.Counter({v: x[v] for v in sorted(x)[:step["n"]]}) for x in as_counters(a)]
        o, v, c = from_counters(cut)
        c = c if a[2] is not None else None
    elif k == "compare":
        sh, tt = brute_compare(SO.split(a[0], a[1]), SO.split(*objs[step["b"]][:2]), step["limit"])
        return dict(shared=sh, total=tt)
    else:
        assert k == "search", k
        o, t, s = brute_search(as_sets(a), as_sets(objs[step["q"]]), step["min_shared"], 0.0, 0.0)
        out = dict(offsets=o, targets=t, shared=s)
        if step["top"]:
            best = [sorted(zip(t[int(o[q]):int(o[q + 1])], s[int(o[q]):int(o[q + 1])]), key=lambda h: (-int(h[1]), int(h[0])))[:step["top"]] for q in range(len(o) - 1)]
            out.update(top_offsets=np.concatenate([[0], np.cumsum([len(x) for x in best])]).astype(U64),
                       top_targets=np.array([h[0] for x in best for h in x], np.uint32), top_shared=np.array([h[1] for x in best for h in x], np.uint32))
        return out
    return dict(offsets=o, values=v, counts=c, n_values=len(v), counted=c is not None)


@pytest.mark.parametrize("b", [0, 5, 11])
def test_the_model_agrees_with_brute_force(b):
    """every step of the block's programs whose operands hold at most 4 000 values: Python sets and Counters, not NumPy's set routines"""
    done = collections.Counter()
    for prog, recs in block(b):
        objs, values = {}, None
        for step, rec in zip(prog, recs):
            if step["kind"] == "sketch":
                values = AP.standin_values(step)
            ids = [step[x] for x in ("a", "b", "q") if step.get(x) is not None]
            if step["kind"] not in ("load", "refused") and sum(AP.n_values(objs[i]) for i in ids) <= 4000:
                want = brute_step(step, objs, values)
                assert AP.same(want, {key: rec[key] for key in want}) == [], AP.message(AP.BASE, prog.index(step), prog, step["kind"])
                done[step["kind"]] += 1
            if "out" in step:
                objs[step["out"]] = (rec["offsets"], rec["values"], rec["counts"])
    assert all(done[k] >= 5 for k in ("op", "op_counted", "reduce", "filter", "bottom", "compare", "search")), done


# ---- what the campaign reaches ----
@pytest.mark.parametrize("b", range(AP.BLOCKS))
def test_what_a_block_reaches(b):
    f = AP.figures(block(b))
    assert 4 * f["empty"] <= f["checked"], ("results without values", f["empty"], f["checked"])
    assert min(f["paths"]) >= 50, ("pairs on k_so_group, k_so_wave, k_so_tile", f["paths"])
    assert f["multi_round"] >= 1 and f["filters"] >= 3 and f["strict_reduces"] >= 3 and f["into_other"] >= 5 and f["refused"] >= 1, f
    for prog, recs in block(b):
        made = sum(r.get("n_values", 0) for r in recs[:-1])
        cells = max([r["n_a"] * r["n_b"] for r in recs[:-1] if "n_a" in r], default=0)
        assert made <= 2 * AP.VALUE_BUDGET and cells <= 1600, (made, cells)


def test_what_the_campaign_reaches():
    f = AP.figures(campaign())
    assert f["entries"] == set(AP.ENTRIES), set(AP.ENTRIES) ^ f["entries"]
    assert f["bottoms"] == set(AP.BOTTOM_NS) and f["limits"] == set(AP.LIMITS) and f["classes"] >= set(range(len(AP.size_classes())))
    assert f["refusals"] == set(AP.REFUSALS)
    assert f["saturated"] >= 1 and f["big_totals"] >= 1 and f["a_broadcast"] >= 1 and f["multi_round"] >= 30, f


# ---- the campaign sees the mistakes these kernels can make ----
@pytest.mark.parametrize("sabotage", AP.SABOTAGES, ids=[s.name.split()[0] for s in AP.SABOTAGES])
def test_every_sabotaged_model_is_caught(sabotage):
    """programs of the campaign at which AP.same tells the sabotaged model from the true one (in their order 52, 33, 158, 65, 64, 48, 46, 16, 11, 162 and 32 of the 240)"""
    caught = [seed for b in range(AP.BLOCKS) for seed, (prog, recs) in zip(AP.seeds(b), block(b))
              if any(s["kind"] in sabotage.kinds for s in prog) and AP.first_difference(prog, recs, sabotage()) is not None]
    print("%s: caught by %d programs of %d" % (sabotage.name, len(caught), AP.BLOCKS * AP.PER_BLOCK))
    assert caught, sabotage.name
