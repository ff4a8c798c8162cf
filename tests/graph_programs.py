"""Seeded programs over the compare, neighbour, hits and cluster objects of the sets side (compare.hip, search.hip, cluster.hip) and
their NumPy interpreter: the second campaign, beside tests/algebra_programs.py (AP), whose programs and records it leaves as they are.

program(seed) starts as an AP program does -- four sources, at least one counted and one uncounted -- and then chains 10 to 16 calls.
The sets-making calls are AP's own (op, op_counted, reduce, filter, bottom, result_sets: they make the operands, and the objects whose
counts array is STALE: counted once, last written by an uncounted entry).  The new calls write into objects that other entries made:
  compare / compare_counted     into one pool of bsk_compare objects (the `weighted` flag follows the last writer);
  neighbors / neighbors_counted / search / top / hits_load
                                into one pool of bsk_hits objects (`has_total` and `has_weights` follow the last writer, the five
                                arrays only grow, so the first room of the next neighbours call depends on the object's history);
  cluster                       of any live hits whose targets are all below n_queries -- symmetric neighbour results, the one-directional
                                k-nearest graph of a top(n), a square search result, a host graph -- into a pool of bsk_clusters;
  refused                       calls the library must refuse with BSK_ERR_ARG, the slot and every operand left as they were.
Every sets record carries `sumsq` (bsk_sets_sumsq) beside AP's fields.  run_model(program) gives what every step must yield, with the
references the entries' own suites use (compare_cases.ref_compare / plan_figures, compare_counted_cases.ref_compare / ref_sumsq,
neighbor_cases.filter_matrices / expected_tiles, neighbor_counted_cases.filter_weighted, search_cases.ref_search / ref_top,
cluster_cases.MODELS / ROUND_MODELS / n_offdiagonal); AP.same is the one comparison, used by tests/test_gpu_graph_fuzz.py on the
device's records and by tests/test_graph_programs.py on the records of the SABOTAGES.  Nothing here imports the engine.

    python -m tests.graph_programs SEED      prints the program of that seed, call by call"""
import math
import sys

import numpy as np

from tests import algebra_programs as AP
from tests import cluster_cases as CL
from tests import compare_cases as CC
from tests import compare_counted_cases as WC
from tests import neighbor_cases as NC
from tests import neighbor_counted_cases as NW
from tests import setops_cases as SO

U64, U32 = np.uint64, np.uint32
MAX64, CMP = WC.MAX, AP.CMP

BASE, BLOCKS, PER_BLOCK = 0x6A9F0000, 8, 20
NS, LIMITS = AP.NS, AP.LIMITS
MIN_SHARED = (1, 2, 5)
MIN_JACCARD = (None, (1, 2), (1, 1), (3, 10), 0.25)
JACCARD_WEIGHTS = (0.35, 0.15, 0.08, 0.20, 0.22)
TOP_NS = (1, 3)
SCORE_KINDS = ("none", "scores", "equal")
SCORE_NAMES = ("random", "few", "extremes", "descending")  # of cluster_cases.scores
GRAPHS = ("multigraph", "path", "star")
ENTRIES = ("bsk_sets_compare", "bsk_sets_compare_counted", "bsk_sets_sumsq", "bsk_sets_neighbors", "bsk_sets_neighbors_counted", "bsk_index_search",
           "bsk_hits_top", "bsk_hits_from_host", "bsk_hits_cluster", "bsk_hits_fetch_totals", "bsk_hits_fetch_weights", "bsk_compare_fetch_weights",
           "bsk_clusters_fetch")
REFUSALS = ("cluster of rectangular hits", "fetch_weights of hits without weights", "fetch_totals of hits without totals",
            "fetch_weights of an unweighted compare", "neighbors with jaccard_num > jaccard_den", "neighbors with an unknown flag bit",
            "hits of the other engine in the slot", "clusters of the other engine in the slot", "hits_from_host with a row not strictly ascending",
            "top into its own input")
COMPARE_WORK = AP.COMPARE_WORK  # the values the pairs of one plain compare walk together, as in AP
WEIGHTED_WORK = 60_000          # ... of a weighted or a neighbours call (their references walk in Python integers)
SETS_KINDS = ("load", "sketch", "result_sets", "op", "op_counted", "reduce", "filter", "bottom")
HITS_ENTRY = dict(neighbors="bsk_sets_neighbors", neighbors_counted="bsk_sets_neighbors_counted", search="bsk_index_search", top="bsk_hits_top",
                  hits_load="bsk_hits_from_host")
CMP_ENTRY = dict(compare="bsk_sets_compare", compare_counted="bsk_sets_compare_counted")


def seeds(block):
    return [BASE + PER_BLOCK * block + i for i in range(PER_BLOCK)]


def rule_of(step):
    """min_shared, min_jaccard and upper of a neighbours step -> the keyword arguments of neighbor_cases.keeps; a float goes the way of
    Sets._neighbors: (ceil(x * 2^30), 2^30)"""
    j = step["min_jaccard"]
    num, den = (0, 0) if j is None else j if isinstance(j, tuple) else (int(math.ceil(float(j) * (1 << 30))), 1 << 30)
    return dict(min_shared=step["min_shared"], num=num, den=den, upper=step["upper"])


# ---- the references behind the model, computed once per operands ----
_plain, _weighted = {}, {}


def _key(t, c):
    return (AP.digest(t[0], t[1], c), len(t[0]), len(t[1]), c is None)


def plain_compare(a, b, limit):
    key = (_key(a, None), _key(b, None), limit)
    if key not in _plain:
        _plain[key] = CC.ref_compare(SO.split(a[0], a[1]), SO.split(b[0], b[1]), limit)
    return _plain[key]


def weighted_compare(a, ca, b, cb, limit):
    """compare_counted_cases.ref_compare of (a with the counts ca) and (b with cb); None: every count 1.  Under a limit every set is cut
    to its first `limit` values first: the first `limit` values of a union lie in the first `limit` of both sets."""
    key = (_key(a, ca), _key(b, cb), limit)
    if key not in _weighted:
        cut = (lambda xs: [x[:limit] for x in xs]) if limit else (lambda xs: xs)
        A, B = cut(SO.split(a[0], a[1])), cut(SO.split(b[0], b[1]))
        CA = None if ca is None else cut(SO.split(a[0], ca))
        CB = None if cb is None else cut(SO.split(b[0], cb))
        _weighted[key] = WC.ref_compare(A, CA, B, CB, limit)
    return _weighted[key]


def sumsq_of(t):
    """bsk_sets_sumsq: compare_counted_cases.ref_sumsq of the counts; the sizes for sets without counts"""
    if t[2] is None:
        return np.diff(t[0]).astype(U64)
    return WC.ref_sumsq(SO.split(t[0], t[2]))


def hits_of(n_queries, offsets, target, shared, total=None, dot=None, min_sum=None):
    """everything the device can be asked about a bsk_hits"""
    return dict(n_queries=int(n_queries), n_hits=int(offsets[-1]), offsets=offsets, target=target, shared=shared, has_total=total is not None,
                has_weights=dot is not None, total=total, dot=dot, min_sum=min_sum)


def clusters_of(lay):
    label, rep, offsets, members, largest = lay
    return dict(n_items=len(label), n_clusters=len(rep), largest=int(largest), label=label, rep=rep, offsets=offsets, members=members)


def square(h):
    """whether bsk_hits_cluster takes these hits: every target below n_queries"""
    return h["n_hits"] == 0 or int(h["target"].max()) < h["n_queries"]


def symmetric(h):
    e = set(CL.edge_list(h["offsets"], h["target"], directed=True))
    return all((j, i) in e for i, j in e)


# ---- the model: one method per thing a kernel decides; a sabotage overrides one ----
class Model(AP.Model):
    name = "the references"
    kinds = ()

    def sumsq(self, t):
        return sumsq_of(t)

    def counts_read(self, t, stale):
        """the counts a weighted kernel reads of an operand (stale: what its counts array still holds when the object is uncounted)"""
        return t[2]

    def weights(self, a, ca, b, cb, limit):
        """-> shared, total, dot, min_sum [n_a, n_b]"""
        return weighted_compare(a, ca, b, cb, limit)

    def kept(self, sh, tt, dt, ms, rule):
        """the cells the rule keeps -> (offsets, target, shared, total, dot, min_sum); the last two None without weights"""
        if dt is None:
            return NC.filter_matrices(sh, tt, **rule) + (None, None)
        return NW.filter_weighted(sh, tt, dt, ms, **rule)

    def hits_after(self, before, new, kind):
        """the hits object after the entry of a `kind` step wrote `new` into it (before: what it held, None for a new object)"""
        return new

    def cmp_after(self, before, new, kind):
        return new

    def cluster(self, n, offsets, target, method, score):
        return CL.MODELS[method](n, offsets, target, score)


def _resized(x, n, fill):
    return np.resize(np.concatenate([x, np.full(1, fill, x.dtype)]), n).astype(x.dtype)


class HasTotalStays(Model):
    name = "1 a search or a top into hits with totals leaves has_total set"
    kinds = ("search", "top")

    def hits_after(self, before, new, kind):
        if kind in ("search", "top") and before is not None and before["has_total"]:
            return dict(new, has_total=True, total=_resized(before["total"], new["n_hits"], 0))
        return new


class HasWeightsStays(Model):
    name = "2 an unweighted neighbors into weighted hits leaves has_weights set"
    kinds = ("neighbors",)

    def hits_after(self, before, new, kind):
        if kind == "neighbors" and before is not None and before["has_weights"]:
            return dict(new, has_weights=True, dot=_resized(before["dot"], new["n_hits"], 0), min_sum=_resized(before["min_sum"], new["n_hits"], 0))
        return new


class WeightedStays(Model):
    name = "3 a plain compare into a weighted compare leaves weighted set"
    kinds = ("compare",)

    def cmp_after(self, before, new, kind):
        if kind == "compare" and before is not None and before["weighted"]:
            cells = new["shared"].size
            return dict(new, weighted=True, dot=_resized(before["dot"].ravel(), cells, 0).reshape(new["shared"].shape),
                        min_sum=_resized(before["min_sum"].ravel(), cells, 0).reshape(new["shared"].shape))
        return new


class StaleCountsRead(Model):
    name = "4 a weighted kernel reads a->counts without the a->counted test: the stale counts of an object an uncounted entry wrote last"
    kinds = ("compare_counted", "neighbors_counted")

    def counts_read(self, t, stale):
        if t[2] is None and stale is not None:
            return _resized(stale, AP.n_values(t), 1)
        return t[2]


def _pair_sums(x, cx, y, cy, limit):
    """(the true sum of the count products, the sum of the minima) over the walked values both sets hold, in Python integers"""
    if limit:
        u = np.union1d(x, y)[:limit]
        last = u[-1] if len(u) else None
    _, ix, iy = np.intersect1d(x, y, return_indices=True)
    if limit and len(ix):
        keep = x[ix] <= last
        ix, iy = ix[keep], iy[keep]
    px, py = cx[ix].tolist(), cy[iy].tolist()
    return sum(p * q for p, q in zip(px, py)), sum(min(p, q) for p, q in zip(px, py))


def _cells(a, ca, b, cb, limit, where, fn):
    """fn(true dot, min_sum) -> (dot, min_sum) for the cells of `where`"""
    A, B = SO.split(a[0], a[1]), SO.split(b[0], b[1])
    CA = SO.split(a[0], ca) if ca is not None else WC.ones(A)
    CB = SO.split(b[0], cb) if cb is not None else WC.ones(B)
    return {(int(i), int(j)): fn(*_pair_sums(A[i], CA[i], B[j], CB[j], limit)) for i, j in np.argwhere(where)}


class DotWraps(Model):
    name = "5 dot wraps instead of saturating at 2^64 - 1"
    kinds = ("compare_counted", "neighbors_counted")

    def weights(self, a, ca, b, cb, limit):
        sh, tt, dt, ms = weighted_compare(a, ca, b, cb, limit)
        if (dt == U64(MAX64)).any():  # (no other cell reached 2^64)
            dt = dt.copy()
            for (i, j), (d, _) in _cells(a, ca, b, cb, limit, dt == U64(MAX64), lambda d, m: (d & MAX64, m)).items():
                dt[i, j] = d
        return sh, tt, dt, ms


class SumsqWraps(Model):
    name = "6 sumsq wraps instead of saturating"
    kinds = SETS_KINDS

    def sumsq(self, t):
        q = sumsq_of(t)
        if (q == U64(MAX64)).any():
            q = np.array([sum(int(c) * int(c) for c in cs) & MAX64 for cs in SO.split(t[0], t[2])], U64)
        return q


class WeightsPastTheLimit(Model):
    name = "7 dot and min_sum summed over all shared values, not over the walked prefix (limit ignored for the weights)"
    kinds = ("compare_counted", "neighbors_counted")

    def weights(self, a, ca, b, cb, limit):
        sh, tt, dt, ms = weighted_compare(a, ca, b, cb, limit)
        if limit:
            dt, ms = dt.copy(), ms.copy()
            for (i, j), (d, m) in _cells(a, ca, b, cb, 0, sh > 0, lambda d, m: (min(d, MAX64), m)).items():
                dt[i, j], ms[i, j] = d, m
        return sh, tt, dt, ms


class _Rule(Model):
    def keeps(self, s, t, i, j, r):
        raise NotImplementedError

    def kept(self, sh, tt, dt, ms, rule):
        n_a, n_b = sh.shape
        offsets, cells = np.zeros(n_a + 1, U64), []
        for i in range(n_a):
            cells += [(i, j) for j in range(n_b) if self.keeps(int(sh[i, j]), int(tt[i, j]), i, j, rule)]
            offsets[i + 1] = len(cells)
        rows, cols = np.array([c[0] for c in cells], np.int64), np.array([c[1] for c in cells], np.int64)
        out = (offsets, cols.astype(U32), sh[rows, cols].astype(U32), tt[rows, cols].astype(U32))
        return out + ((None, None) if dt is None else (dt[rows, cols].astype(U64), ms[rows, cols].astype(U64)))


class JaccardIn32Bits(_Rule):
    name = "8 the Jaccard rule with its products in 32 bits"
    kinds = ("neighbors", "neighbors_counted")

    def keeps(self, s, t, i, j, r):
        m = 0xFFFFFFFF
        return s >= max(r["min_shared"], 1) and (r["den"] == 0 or ((s * r["den"]) & m) >= ((r["num"] * t) & m)) and (not r["upper"] or j > i)


class UpperKeepsTheDiagonal(_Rule):
    name = "9 upper keeps j >= i"
    kinds = ("neighbors", "neighbors_counted")

    def keeps(self, s, t, i, j, r):
        return NC.keeps(s, t, i, j, r["min_shared"], r["num"], r["den"], False) and (not r["upper"] or j >= i)


class WeightsInRecordOrder(Model):
    name = "10 the weights of a row placed in record order, not in the sorted column order (a row's weights reversed)"
    kinds = ("neighbors_counted",)

    def kept(self, sh, tt, dt, ms, rule):
        o, t, s, tot, d, m = Model.kept(self, sh, tt, dt, ms, rule)
        if d is not None:
            d, m = d.copy(), m.copy()
            for i in range(len(o) - 1):
                lo, hi = int(o[i]), int(o[i + 1])
                d[lo:hi], m[lo:hi] = d[lo:hi][::-1].copy(), m[lo:hi][::-1].copy()
        return o, t, s, tot, d, m


class ClusterReadsDirectedEdges(Model):
    name = "11 cluster reads hit (i, j) as the directed edge i -> j only: j never learns of i"
    kinds = ("cluster",)

    def cluster(self, n, offsets, target, method, score):
        order, rank = CL.ranking(n, score)
        out = [[] for _ in range(n)]
        for i, j in CL.edge_list(offsets, target, directed=True):
            out[i].append(j)
        if method == "greedy":
            is_rep, rep_of = [False] * n, [0] * n
            for v in order:
                cands = [u for u in out[v] if is_rep[u]]
                if cands:
                    rep_of[v] = min(cands, key=lambda u: rank[u])
                else:
                    is_rep[v], rep_of[v] = True, v
            return CL.layout(rep_of)
        best = list(range(n))  # components: every node takes the best rank it can REACH along the arrows
        changed = True
        while changed:
            changed = False
            for v in range(n):
                for u in out[v]:
                    if rank[best[u]] < rank[best[v]]:
                        best[v], changed = best[u], True
        return CL.layout(best)


class ComponentsRepSmallestIndex(Model):
    name = "12 components: the representative is the smallest index, not the best rank"
    kinds = ("cluster",)

    def cluster(self, n, offsets, target, method, score):
        return CL.MODELS[method](n, offsets, target, None if method == "components" else score)


class GreedyJoinsSmallestIndex(Model):
    name = "13 greedy joins the neighbouring representative of smallest index, not of best rank"
    kinds = ("cluster",)

    def cluster(self, n, offsets, target, method, score):
        if method != "greedy":
            return CL.MODELS[method](n, offsets, target, score)
        order, _ = CL.ranking(n, score)
        nbr = [[] for _ in range(n)]
        for u, v in CL.edge_list(offsets, target):
            nbr[u].append(v)
            nbr[v].append(u)
        is_rep, rep_of = [False] * n, [0] * n
        for v in order:
            cands = [u for u in nbr[v] if is_rep[u]]
            if cands:
                rep_of[v] = min(cands)
            else:
                is_rep[v], rep_of[v] = True, v
        return CL.layout(rep_of)


SABOTAGES = (HasTotalStays, HasWeightsStays, WeightedStays, StaleCountsRead, DotWraps, SumsqWraps, WeightsPastTheLimit, JaccardIn32Bits,
             UpperKeepsTheDiagonal, WeightsInRecordOrder, ClusterReadsDirectedEdges, ComponentsRepSmallestIndex, GreedyJoinsSmallestIndex)


# ---- the interpreter ----
class State(AP.State):
    """AP's state -- objs, maker, cmps, hits -- and the makers of the other pools, the clusters, and per sets object the counts its
    array still holds after an uncounted entry wrote it (stale)"""

    def __init__(self, model, read_values=None):
        AP.State.__init__(self, model, read_values)
        self.cmaker, self.hmaker, self.clusters, self.kmaker, self.stale = {}, {}, {}, {}, {}

    def end(self):
        return dict(pool=dict(self.objs), compares=dict(self.cmps), hits=dict(self.hits), clusters=dict(self.clusters))


def _sets_step(st, step):
    out = step["out"]
    before, stale = st.objs.get(out), st.stale.get(out)
    rec = AP.apply(st, step)
    new = (rec["offsets"], rec["values"], rec["counts"])
    rec["sumsq"] = st.model.sumsq(new)
    held = None if before is None else before[2] if before[2] is not None else stale
    if new[2] is None and held is not None and step.get("keep", True):
        st.stale[out] = held
    else:
        st.stale.pop(out, None)
    return rec


def _write_hits(st, step, new):
    slot = step["slot"]
    new = st.model.hits_after(st.hits.get(slot), new, step["kind"])
    st.hits[slot], st.hmaker[slot] = new, HITS_ENTRY[step["kind"]]
    return dict(new)


def _touched(st, step):
    """the objects a refused call names, as they must still be"""
    return dict(sets=st.snap(dict.fromkeys(step[x] for x in ("a", "b") if step.get(x) is not None)),
                hits={i: st.hits[i] for i in dict.fromkeys(step[x] for x in ("hits", "hslot") if step.get(x) is not None)},
                compares={i: st.cmps[i] for i in [step.get("cmp")] if i is not None},
                clusters={i: st.clusters[i] for i in [step.get("kslot")] if i is not None})


def apply(st, step):
    """one step on the model's state -> what the step must yield"""
    M, k = st.model, step["kind"]
    if k in SETS_KINDS:
        return _sets_step(st, step)
    if k == "refused":
        return dict(rc="ERR_ARG", **_touched(st, step))
    if k in ("compare", "compare_counted"):
        a, b = st.objs[step["a"]], st.objs[step["b"]]
        if k == "compare":
            sh, tt = plain_compare(a, b, step["limit"])
            dt = ms = None
        else:
            sh, tt, dt, ms = M.weights(a, M.counts_read(a, st.stale.get(step["a"])), b, M.counts_read(b, st.stale.get(step["b"])), step["limit"])
        new = dict(n_a=AP.n_sets(a), n_b=AP.n_sets(b), limit=step["limit"], shared=sh, total=tt, weighted=dt is not None, dot=dt, min_sum=ms)
        new = M.cmp_after(st.cmps.get(step["cmp"]), new, k)
        st.cmps[step["cmp"]], st.cmaker[step["cmp"]] = new, CMP_ENTRY[k]
        return dict(new, figures=AP.plan_figures(a, b, step["limit"]), operands=st.snap([step["a"], step["b"]]))
    if k in ("neighbors", "neighbors_counted"):
        a, b = st.objs[step["a"]], st.objs[step["b"]]
        if k == "neighbors":
            sh, tt = plain_compare(a, b, step["limit"])
            dt = ms = None
        else:
            sh, tt, dt, ms = M.weights(a, M.counts_read(a, st.stale.get(step["a"])), b, M.counts_read(b, st.stale.get(step["b"])), step["limit"])
        o, t, s, tot, d, m = M.kept(sh, tt, dt, ms, rule_of(step))
        tiles, skipped = NC.expected_tiles(AP.n_sets(a), AP.n_sets(b), step["upper"], CMP)
        rec = _write_hits(st, step, hits_of(AP.n_sets(a), o, t, s, tot, d, m))
        return dict(rec, tiles=tiles, skipped=skipped, operands=st.snap([step["a"], step["b"]]))
    if k == "search":
        a, q = st.objs[step["a"]], st.objs[step["q"]]
        o, t, s = M.search(a, q, step["min_shared"])
        return dict(_write_hits(st, step, hits_of(AP.n_sets(q), o, t, s)), operands=st.snap([step["a"], step["q"]]))
    if k == "top":
        h = st.hits[step["hits"]]
        o, t, s = M.top((h["offsets"], h["target"], h["shared"]), step["n"])
        return dict(_write_hits(st, step, hits_of(h["n_queries"], o, t, s)), input=st.hits[step["hits"]])
    if k == "hits_load":
        return _write_hits(st, step, hits_of(len(step["offsets"]) - 1, step["offsets"], step["target"], step["shared"], step["total"]))
    assert k == "cluster", k
    h = st.hits[step["hits"]]
    n = h["n_queries"]
    new = clusters_of(M.cluster(n, h["offsets"], h["target"], step["method"], step["score"]))
    st.clusters[step["slot"]], st.kmaker[step["slot"]] = new, "bsk_hits_cluster"
    rounds = CL.ROUND_MODELS[step["method"]](n, h["offsets"], h["target"], step["score"])[1]
    return dict(new, figures=(rounds, CL.n_offdiagonal(h["offsets"], h["target"])), input=h)


def run_model(program, model=None, read_values=None):
    """-> one record per step and a last one: every object alive at the end.  read_values: the values of the sketch step's reads (from
    the device; None: AP.standin_values)"""
    st = State(model or Model(), read_values)
    records = [apply(st, step) for step in program]
    records.append(st.end())
    return records


def _replay(st, step, rec):
    """the state after a step whose record is known"""
    k = step["kind"]
    if k in SETS_KINDS:
        if k == "sketch":
            st.sketch, st.read_values = step, AP.standin_values(step)
        out = step["out"]
        before, stale = st.objs.get(out), st.stale.get(out)
        held = None if before is None else before[2] if before[2] is not None else stale
        if step.get("keep", True):
            st.objs[out] = (rec["offsets"], rec["values"], rec["counts"])
        else:
            st.objs.pop(out, None)
        if rec["counts"] is None and held is not None and step.get("keep", True):
            st.stale[out] = held
        else:
            st.stale.pop(out, None)
    elif k in CMP_ENTRY:
        st.cmps[step["cmp"]] = {key: rec[key] for key in rec if key not in ("figures", "operands")}
    elif k in HITS_ENTRY:
        st.hits[step["slot"]] = {key: rec[key] for key in rec if key not in ("tiles", "skipped", "operands", "input")}
    elif k == "cluster":
        st.clusters[step["slot"]] = {key: rec[key] for key in rec if key not in ("figures", "input")}


def first_difference(program, want, model):
    """the first step at which `model` yields something else than the records `want` -> (step, differences), or None"""
    st = State(model)
    for i, step in enumerate(program):
        if step["kind"] not in model.kinds:  # nothing differed so far and this step cannot: its record is the wanted one
            _replay(st, step, want[i])
            continue
        diff = AP.same(want[i], apply(st, step))
        if diff:
            return i, diff
    diff = AP.same(want[-1], st.end())
    return (len(program), diff) if diff else None


# ---- the generator ----
class _Gen(AP._Gen):
    def __init__(self, seed):
        AP._Gen.__init__(self, seed)
        self.st = State(Model())

    def emit(self, step):
        rec = apply(self.st, step)
        self.steps.append(step)
        self.records.append(rec)
        self.made += rec.get("n_values", 0)
        return rec

    def finish(self, step):
        rec = AP._Gen.finish(self, step)
        if not step.get("keep", True):
            self.st.stale.pop(step["out"], None)
        return rec

    def choice(self, xs):
        xs = list(xs)
        return xs[int(self.rng.integers(0, len(xs)))]

    def slot(self, step, pool, maker, prefix, exclude=()):
        """where a result goes: a new object or, half the time, a live one of the pool"""
        live = [i for i in pool if i not in exclude]
        if live and self.rng.random() < 0.5:
            step["slot"], step["into"] = self.choice(live), True
        else:
            step["slot"], step["into"] = self.new_id(prefix), False
        step["made_by"] = maker.get(step["slot"])
        return step

    def operands(self, weighted, itself):
        """a and b of a compare or a neighbours call: b is a itself with that probability; a weighted call reaches half the time for
        an object with stale counts"""
        st = self.st
        a = self.choice(st.stale) if weighted and st.stale and self.rng.random() < 0.6 else self.pick()
        return a, a if self.rng.random() < itself else self.choice(st.stale) if weighted and st.stale and self.rng.random() < 0.3 else self.pick()

    def limit(self, a, b, bound):
        objs = self.st.objs
        limit = int(LIMITS[int(self.rng.integers(0, len(LIMITS)))])
        cut = lambda t, lim: np.minimum(np.diff(t[0]).astype(np.int64), lim or (1 << 62))  # noqa: E731
        work = lambda lim: int(cut(objs[a], lim).sum()) * AP.n_sets(objs[b]) + int(cut(objs[b], lim).sum()) * AP.n_sets(objs[a])  # noqa: E731
        if work(limit) > bound:
            limit = int((1, 7, 128, 129)[int(self.rng.integers(0, 4))])
        if work(limit) > bound:
            limit = 7
        return limit


def _graph(rng):
    """a seeded graph for bsk_hits_from_host -> (text, n, directed pairs)"""
    kind = GRAPHS[int(rng.choice(len(GRAPHS), p=[0.34, 0.33, 0.33]))]
    seed = int(rng.integers(0, 1 << 16))
    if kind == "multigraph":
        n, pairs = CL.random_multigraph(seed)
        return "random_multigraph(%d): n=%d" % (seed, n), n, pairs
    n = int(CL.SIZES[int(rng.integers(0, len(CL.SIZES)))])
    form = ("full", "upper", "mixed")[int(rng.integers(0, 3))]
    if kind == "path":
        shuffled = bool(rng.random() < 0.6)
        edges = CL.path(n, seed if shuffled else None)
        return "path(%d%s) %s" % (n, ", seed=%d" % seed if shuffled else "", form), n, CL.forms(edges)[form]
    hub = 0 if rng.random() < 0.5 else n - 1
    return "star(%d, hub %d) %s" % (n, hub, form), n, CL.forms([(hub, v) for v in range(n) if v != hub])[form]


def _step(g, kind, src=None):
    """one call of a kind -> its record, or None where nothing alive fits it.  src: the hits a cluster step must take, the `a` of a
    weighted one"""
    rng, st = g.rng, g.st
    if kind in AP.KINDS and kind not in ("compare", "search"):
        return AP._step(g, kind)
    if kind in ("compare", "compare_counted"):
        a, b = g.operands(kind == "compare_counted", 0.25)
        a = a if src is None else src
        limit = g.limit(a, b, COMPARE_WORK if kind == "compare" else WEIGHTED_WORK)
        cmp = g.new_id("c")
        if st.cmps and rng.random() < 0.6:  # a live object, mostly one the other compare wrote last
            other = [i for i, c in st.cmps.items() if c["weighted"] != (kind == "compare_counted")]
            cmp = g.choice(other) if other and rng.random() < 0.75 else g.choice(st.cmps)
        return g.emit(dict(kind=kind, a=a, b=b, limit=limit, cmp=cmp, made_by=st.cmaker.get(cmp), stale=[i for i in dict.fromkeys((a, b)) if i in st.stale]))
    if kind in ("neighbors", "neighbors_counted"):
        a, b = g.operands(kind == "neighbors_counted", 1 / 3)
        if AP.n_sets(st.objs[a]) > AP.n_sets(st.objs[b]) and rng.random() < 0.4:
            a, b = b, a  # (more columns than rows: hits that bsk_hits_cluster refuses)
        a = a if src is None else src
        step = dict(kind=kind, a=a, b=b, limit=g.limit(a, b, WEIGHTED_WORK), min_shared=int(MIN_SHARED[int(rng.integers(0, 3))]),
                    min_jaccard=MIN_JACCARD[int(rng.choice(len(MIN_JACCARD), p=JACCARD_WEIGHTS))], upper=bool(rng.random() < 0.4),
                    stale=[i for i in dict.fromkeys((a, b)) if i in st.stale] if kind == "neighbors_counted" else [])
        none = lambda: int(NC.filter_matrices(*plain_compare(st.objs[a], st.objs[step["b"]], step["limit"]), **rule_of(step))[0][-1]) == 0  # noqa: E731
        if none() and rng.random() < 0.92:  # mostly a call that keeps a pair: a looser rule, the full matrix, then a against itself
            step["min_shared"] = 1
            if none():
                step["min_jaccard"] = None
            if none():
                step["upper"] = False
            if none():
                step["b"] = a
        return g.emit(g.slot(step, st.hits, st.hmaker, "h"))
    if kind == "search":
        a = g.pick()
        q = a if rng.random() < 1 / 3 else g.pick()
        return g.emit(g.slot(dict(kind="search", a=a, q=q, min_shared=int(MIN_SHARED[int(rng.integers(0, 3))])), st.hits, st.hmaker, "h"))
    if kind == "top":
        if not st.hits:
            return None
        with_totals = [i for i, h in st.hits.items() if h["has_total"] and h["n_hits"] and square(h)]  # (what a k-nearest graph is cut from)
        src = g.choice(with_totals) if with_totals and rng.random() < 0.7 else g.choice(st.hits)
        step = dict(kind="top", hits=src, n=int(TOP_NS[int(rng.random() < 0.65)]), input_made_by=st.hmaker[src])
        return g.emit(g.slot(step, st.hits, st.hmaker, "h", exclude=(src,)))
    if kind == "hits_load":
        text, n, pairs = _graph(rng)
        o, t, s = CL.csr(n, pairs)
        s = rng.integers(1, 10, len(t)).astype(U32)
        total = (s + rng.integers(0, 10, len(t)).astype(U32)).astype(U32) if rng.random() < 0.5 else None
        return g.emit(g.slot(dict(kind="hits_load", graph=text, n=n, offsets=o, target=t, shared=s, total=total), st.hits, st.hmaker, "h"))
    assert kind == "cluster", kind
    ok = [i for i, h in st.hits.items() if square(h)]
    if not ok:
        return None
    tops = [i for i in ok if st.hmaker[i] == "bsk_hits_top" and not symmetric(st.hits[i])]
    searches = [i for i in ok if st.hmaker[i] == "bsk_index_search" and st.hits[i]["n_hits"]]
    r = rng.random()
    src = src if src is not None else g.choice(tops) if tops and r < 0.55 else g.choice(searches) if searches and r < 0.7 else g.choice(ok)
    n = st.hits[src]["n_queries"]
    sk = SCORE_KINDS[int(rng.integers(0, 3))]
    sname, sseed = SCORE_NAMES[int(rng.integers(0, len(SCORE_NAMES)))], int(rng.integers(0, 1000))
    score = None if sk == "none" else np.full(n, 5, U64) if sk == "equal" else CL.scores(n, sseed)[sname]
    step = dict(kind="cluster", hits=src, method=CL.METHODS[int(rng.integers(0, 2))], score_kind=sk, score=score,
                score_text="None" if sk == "none" else "all 5" if sk == "equal" else "scores(%d, %d)[%r]" % (n, sseed, sname), input_made_by=st.hmaker[src])
    return g.emit(g.slot(step, st.clusters, st.kmaker, "k"))


def _refused(g):
    """a call the library refuses before it takes the slot over; the slot and everything the call names must stay what they were"""
    rng, st = g.rng, g.st
    order = [REFUSALS[int(i)] for i in rng.permutation(len(REFUSALS))]
    if rng.random() < 0.3:
        order.insert(0, REFUSALS[0])  # (rectangular hits are rare: taken more often when there are some)
    for what in order:  # the first one the live objects allow
        step = dict(kind="refused", what=what, a=None, b=None, hits=None, hslot=None, cmp=None, kslot=None, counted=bool(rng.random() < 0.5))
        hslot = g.choice(st.hits) if st.hits and rng.random() < 0.7 else None
        if what == "cluster of rectangular hits":
            rect = [i for i, h in st.hits.items() if not square(h)]
            if not rect:
                continue
            step["hits"] = g.choice(rect)
            step["kslot"] = g.choice(st.clusters) if st.clusters and rng.random() < 0.8 else None
        elif what in ("fetch_weights of hits without weights", "fetch_totals of hits without totals"):
            flag = "has_weights" if "weights" in what else "has_total"
            bare = [i for i, h in st.hits.items() if not h[flag]]
            if not bare:
                continue
            step["hits"] = g.choice(bare)
        elif what == "fetch_weights of an unweighted compare":
            plain = [i for i, c in st.cmps.items() if not c["weighted"]]
            if not plain:
                continue
            step["cmp"] = g.choice(plain)
        elif what in ("neighbors with jaccard_num > jaccard_den", "neighbors with an unknown flag bit", "hits of the other engine in the slot"):
            step["a"], step["b"] = g.pick(), g.pick()
            step["hslot"] = None if "other engine" in what else hslot
        elif what == "clusters of the other engine in the slot":
            ok = [i for i, h in st.hits.items() if square(h)]
            if not ok:
                continue
            step["hits"] = g.choice(ok)
        elif what == "hits_from_host with a row not strictly ascending":
            step["hslot"] = hslot
        else:
            assert what == "top into its own input", what
            if not st.hits:
                continue
            step["hits"] = step["hslot"] = g.choice(st.hits)
        return g.emit(step)
    raise AssertionError("no refusal fits")  # (the two neighbours ones always do)


KINDS = ("op", "op_counted", "reduce", "filter", "bottom", "result_sets", "compare", "compare_counted", "neighbors", "neighbors_counted", "search", "top",
         "hits_load", "cluster")
KIND_WEIGHTS = (0.06, 0.06, 0.04, 0.03, 0.04, 0.03, 0.08, 0.10, 0.10, 0.11, 0.07, 0.10, 0.05, 0.13)


def program(seed):
    return program_and_records(seed)[0]


def program_and_records(seed):
    """the program of a seed and run_model's records of it (the generator runs the model as it goes)"""
    g = _Gen(seed)
    rng = g.rng
    name, pool = AP._universe(rng)
    n = int(NS[int(rng.integers(0, len(NS)))])
    sketched = int(rng.integers(0, 4)) if rng.random() < 0.25 else None
    counted = [bool(rng.random() < 0.5) for _ in range(4)]
    if len(set(counted)) == 1:  # at least one counted and one uncounted source
        counted[int(rng.integers(0, 4))] ^= True
    for which in range(4):
        ns = n if which < 3 else 1
        if which == sketched:
            whole = which == 3
            mini = bool(rng.random() < 0.5)
            g.emit(dict(kind="sketch", out=g.new_id(), sketch="minimizer" if mini else "nthash", k=15 if mini else 21, w=5 if mini else 0,
                        reads=AP._reads(rng, int(rng.integers(24, 49)) if whole else ns), whole=whole, scale=int(rng.choice([1, 3])),
                        counted=counted[which], no_small=bool(rng.random() < 0.4), universe=name))
            continue
        sets, layout = AP._collection(rng, pool, name.startswith("dense"), AP._sizes(rng, ns, which == 3))
        offs, vals = SO.collection(sets)
        g.emit(dict(kind="load", out=g.new_id(), offsets=offs, values=vals, counts=AP._counts(rng, len(vals)) if counted[which] else None,
                    layout=layout, universe=name))
    todo = int(rng.integers(10, 17))
    while todo:
        if rng.random() < 1 / 12:
            _refused(g)
            todo -= 1
            continue
        kind = KINDS[int(rng.choice(len(KINDS), p=KIND_WEIGHTS))]
        if _step(g, kind) is None:
            continue
        todo -= 1
        made = g.steps[-1].get("slot")
        if kind == "top" and todo and square(g.st.hits[made]) and not symmetric(g.st.hits[made]) and rng.random() < 0.5:
            _step(g, "cluster", src=made)  # a k-nearest graph, one direction per edge: clustered while it is there
            todo -= 1
        made = g.steps[-1].get("out")
        if kind in SETS_KINDS and todo and made in g.st.stale and rng.random() < 0.5:
            _step(g, ("compare_counted", "neighbors_counted")[int(rng.integers(0, 2))], src=made)  # stale counts: read while they are there
            todo -= 1
    g.records.append(g.st.end())
    return g.steps, g.records


# ---- the text of a program ----
def describe_step(i, s):
    k = s["kind"]
    if k in SETS_KINDS:
        return AP.describe_step(i, s)
    into = " into %s (made by %s)" % (s.get("slot", s.get("cmp")), s["made_by"]) if s.get("made_by") else ""
    stale = "; stale counts in %s" % ", ".join(s["stale"]) if s.get("stale") else ""
    if k in CMP_ENTRY:
        text = "%s = %s.%s(%s, limit=%d)%s%s" % (s["cmp"], s["a"], k, s["b"], s["limit"], into, stale)
    elif k in ("neighbors", "neighbors_counted"):
        text = "%s = %s.%s(%s, limit=%d, min_shared=%d, min_jaccard=%r, upper=%s)%s%s" % (s["slot"], s["a"], k, s["b"], s["limit"], s["min_shared"], s["min_jaccard"],
                                                                                       s["upper"], into, stale)
    elif k == "search":
        text = "%s = %s.index().search(%s, min_shared=%d)%s" % (s["slot"], s["a"], s["q"], s["min_shared"], into)
    elif k == "top":
        text = "%s = %s.top(%d)%s   [%s made by %s]" % (s["slot"], s["hits"], s["n"], into, s["hits"], s["input_made_by"])
    elif k == "hits_load":
        text = "%s = hits_from_arrays(%s; %d hits, crc %s, %s)%s" % (s["slot"], s["graph"], len(s["target"]), AP.digest(s["offsets"], s["target"], s["shared"], s["total"]),
                                                                   "with totals" if s["total"] is not None else "no totals", into)
    elif k == "cluster":
        text = "%s = %s.cluster(%r, score=%s)%s   [%s made by %s]" % (s["slot"], s["hits"], s["method"], s["score_text"], into, s["hits"], s["input_made_by"])
    else:
        text = "REFUSED (%s): a=%s b=%s hits=%s cmp=%s hits slot=%s clusters slot=%s%s" % (s["what"], s["a"], s["b"], s["hits"], s["cmp"], s["hslot"], s["kslot"],
                                                                                         " (counted)" if s["counted"] and s["a"] is not None else "")
    return "%2d  %s" % (i, text)


def describe(prog, upto=None):
    return "\n".join(describe_step(i, s) for i, s in enumerate(prog[:upto]))


def message(seed, i, prog, what):
    """what an assertion says: the seed, the step and the program up to it"""
    return "seed %#x, step %d: %s\n%s\n(python -m tests.graph_programs %#x)" % (seed, i, what, describe(prog, i + 1), seed)


# ---- what a campaign reaches ----
def figures(programs_and_records):
    """counts over programs with their model records: what tests/test_graph_programs.py holds the campaign to"""
    f = dict(steps=0, checked=0, entries=set(), neighbour_steps=0, no_pair=0, into_other=0, totals_to_none=0, weights_to_none=0, none_to_weights=0,
             weighted_to_plain=0, plain_to_weighted=0, stale_weighted=0, top_clusters=0, search_clusters=0, skipping=0, jaccards=set(), sizes=set(),
             methods=set(), score_kinds=set(), refusals=set(), saturated_dot=0, saturated_sumsq=0, cut_unions=0, methods_differ=0, long_greedy=0,
             grown=0)
    for prog, recs in programs_and_records:
        objs, hits, cmps = {}, {}, {}
        f["checked"] += sum(len(p) for p in recs[-1].values())
        for s, r in zip(prog, recs):
            k = s["kind"]
            f["steps"] += k not in ("load", "sketch")
            f["checked"] += k != "refused"
            if k == "refused":
                f["refusals"].add(s["what"])
            elif k in SETS_KINDS:
                f["entries"].add("bsk_sets_sumsq")
                f["saturated_sumsq"] += bool((r["sumsq"] == U64(MAX64)).any())
                if s.get("keep", True):
                    objs[s["out"]] = (r["offsets"], r["values"], r["counts"])
                else:
                    objs.pop(s["out"], None)
            elif k in CMP_ENTRY:
                f["entries"].add(CMP_ENTRY[k])
                before = cmps.get(s["cmp"])
                if before is not None:
                    f["weighted_to_plain"] += before["weighted"] and not r["weighted"]
                    f["plain_to_weighted"] += r["weighted"] and not before["weighted"]
                if r["weighted"]:
                    f["entries"].add("bsk_compare_fetch_weights")
                    f["saturated_dot"] += bool((r["dot"] == U64(MAX64)).any())
                    f["stale_weighted"] += bool(s["stale"])
                cmps[s["cmp"]] = r
            elif k in HITS_ENTRY:
                f["entries"].add(HITS_ENTRY[k])
                f["entries"] |= ({"bsk_hits_fetch_totals"} if r["has_total"] else set()) | ({"bsk_hits_fetch_weights"} if r["has_weights"] else set())
                before = hits.get(s["slot"])
                if before is not None:
                    f["totals_to_none"] += before["has_total"] and not r["has_total"]
                    f["weights_to_none"] += before["has_weights"] and not r["has_weights"]
                    f["none_to_weights"] += r["has_weights"] and not before["has_weights"]
                    f["grown"] += r["n_hits"] > before["n_hits"]
                if k in ("neighbors", "neighbors_counted", "search"):
                    f["into_other"] += before is not None and s["made_by"] != HITS_ENTRY[k]
                if k in ("neighbors", "neighbors_counted"):
                    f["neighbour_steps"] += 1
                    f["no_pair"] += r["n_hits"] == 0
                    f["skipping"] += r["skipped"] > 0
                    f["jaccards"].add(s["min_jaccard"])
                    f["stale_weighted"] += bool(s["stale"])
                    if r["has_weights"]:
                        f["saturated_dot"] += bool((r["dot"] == U64(MAX64)).any())
                    if s["limit"] and r["n_hits"]:
                        sa, sb = np.diff(objs[s["a"]][0]).astype(np.int64), np.diff(objs[s["b"]][0]).astype(np.int64)
                        rows = np.repeat(np.arange(r["n_queries"]), np.diff(r["offsets"]).astype(np.int64))
                        f["cut_unions"] += bool((np.maximum(sa[rows], sb[r["target"].astype(np.int64)]) > s["limit"]).any())
                if k == "hits_load":
                    f["sizes"].add(s["n"])
                hits[s["slot"]] = r
            else:
                assert k == "cluster", k
                f["entries"] |= {"bsk_hits_cluster", "bsk_clusters_fetch"}
                f["methods"].add(s["method"])
                f["score_kinds"].add(s["score_kind"])
                h = r["input"]
                f["top_clusters"] += s["input_made_by"] == "bsk_hits_top" and not symmetric(h)
                f["search_clusters"] += s["input_made_by"] == "bsk_index_search"
                both = [CL.MODELS[m](h["n_queries"], h["offsets"], h["target"], s["score"]) for m in CL.METHODS]
                f["methods_differ"] += not CL.same(*both)
                f["long_greedy"] += s["method"] == "greedy" and r["figures"][0] >= 3
    return f


if __name__ == "__main__":
    for arg in sys.argv[1:]:
        print("program %#x" % int(arg, 0))
        print(describe(program(int(arg, 0))))
