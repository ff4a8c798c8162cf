"""Seeded programs over the long-lived indexes, the window sets and the weighted and folded hits of the sets side (search.hip, windows.hip,
fold.hip) and their NumPy interpreter: the third campaign, beside tests/algebra_programs.py (AP) and tests/graph_programs.py (GP), whose
programs and records it leaves as they are.

program(seed) starts as a GP program does -- four sources, at least one counted and one uncounted, one of them ALWAYS from a sketch result,
whose tuples (hash and position) the window sets are cut from -- and then chains 10 to 16 calls over four pools:
  sets      AP's sets-making kinds (the operands, and the objects whose counts array is STALE: counted once, last written by an uncounted
            entry); windows = BatchResult.window_sets(..., into=any live sets or None), a sets record plus group_offsets; reduce of a window
            object by its own group_offsets (the per-sequence sets again); copy = a live object's arrays loaded on the second engine (the
            queries of an attached index); close_sets of an object an index was built from or a weighted result is bound to;
  indexes   index / index_counted of any live sets, stale-counts and window sets included; attach to the other engine; close_index of a
            handle while a sibling lives.  An index outlives its source sets: the generator overwrites or closes them on purpose;
  hits      search / search_counted on any live index handle (min_shared and both covers, queries on the handle's engine), fold (by the
            group_offsets of the window object the index was built from, or by random runs with empty groups), top, neighbors,
            neighbors_counted and hits_load -- any writer into any object of its engine, so that has_total, has_weights and has_members
            follow the last writer through all twelve transitions;
  refused   calls the library must refuse with BSK_ERR_ARG, the slot and every operand left as they were.
At the end of a program every live object is fetched once more and every live hits object is asked containment() and jaccard(), every
weighted one the weighted formulas -- late, after their operands may have been overwritten or closed: the record is then "stale" (the
owners raise ValueError), never the call's dot and min_sum mixed with other sets' norms; "closed" where the index handle of a weighted
search was closed before a formula fetched its norms.

run_model(program) gives what every step must yield, with the suites' own references (search_cases.ref_search / ref_top / posting_sums /
directory, search_counted_cases.ref_search_counted / paths / plan_tail, window_cases.windows_model / fold_model, neighbor_cases,
neighbor_counted_cases, counts_cases.ref_counted, AP.Model and GP.Model); AP.same is the one comparison, used by
tests/test_gpu_index_fuzz.py on the device's records and by tests/test_index_programs.py on the records of the SABOTAGES.  Floats are
computed from the exact integers with the owners' expressions and compared as their bit patterns (fbits).  Nothing here imports the engine.

    python -m tests.index_programs SEED      prints the program of that seed, call by call"""
import re
import sys

import numpy as np

from tests import algebra_programs as AP
from tests import counts_cases as CN
from tests import graph_programs as GP
from tests import neighbor_cases as NC
from tests import search_cases as SR
from tests import search_counted_cases as SW
from tests import setops_cases as SO
from tests import window_cases as WN

U64, U32, I64, F64 = np.uint64, np.uint32, np.int64, np.float64
MAX64, CMP = GP.MAX64, AP.CMP

BASE, BLOCKS, PER_BLOCK = 0x1D3C0000, 8, 20
NS = AP.NS
MIN_SHARED = (1, 2, 5)
COVERS = (0.0, 0.0, 0.0, 0.25, 0.5, 1.0)
TOP_NS = (1, 3)
WINDOWS = (dict(window=4), dict(window=7, step=3), dict(window=16), dict(window=16, step=16), dict(window=32, step=8), dict(window=9, step=3), dict(count=2), dict(count=3),
           dict(count=7))
RULES = [dict(), dict(min_members=0), dict(min_members=2), dict(frac=(1, 1)), dict(frac=(8, 10)), dict(frac=(1, 3)), dict(min_members=2, frac=(1, 3))]  # test_gpu_fold.RULES
REFUSALS = ("fold into its own input", "fold of top output (not ascending)", "fold with a target beyond the last group", "fetch_members of hits without members",
            "fetch_norms with a range outside the targets", "search_counted with queries of the other engine", "search_counted into hits of the other engine",
            "index_build_counted of foreign sets", "window_sets with window == 0 and count == 0")
WEIGHTED_WORK = GP.WEIGHTED_WORK  # the postings the queries of one search meet together (the weights' reference walks them in Python integers)
SETS_KINDS = GP.SETS_KINDS + ("windows",)
HITS_KINDS = ("search", "search_counted", "fold", "top", "neighbors", "neighbors_counted", "hits_load")
PAYLOADS = ("none", "totals", "weights", "members")
FORMULAS = ("cosine", "angular_similarity", "weighted_jaccard", "bray_curtis", "weighted_containment")
STRAND = 0x80000000


def seeds(block):
    return [BASE + PER_BLOCK * block + i for i in range(PER_BLOCK)]


def fbits(x):
    """a float64 array as its bit patterns, every NaN the same one: what AP.same compares (exactly, NaN equal to NaN)"""
    x = np.array(x, F64)
    x[np.isnan(x)] = np.nan
    return x.view(U64)


def payload(h):
    return "members" if h["has_members"] else "weights" if h["has_weights"] else "totals" if h["has_total"] else "none"


def rows_of(offsets):
    return np.repeat(np.arange(len(offsets) - 1, dtype=I64), np.diff(offsets).astype(I64))


def ascending(h):
    """whether every row lists its targets strictly ascending (what bsk_hits_fold asks of its input)"""
    t, r = h["target"].astype(I64), rows_of(h["offsets"])
    return bool(((t[1:] > t[:-1]) | (r[1:] != r[:-1])).all())


# ---- the sketch step's tuples ----
def standin_tuples(step):
    """(offsets, hash, pos or None) a sketch of the reads might give, without an engine: AP.standin_values per read; the minimizers with
    ascending positions, every third one on the reverse strand.  On the device the tuples are the result's own (BatchResult.fetch)."""
    vals = AP.standin_values(step)
    offs = np.concatenate([[0], np.cumsum([len(v) for v in vals])]).astype(U64)
    hash_ = np.concatenate(vals + [np.zeros(0, U64)]).astype(U64)
    if step["sketch"] != "minimizer":
        return offs, hash_, None
    j = np.arange(len(hash_), dtype=I64) - np.repeat(offs[:-1].astype(I64), np.diff(offs).astype(I64))
    return offs, hash_, (2 * j + j // 5).astype(U32) | np.where(j % 3 == 0, U32(STRAND), U32(0)).astype(U32)


def values_of(tuples):
    o = tuples[0].astype(I64)
    return [tuples[1][o[i]:o[i + 1]] for i in range(len(o) - 1)]


# ---- the references behind the model, computed once per operands ----
_searches, _weights, _records, _norms = {}, {}, {}, {}


def _key(t, c=None):
    return (AP.digest(t[0], t[1], c), len(t[0]), len(t[1]), c is None)


def ref_search(t, q, thr):
    key = (_key(t), _key(q), thr)
    if key not in _searches:
        _searches[key] = SR.ref_search(t[0], t[1], q[0], q[1], *thr) + (SR.posting_sums(t[0], t[1], q[0], q[1]),)
    return _searches[key]


def ref_weights(t, tc, q, qc, offsets, target):
    key = (_key(t, tc), _key(q, qc), AP.digest(offsets, target))
    if key not in _weights:
        _weights[key] = SW.ref_weights(SW.postings(t[0], t[1], tc), q[0], q[1], qc, offsets, target)
    return _weights[key]


def norms_of(t):
    """(sumsq, totals) of sets (offsets, values, counts or None): bsk_sets_sumsq and bsk_sets_totals"""
    key = _key(t, t[2])
    if key not in _norms:
        _norms[key] = (GP.sumsq_of(t), CN.ref_totals(t))
    return _norms[key]


def index_record(t, cnt):
    """everything an index of the targets t (counts cnt, None: an index without counts) can be asked: bsk_index_counted, bsk_index_info --
    the directory's figures by search_cases.directory, device_bytes as search.hip adds its arrays up --, bsk_index_fetch_norms and the
    owner's target_sizes"""
    key = _key(t, cnt)
    if key not in _records:
        T, P = AP.n_sets(t), AP.n_values(t)
        d = SR.directory(t[1])
        U, nb = d["n_distinct"], 1 << d["bits"]
        size = max(U, 1) * 8 + (U + 1) * 4 + max(P, 1) * 4 + (nb + 1) * 4 + max(T, 1) * 4
        if cnt is not None:
            size += max(P, 1) * 4 + 2 * max(T, 1) * 8  # (test_counted_index_equals_plain_index: the postings' counts and both norms)
        sumsq, totals = norms_of((t[0], t[1], cnt))
        _records[key] = dict(counted=cnt is not None, n_targets=T, n_postings=P, n_distinct=U, max_bucket=d["max_bucket"], device_bytes=size, sumsq=sumsq, totals=totals,
                           target_sizes=np.diff(t[0]).astype(U64))
    return dict(_records[key])


def hits_of(n_queries, offsets, target, shared, total=None, dot=None, min_sum=None, members=None):
    """everything the device can be asked about a bsk_hits"""
    return dict(n_queries=int(n_queries), n_hits=int(offsets[-1]), offsets=offsets, target=target, shared=shared, has_total=total is not None, has_weights=dot is not None,
                has_members=members is not None, total=total, dot=dot, min_sum=min_sum, members=members)


def fold_runs(h, go):
    """the (row, group) runs bsk_hits_fold finds before its rule: the plan's runs="""
    g = np.searchsorted(np.asarray(go, I64), h["target"].astype(I64), side="right") - 1
    return len(np.unique(rows_of(h["offsets"]) * (len(go) + 1) + g))


# ---- the owners' formulas, from the exact integers, in the docstrings' operation order ----
def plain_formulas(h, qs, ts):
    """Hits.containment() and Hits.jaccard() -> their bit patterns"""
    with np.errstate(all="ignore"):
        s, q = h["shared"].astype(F64), qs[rows_of(h["offsets"])].astype(F64)
        if h["has_total"]:
            jac = s / h["total"].astype(F64)
        else:
            jac = s / (q + ts[h["target"].astype(I64)].astype(F64) - s)
        return dict(containment=fbits(s / q), jaccard=fbits(jac))


def weighted_formulas(h, norms, plain_targets):
    """Hits.cosine() and its kin of weighted hits with the norms (sumsq_a, sumsq_b, totals_a, totals_b) of the two operands"""
    i, j = rows_of(h["offsets"]), h["target"].astype(I64)
    dt, ms, qa, qb, ta, tb = h["dot"], h["min_sum"], norms[0][i], norms[1][j], norms[2][i], norms[3][j]
    top = U64(MAX64)
    with np.errstate(all="ignore"):
        den = np.sqrt(qa.astype(F64)) * np.sqrt(qb.astype(F64))
        cos = np.divide(dt.astype(F64), den, out=np.zeros(dt.shape, F64), where=den != 0)
        cos[(dt == top) | (qa == top) | (qb == top)] = np.nan
        ang = 1.0 - 2.0 * np.arccos(np.minimum(cos, 1.0)) / np.pi
        m = ms.astype(F64)
        den = ta.astype(F64) + tb.astype(F64) - m
        wj = np.divide(m, den, out=np.zeros_like(m), where=den != 0)
        den = ta.astype(F64) + tb.astype(F64)
        bc, nz = np.zeros_like(m), den != 0
        bc[nz] = 1.0 - 2.0 * m[nz] / den[nz]
        wc = "undefined"
        if plain_targets:
            wc = np.divide(dt.astype(F64), ta.astype(F64), out=np.zeros(dt.shape, F64), where=ta != 0)
            wc[dt == top] = np.nan
            wc = fbits(wc)
    return dict(cosine=fbits(cos), angular_similarity=fbits(ang), weighted_jaccard=fbits(wj), bray_curtis=fbits(bc), weighted_containment=wc)


# ---- the model: one method per thing the library decides; a sabotage overrides one ----
class Model(GP.Model):
    name = "the references"
    kinds = ()

    def windows(self, tuples, p):
        return WN.windows_model(tuples[0], tuples[1], tuples[2], p.get("window", 0), p.get("step", 0), p.get("count", 0), p["scale"])

    def build_counts(self, t, stale):
        """the counts bsk_index_build_counted reads of its targets (stale: what the counts array of uncounted sets still holds)"""
        return t[2]

    def query_counts(self, q, stale):
        """... and the payload pass of bsk_index_search_counted of its queries"""
        return q[2]

    def core(self, st, core):
        """the targets and counts a handle of this index answers with"""
        return core["t"], core["cnt"]

    def close_index(self, st, x):
        """the handles that die with x"""
        return [x]

    def fold(self, h, go, min_members, frac):
        return WN.fold_model(h["offsets"], h["target"], h["shared"], go, min_members, frac)

    def bound(self, st, sid, snapshot, gen):
        """the sets a late formula takes its norms from: the operand as the call saw it, or "stale" when it was written or closed since"""
        return snapshot if st.gen.get(sid, 0) == gen else "stale"


def _resized(x, n, fill):
    return np.resize(np.concatenate([x, np.full(1, fill, x.dtype)]), n).astype(x.dtype)


class QueryStaleCounts(Model):
    name = "1 the payload pass reads the stale counts of an uncounted query (qs->counts without the qs->counted test)"
    kinds = ("search_counted",)

    def query_counts(self, q, stale):
        return _resized(stale, AP.n_values(q), 1) if q[2] is None and stale is not None else q[2]


class TargetStaleCounts(Model):
    name = "2 bsk_index_build_counted reads the stale counts of uncounted targets: a counted index of sets without counts"
    kinds = ("index",)

    def build_counts(self, t, stale):
        return _resized(stale, AP.n_values(t), 1) if t[2] is None and stale is not None else t[2]


class FoldLeavesWeights(Model):
    name = "3 a fold into weighted hits leaves has_weights set"
    kinds = ("fold",)

    def hits_after(self, before, new, kind):
        if kind == "fold" and before is not None and before["has_weights"]:
            return dict(new, has_weights=True, dot=_resized(before["dot"], new["n_hits"], 0), min_sum=_resized(before["min_sum"], new["n_hits"], 0))
        return new


class SearchLeavesMembers(Model):
    name = "4 a search into folded hits leaves has_members set"
    kinds = ("search", "search_counted")

    def hits_after(self, before, new, kind):
        if kind in self.kinds and before is not None and before["has_members"]:
            return dict(new, has_members=True, members=_resized(before["members"], new["n_hits"], 0))
        return new


class TopLeavesMembers(SearchLeavesMembers):
    name = "5 a top or a neighbours call into folded hits leaves has_members set"
    kinds = ("top", "neighbors", "neighbors_counted")


class FractionOfTheHits(Model):
    name = "6 a group's size in the fraction rule is its hit count: the rule keeps every group"
    kinds = ("fold",)

    def fold(self, h, go, min_members, frac):
        return WN.fold_model(h["offsets"], h["target"], h["shared"], go, min_members, None)


class FractionRounded(Model):
    name = "7 the fraction rule divides first: members >= floor(num * size / den)"
    kinds = ("fold",)

    def fold(self, h, go, min_members, frac):
        return WN.fold_brute(h["offsets"], h["target"], h["shared"], go, min_members, frac, wrong="fraction_rounded")


class FoldAcrossRows(Model):
    name = "8 fold lets a group's run continue across a row boundary: the next row's hits of that group land in this row"
    kinds = ("fold",)

    def fold(self, h, go, min_members, frac):
        o, t, s = h["offsets"].astype(I64), h["target"].astype(I64), h["shared"].astype(I64)
        g, row = np.searchsorted(np.asarray(go, I64), t, side="right") - 1, rows_of(o)
        for k in range(1, len(t)):
            if g[k] == g[k - 1] and row[k] != row[k - 1]:
                row[k:][row[k:] == row[k]] = row[k - 1]  # (the run's row is its head's)
        order = np.lexsort((t, row))
        no = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=len(o) - 1))]).astype(U64)
        uniq = np.ones(len(t), bool)
        tt, rr = t[order], row[order]
        uniq[1:] = (tt[1:] != tt[:-1]) | (rr[1:] != rr[:-1])
        if not uniq.all():  # (the same target twice in one row: beyond the model, and different anyway)
            return no, t[order].astype(U32), s[order].astype(U32), np.zeros(len(t), U32)
        return WN.fold_model(no, tt, s[order], go, min_members, frac)


class IndexFollowsItsSource(Model):
    name = "9 an index follows its source sets: a search after they were overwritten answers with the new sets"
    kinds = ("search", "search_counted", "attach", "close_index")

    def core(self, st, core):
        src = st.objs.get(core["src"])
        if src is None or st.gen.get(core["src"], 0) == core["src_gen"]:
            return core["t"], core["cnt"]
        return (src[0], src[1]), (src[2] if core["cnt"] is not None else None)


class AttachedDiesWithTheFirst(Model):
    name = "10 an attached handle dies with the handle it was attached from"
    kinds = ("close_index",)

    def close_index(self, st, x):
        return [i for i, v in st.idx.items() if v["core"] == st.idx[x]["core"]]


class WindowsFirstAtW(Model):
    name = "11 window sets: the first window of a position p is 0 up to p == W (window_cases' misreading first_at_w)"
    kinds = ("windows",)

    def windows(self, tuples, p):
        return WN.windows_brute(tuples[0], tuples[1], tuples[2], p.get("window", 0), p.get("step", 0), p.get("count", 0), p["scale"], wrong="first_at_w")


class WindowsDropTheLast(Model):
    name = "12 window sets: a sequence's last window is dropped (window_cases' misreading last_window_dropped)"
    kinds = ("windows",)

    def windows(self, tuples, p):
        return WN.windows_brute(tuples[0], tuples[1], tuples[2], p.get("window", 0), p.get("step", 0), p.get("count", 0), p["scale"], wrong="last_window_dropped")


class NormsFollowTheOperand(Model):
    name = "13 a late formula takes its norms from the operand OBJECT: the call's dot and min_sum with the norms of what was written there since"
    kinds = ("end",)

    def bound(self, st, sid, snapshot, gen):
        return st.objs.get(sid, st.fsets.get(sid, "stale"))


SABOTAGES = (QueryStaleCounts, TargetStaleCounts, FoldLeavesWeights, SearchLeavesMembers, TopLeavesMembers, FractionOfTheHits, FractionRounded, FoldAcrossRows,
             IndexFollowsItsSource, AttachedDiesWithTheFirst, WindowsFirstAtW, WindowsDropTheLast, NormsFollowTheOperand)


# ---- the interpreter ----
class State(GP.State):
    """GP's state and: the sketch step's tuples; per sets object its write generation (gen) and, for window objects, their group_offsets
    (groups); the sets on the second engine (fsets); the indexes (cores: targets, counts, source; idx: handle -> core and engine); per hits
    object what the owner knows besides the arrays (hmeta: engine, the operands' sizes, the index it searched, what its formulas are bound to)"""

    def __init__(self, model, tuples=None):
        GP.State.__init__(self, model, None if tuples is None else values_of(tuples))
        self.tuples = tuples
        self.groups, self.gen, self.fsets, self.cores, self.idx, self.hmeta = {}, {}, {}, {}, {}, {}
        self.shape, self.concrete = {}, []  # per sets object of window lineage the token of its set number (it follows the tuples); the steps as they ran

    def sets(self, i):
        return self.objs[i] if i in self.objs else self.fsets[i]

    def touch(self, i):
        self.gen[i] = self.gen.get(i, 0) + 1

    def index_record(self, x):
        t, cnt = self.model.core(self, self.cores[self.idx[x]["core"]])
        return index_record(t, cnt)

    def formulas(self, i):
        """what the owner of hits i answers at the end: containment() and jaccard() where it knows the sets' sizes, the weighted formulas
        where the hits carry weights"""
        h, m = self.hits[i], self.hmeta[i]
        out = dict(plain=None, weighted=None)
        if m["qs"] is not None:
            out["plain"] = plain_formulas(h, m["qs"], m["ts"])
        if h["has_weights"]:
            b = m["bound"]
            sets = [self.model.bound(self, sid, snap, gen) for sid, snap, gen in b["sets"]]
            if any(isinstance(x, str) for x in sets):
                out["weighted"] = "stale"
            elif b["handle"] is not None and b["handle"] not in self.idx:
                out["weighted"] = "closed"  # (the index's norms are fetched through the handle of the call, when a formula first asks)
            elif b["limit"] != 0:
                out["weighted"] = "limit"
            else:
                na = norms_of(sets[0])
                nb = b["index"] if b["index"] is not None else norms_of(sets[1])
                try:
                    out["weighted"] = weighted_formulas(h, (na[0], nb[0], na[1], nb[1]), b["plain_targets"])
                except IndexError:
                    out["weighted"] = "IndexError"  # (a sabotaged model only: norms of fewer sets than the hits have rows)
        return out

    def end(self):
        return dict(pool=dict(self.objs), groups=dict(self.groups), foreign=dict(self.fsets), indexes={x: self.index_record(x) for x in self.idx},
                    hits={i: dict(h, **self.formulas(i)) for i, h in self.hits.items()})


def _sets_after(st, step, rec):
    """the side tables after a sets-making step"""
    out, k = step["out"], step["kind"]
    a, b = st.shape.get(step.get("a")), st.shape.get(step.get("b"))
    st.shape.pop(out, None)
    token = (k, len(st.concrete)) if k == "windows" else (a or b) if k in ("op", "op_counted") else a if k in ("filter", "bottom") else None
    if token is not None and step.get("keep", True):
        st.shape[out] = token  # (as many sets as the window object it comes from: a number that follows the tuples, not the program)
    st.groups.pop(out, None)
    if step.get("into"):
        st.touch(out)
    if not step.get("keep", True):
        st.touch(out)
    elif step["kind"] == "windows":
        st.groups[out] = rec["group_offsets"]


def _sets_step(st, step):
    k, out = step["kind"], step["out"]
    if k == "sketch" and st.tuples is None:
        st.tuples = standin_tuples(step)
        st.read_values = values_of(st.tuples)
    if k != "windows":
        rec = GP._sets_step(st, step)
    else:
        before, stale = st.objs.get(out), st.stale.get(out)
        go, so, vals, cnts = st.model.windows(st.tuples, step)
        rec = AP._sets_record(st, step, (so, vals, cnts if step["counted"] else None), "bsk_result_sets_windows", [])
        rec["sumsq"] = st.model.sumsq((rec["offsets"], rec["values"], rec["counts"]))
        rec["group_offsets"] = go
        held = None if before is None else before[2] if before[2] is not None else stale
        if rec["counts"] is None and held is not None and step.get("keep", True):
            st.stale[out] = held
        else:
            st.stale.pop(out, None)
    _sets_after(st, step, rec)
    return rec


def _foreign_record(t):
    return dict(n_sets=AP.n_sets(t), n_values=AP.n_values(t), offsets=t[0], values=t[1], counted=t[2] is not None, counts=t[2], totals=CN.ref_totals(t), sumsq=GP.sumsq_of(t))


def _touched(st, step):
    """the objects a refused call names, as they must still be"""
    return dict(sets={i: st.sets(i) for i in dict.fromkeys(step[x] for x in ("a", "sslot") if step.get(x) is not None)},
                hits={i: st.hits[i] for i in dict.fromkeys(step[x] for x in ("hits", "hslot") if step.get(x) is not None)},
                indexes={i: st.index_record(i) for i in [step.get("x")] if i is not None})


def compute(st, step):
    """what a step of a kind that makes no sets must yield (the state is not changed)"""
    M, k = st.model, step["kind"]
    if k == "refused":
        return dict(rc="ERR_ARG", **_touched(st, step))
    if k == "copy":
        return dict(_foreign_record(st.objs[step["a"]]), operands=st.snap([step["a"]]))
    if k == "close_sets":
        return dict(closed=step["a"])
    if k == "index":
        t = st.objs[step["a"]]
        cnt = M.build_counts(t, st.stale.get(step["a"])) if step["counted"] else None
        return dict(index_record((t[0], t[1]), cnt), operands=st.snap([step["a"]]))
    if k == "attach":
        return st.index_record(step["x"])
    if k == "close_index":
        gone = M.close_index(st, step["x"])
        return dict(closed=step["x"], siblings={i: st.index_record(i) for i, v in st.idx.items() if v["core"] == st.idx[step["x"]]["core"] and i not in gone})
    before = st.hits.get(step["slot"])
    if k in ("search", "search_counted"):
        t, cnt = M.core(st, st.cores[st.idx[step["x"]]["core"]])
        q = st.sets(step["q"])
        thr = (step["min_shared"], step["min_query_cov"], step["min_target_cov"])
        o, tg, s, sums = ref_search(t, q, thr)
        extra = dict(n_large_queries=int((sums > SR.SR_CAP).sum()))
        d = m = None
        if k == "search_counted":
            d, m = ref_weights(t, cnt, q, M.query_counts(q, st.stale.get(step["q"])), o, tg)
            extra["plan_tail"] = SW.plan_tail(sums, q[0], o)
        new = M.hits_after(before, hits_of(AP.n_sets(q), o, tg, s, None, d, m), k)
        return dict(new, operands={step["q"]: q}, index=st.index_record(step["x"]), **extra)
    if k == "fold":
        h = st.hits[step["hits"]]
        o, t, s, mem = M.fold(h, step["groups"], step["rule"].get("min_members", 1), step["rule"].get("frac"))
        new = M.hits_after(before, hits_of(h["n_queries"], o, t, s, members=mem), k)
        return dict(new, n_large_queries=0, figures=(len(step["groups"]) - 1, fold_runs(h, step["groups"]), int(o[-1])), input=h)
    if k == "top":
        h = st.hits[step["hits"]]
        o, t, s = M.top((h["offsets"], h["target"], h["shared"]), step["n"])
        return dict(M.hits_after(before, hits_of(h["n_queries"], o, t, s), k), input=h)
    if k == "hits_load":
        return M.hits_after(before, hits_of(len(step["offsets"]) - 1, step["offsets"], step["target"], step["shared"], step["total"]), k)
    assert k in ("neighbors", "neighbors_counted"), k
    a, b = st.objs[step["a"]], st.objs[step["b"]]
    if k == "neighbors":
        sh, tt = GP.plain_compare(a, b, step["limit"])
        dt = ms = None
    else:
        sh, tt, dt, ms = M.weights(a, M.counts_read(a, st.stale.get(step["a"])), b, M.counts_read(b, st.stale.get(step["b"])), step["limit"])
    o, t, s, tot, d, m = M.kept(sh, tt, dt, ms, GP.rule_of(step))
    tiles, skipped = NC.expected_tiles(AP.n_sets(a), AP.n_sets(b), step["upper"], CMP)
    new = M.hits_after(before, hits_of(AP.n_sets(a), o, t, s, tot, d, m), k)
    return dict(new, tiles=tiles, skipped=skipped, operands=st.snap([step["a"], step["b"]]))


HITS_FIELDS = tuple(hits_of(0, np.zeros(1, U64), None, None))


def commit(st, step, rec):
    """the state after a step of a kind that makes no sets, whose record is rec"""
    k = step["kind"]
    if k == "copy":
        st.fsets[step["out"]] = st.objs[step["a"]]
    elif k == "close_sets":
        a = step["a"]
        st.touch(a)
        st.groups.pop(a, None)
        st.shape.pop(a, None)
        st.stale.pop(a, None)
        if a in st.objs:
            del st.objs[a], st.maker[a]
        else:
            del st.fsets[a]
    elif k == "index":
        a = step["a"]
        t = st.objs[a]
        cnt = None if not rec["counted"] else t[2] if t[2] is not None else _resized(st.stale[a], AP.n_values(t), 1)  # (uncounted and yet counted: a sabotaged model)
        st.cores[step["out"]] = dict(t=(t[0], t[1]), cnt=cnt, src=a, src_gen=st.gen.get(a, 0), groups=st.groups.get(a), first=step["out"])
        st.idx[step["out"]] = dict(core=step["out"], eng=0)
    elif k == "attach":
        st.idx[step["out"]] = dict(core=st.idx[step["x"]]["core"], eng=1 - st.idx[step["x"]]["eng"])
    elif k == "close_index":
        for i in [i for i, v in st.idx.items() if v["core"] == st.idx[step["x"]]["core"] and i != step["x"] and i not in rec["siblings"]] + [step["x"]]:
            del st.idx[i]
    elif k in HITS_KINDS:
        slot = step["slot"]
        st.hits[slot] = {f: rec[f] for f in HITS_FIELDS}
        meta = dict(eng=step["eng"], qs=None, ts=None, nt=None, core=None, bound=None, kind=k, pure=k == "hits_load" or (k in ("top", "fold") and st.hmeta[step["hits"]]["pure"]))
        if k in ("search", "search_counted"):
            core = st.cores[st.idx[step["x"]]["core"]]
            q = st.sets(step["q"])
            meta.update(qs=np.diff(q[0]).astype(U64), ts=np.diff(core["t"][0]).astype(U64), nt=AP.n_sets(core["t"]), core=st.idx[step["x"]]["core"])
            if k == "search_counted":
                meta["bound"] = dict(sets=[(step["q"], q, st.gen.get(step["q"], 0))], limit=0, index=(rec["index"]["sumsq"], rec["index"]["totals"]), handle=step["x"],
                                     plain_targets=not rec["index"]["counted"])
        elif k in ("neighbors", "neighbors_counted"):
            a, b = st.objs[step["a"]], st.objs[step["b"]]
            meta.update(qs=np.diff(a[0]).astype(U64), ts=np.diff(b[0]).astype(U64), nt=AP.n_sets(b))
            if k == "neighbors_counted":
                meta["bound"] = dict(sets=[(step[x], st.objs[step[x]], st.gen.get(step[x], 0)) for x in ("a", "b")], limit=step["limit"], index=None, handle=None, plain_targets=None)
        elif k == "top":
            src = st.hmeta[step["hits"]]
            meta.update(qs=src["qs"], ts=src["ts"], nt=src["nt"])
        elif k == "fold":
            meta.update(qs=st.hmeta[step["hits"]]["qs"], ts=np.diff(step["groups"]).astype(U64), nt=len(step["groups"]) - 1)
            if meta["qs"] is None:
                meta["ts"] = None
        else:
            meta["nt"] = step["n"]
        st.hmeta[slot] = meta


def resolve(st, step):
    """the step with the group offsets that follow the state spelled out: a reduce by the operand's "own" group_offsets or of "all" its sets
    into one, a fold by the "window" object's group_offsets or by runs given as fractions of the hits' target number"""
    k = step["kind"]
    if k == "reduce" and isinstance(step["groups"], str):
        return dict(step, groups=st.groups[step["a"]].copy() if step["groups"] == "own" else np.array([0, AP.n_sets(st.objs[step["a"]])], U64))
    if k == "fold" and not isinstance(step["groups"], np.ndarray):
        m = st.hmeta[step["hits"]]
        if step["groups"] == "window":
            return dict(step, groups=st.cores[m["core"]]["groups"].copy())
        lead, cuts, trail = step["groups"]
        inner = np.sort(np.minimum(np.floor(np.asarray(cuts, F64) * (m["nt"] + 1)).astype(I64), m["nt"]))
        return dict(step, groups=np.concatenate([[0] * lead, inner, [m["nt"]] * trail]).astype(U64))
    return step


def apply(st, step):
    """one step on the model's state -> what the step must yield"""
    step = resolve(st, step)
    st.concrete.append(step)
    if step["kind"] in SETS_KINDS:
        return _sets_step(st, step)
    rec = compute(st, step)
    commit(st, step, rec)
    return rec


def run_model(program, model=None, tuples=None):
    """-> one record per step and a last one: every object alive at the end, the hits with their formulas.  tuples: (offsets, hash, pos) of
    the sketch step's result (from the device; None: standin_tuples)"""
    return run_concrete(program, model, tuples)[0]


def run_concrete(program, model=None, tuples=None):
    """run_model and the steps as they ran: the group offsets that follow the state spelled out (resolve)"""
    st = State(model or Model(), tuples)
    records = [apply(st, step) for step in program]
    records.append(st.end())
    return records, st.concrete


def _replay(st, step, rec):
    """the state after a step whose record is known"""
    step = resolve(st, step)
    st.concrete.append(step)
    k = step["kind"]
    if k not in SETS_KINDS:
        return commit(st, step, rec)
    if k == "sketch":
        st.sketch, st.tuples = step, standin_tuples(step)
        st.read_values = values_of(st.tuples)
    out = step["out"]
    before, stale = st.objs.get(out), st.stale.get(out)
    held = None if before is None else before[2] if before[2] is not None else stale
    if step.get("keep", True):
        st.objs[out], st.maker[out] = (rec["offsets"], rec["values"], rec["counts"]), None
    else:
        st.objs.pop(out, None), st.maker.pop(out, None)
    if rec["counts"] is None and held is not None and step.get("keep", True):
        st.stale[out] = held
    else:
        st.stale.pop(out, None)
    _sets_after(st, step, rec)


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
class _Gen(GP._Gen):
    def __init__(self, seed):
        AP._Gen.__init__(self, seed)
        self.st = State(Model())
        self.force_out = None

    def emit(self, step):
        rec = apply(self.st, step)
        self.steps.append(step)
        self.records.append(rec)
        self.made += rec.get("n_values", 0)
        return rec

    def out(self, step, operands):
        if self.force_out is not None and self.force_out in self.st.objs and self.force_out not in operands:
            step["out"], step["into"], step["made_by"] = self.force_out, True, self.st.maker.get(self.force_out)
            return step
        return AP._Gen.out(self, step, operands)

    def finish(self, step):
        rec = GP._Gen.finish(self, step)
        if not step.get("keep", True):
            self.st.touch(step["out"])
            self.st.groups.pop(step["out"], None)
        return rec

    def pick(self, ok=lambda i, t: True, exclude=()):
        """AP's pick among the objects whose set number the program fixes: what AP's own kinds pair by set number and cut into runs"""
        return AP._Gen.pick(self, lambda i, t: i not in self.st.shape and ok(i, t), exclude)

    def any_sets(self):
        """... or, one time in three, any live object: the window objects and what was made of them"""
        return self.choice(self.st.shape) if self.st.shape and self.rng.random() < 1 / 3 else self.pick()

    def small(self):
        """a live object of at most 40 sets: an operand of a neighbours call (its references walk every pair)"""
        return self.pick(lambda i, t: AP.n_sets(t) <= 40)

    def hslot(self, step, eng, becomes, exclude=()):
        """where hits go: a new object or, mostly, a live one of the engine -- by preference one whose payload is another than the new one"""
        st = self.st
        live = [i for i in st.hits if st.hmeta[i]["eng"] == eng and i not in exclude]
        other = [i for i in live if payload(st.hits[i]) != becomes]
        if live and self.rng.random() < 0.7:
            step["slot"], step["into"] = self.choice(other) if other and self.rng.random() < 0.85 else self.choice(live), True
        else:
            step["slot"], step["into"] = self.new_id("h"), False
        step["eng"], step["was"] = eng, payload(st.hits[step["slot"]]) if step["into"] else None
        return step


def _posting_work(core, q):
    return int(SR.posting_sums(core["t"][0], core["t"][1], q[0], q[1]).sum())


def _windows(g, into=None):
    rng, st = g.rng, g.st
    p = dict(WINDOWS[int(rng.integers(0, len(WINDOWS)))])
    step = dict(kind="windows", scale=int(rng.choice([1, 1, 3])), counted=bool(rng.random() < 0.5), **p)
    if into is not None and into not in st.shape and len([i for i in st.objs if i not in st.shape]) <= 2:
        into = None  # (two objects of a set number the program fixes stay: the operands of AP's kinds)
    elif into is None and len([i for i in st.objs if i not in st.shape]) > 2 and rng.random() < 0.55:
        made = [i for i in st.objs if st.maker.get(i) not in ("bsk_result_sets_windows", "bsk_sets_from_host", "bsk_sets_from_host_counted")]
        into = g.choice(made) if made and rng.random() < 0.7 else g.choice(st.objs)
    if into is not None:
        step["out"], step["into"], step["made_by"] = into, True, st.maker.get(into)
    else:
        step["out"], step["into"], step["made_by"] = g.new_id(), False, None
    return g.emit(step)


def _index(g, a=None, counted=None):
    rng, st = g.rng, g.st
    if a is None:
        win = [i for i in st.groups if AP.n_values(st.objs[i])]
        a = g.choice(st.stale) if st.stale and rng.random() < 0.35 else g.choice(win) if win and rng.random() < 0.4 else g.any_sets()
        if rng.random() < 0.3:  # the live object of the most values: posting sums beyond SR_CAP
            a = max(st.objs, key=lambda i: AP.n_values(st.objs[i]))
    counted = bool(rng.random() < 0.6) if counted is None else counted
    return g.emit(dict(kind="index", a=a, counted=counted, out=g.new_id("x"), stale=counted and a in st.stale, windows=a in st.groups))


def _copy(g, a=None):
    return g.emit(dict(kind="copy", a=a if a is not None else g.any_sets(), out=g.new_id("f")))


def _search(g, x=None, counted=None, q=None, big=False):
    """a search through handle x (None: any live one; none alive: nothing)"""
    rng, st = g.rng, g.st
    if x is None:
        if not st.idx:
            return None
        attached = [i for i, v in st.idx.items() if v["eng"] == 1]
        x = g.choice(attached) if attached and rng.random() < 0.5 else g.choice(st.idx)
    eng, core = st.idx[x]["eng"], st.cores[st.idx[x]["core"]]
    big = big or bool(rng.random() < 0.25)
    counted = bool(rng.random() < (0.8 if big else 0.65)) if counted is None else counted
    pool = st.fsets if eng else st.objs
    if not pool:
        return None
    if q is None:
        ids = list(pool)
        if big:  # the query that meets the most postings: the large path, the chunks of the payload pass
            q = max(ids, key=lambda i: int(SR.posting_sums(core["t"][0], core["t"][1], pool[i][0], pool[i][1]).max(initial=0)))
        elif counted and not eng and st.stale and rng.random() < 0.5:
            q = g.choice(st.stale)
        else:
            q = core["src"] if core["src"] in pool and rng.random() < 0.25 else g.choice(ids) if eng else g.any_sets()
    if _posting_work(core, pool[q]) > WEIGHTED_WORK:
        fits = [i for i in pool if _posting_work(core, pool[i]) <= WEIGHTED_WORK]
        if not fits:
            return None
        q = g.choice(fits)
    qc, tc = float(COVERS[int(rng.integers(0, len(COVERS)))]), float(COVERS[int(rng.integers(0, len(COVERS)))])
    step = dict(kind="search_counted" if counted else "search", x=x, q=q, min_shared=int(MIN_SHARED[int(rng.choice(3, p=[0.6, 0.25, 0.15]))]), min_query_cov=qc,
                min_target_cov=tc if rng.random() < 0.5 else 0.0, stale_q=counted and q in st.stale, src_gone=st.gen.get(core["src"], 0) != core["src_gen"],
                attached=x != core["first"], first_closed=core["first"] not in st.idx)
    return g.emit(g.hslot(step, eng, "weights" if counted else "none"))


def _fold(g, src=None):
    rng, st = g.rng, g.st
    ok = [i for i in st.hits if st.hmeta[i]["kind"] != "top"]  # (a top's rows come by shared count: whether they ascend follows the values)
    if src is None:
        if not ok:
            return None
        win = [i for i in ok if st.hmeta[i]["core"] is not None and st.cores[st.hmeta[i]["core"]]["groups"] is not None]
        weighted = [i for i in ok if st.hits[i]["has_weights"]]
        r = rng.random()
        src = g.choice(win) if win and r < 0.5 else g.choice(weighted) if weighted and r < 0.75 else g.choice(ok)
    h, m = st.hits[src], st.hmeta[src]
    groups = st.cores[m["core"]]["groups"] if m["core"] is not None else None
    window_fold = groups is not None and rng.random() < 0.85
    groups = "window"
    if not window_fold:  # random runs over the targets -- cuts as fractions of their number --, with empty groups at the start, in the middle and at the end
        cuts = [float(x) for x in np.round(rng.random(int(rng.integers(0, 13))), 3)] + ([0.5, 0.5] if rng.random() < 0.3 else [])
        groups = (1 + int(rng.integers(0, 2)), cuts, 1 + int(rng.integers(0, 3)) // 2)
    step = dict(kind="fold", hits=src, groups=groups, rule=dict(RULES[int(rng.integers(0, len(RULES)))]), window_fold=bool(window_fold), input_kind=m["kind"])
    return g.emit(g.hslot(step, m["eng"], "members", exclude=(src,)))


def _top(g, src=None):
    rng, st = g.rng, g.st
    if not st.hits:
        return None
    folded = [i for i, h in st.hits.items() if h["has_members"] and h["n_hits"]]
    src = src if src is not None else g.choice(folded) if folded and rng.random() < 0.6 else g.choice(st.hits)
    step = dict(kind="top", hits=src, n=int(TOP_NS[int(rng.random() < 0.65)]), input_kind=st.hmeta[src]["kind"])
    return g.emit(g.hslot(step, st.hmeta[src]["eng"], "none", exclude=(src,)))


def _neighbors(g, counted, a=None):
    rng, st = g.rng, g.st
    stale = [i for i in st.stale if AP.n_sets(st.objs[i]) <= 40]
    if a is None:
        a = g.choice(stale) if counted and stale and rng.random() < 0.4 else g.small()
    b = a if rng.random() < 1 / 3 else g.small()
    if a is None or b is None:
        return None
    limit = g.limit(a, b, WEIGHTED_WORK)  # (one that keeps the references' walk within the budget)
    whole = sum(AP.n_values(st.objs[x]) * AP.n_sets(st.objs[y]) for x, y in ((a, b), (b, a)))
    if whole <= WEIGHTED_WORK and rng.random() < 0.6:
        limit = 0  # whole sets: the weighted formulas are defined
    step = dict(kind="neighbors_counted" if counted else "neighbors", a=a, b=b, limit=limit, min_shared=int(MIN_SHARED[int(rng.integers(0, 3))]),
                min_jaccard=GP.MIN_JACCARD[int(rng.choice(len(GP.MIN_JACCARD), p=GP.JACCARD_WEIGHTS))], upper=bool(rng.random() < 0.3),
                stale=[i for i in dict.fromkeys((a, b)) if i in st.stale] if counted else [])
    return g.emit(g.hslot(step, 0, "weights" if counted else "totals"))


def _hits_load(g):
    rng = g.rng
    text, n, pairs = GP._graph(rng)
    o, t, s = GP.CL.csr(n, pairs)
    s = rng.integers(1, 10, len(t)).astype(U32)
    total = (s + rng.integers(0, 10, len(t)).astype(U32)).astype(U32) if rng.random() < 0.6 else None
    step = dict(kind="hits_load", graph=text, n=n, offsets=o, target=t, shared=s, total=total)
    return g.emit(g.hslot(step, int(rng.random() < 0.3), "totals" if total is not None else "none"))


def _attach(g, x=None):
    st = g.st
    firsts = [i for i, v in st.idx.items() if v["eng"] == 0]
    if x is None and not firsts:
        return None
    return g.emit(dict(kind="attach", x=x if x is not None else g.choice(firsts), out=g.new_id("x")))


def _close_index(g, x=None):
    st = g.st
    ok = [i for i, v in st.idx.items() if any(j != i and w["core"] == v["core"] for j, w in st.idx.items())]
    if x is None and not ok:
        return None
    firsts = [i for i in ok if st.cores[st.idx[i]["core"]]["first"] == i]
    return g.emit(dict(kind="close_index", x=x if x is not None else g.choice(firsts) if firsts and g.rng.random() < 0.8 else g.choice(ok)))


def _close_sets(g, a=None):
    """close a sets object on purpose: the source of a live index, the operand a weighted result is bound to, a foreign one"""
    rng, st = g.rng, g.st
    if a is None:
        bound = [sid for i, m in st.hmeta.items() if st.hits[i]["has_weights"] for sid, _, gen in m["bound"]["sets"] if st.gen.get(sid, 0) == gen]
        srcs = [c["src"] for c in st.cores.values() if st.gen.get(c["src"], 0) == c["src_gen"]]
        cands = [i for i in dict.fromkeys(bound + srcs) if i in st.fsets or (i in st.objs and len(st.objs) > 3)]
        if not cands:
            cands = list(st.fsets) if len(st.fsets) > 1 else []
        if not cands:
            return None
        a = g.choice(cands)
    return g.emit(dict(kind="close_sets", a=a))


def _overwrite(g, a):
    """write other sets into the live object a through `into`"""
    g.force_out = a
    try:
        kind = ("op", "reduce", "bottom", "windows")[int(g.rng.integers(0, 4))]
        return _windows(g, into=a) if kind == "windows" else AP._step(g, kind)
    finally:
        g.force_out = None


def _refused(g):
    """a call the library refuses before it takes the slot over; the slot and everything the call names must stay what they were"""
    rng, st = g.rng, g.st
    order = [REFUSALS[int(i)] for i in rng.permutation(len(REFUSALS))]
    order += [REFUSALS[7 + int(i)] for i in rng.permutation(2)]  # (these two fit any state)
    for what in order:  # the first one the live objects allow
        step = dict(kind="refused", what=what, a=None, sslot=None, hits=None, hslot=None, x=None, eng=0, groups=None)
        if what.startswith("fold") or what == "fetch_members of hits without members":
            pure = lambda i: st.hmeta[i]["pure"]  # noqa: E731  (hits that follow the program alone, not the sketch's values)
            ok = {"fold into its own input": lambda i, h: True, "fold of top output (not ascending)": lambda i, h: pure(i) and not ascending(h),
                  "fold with a target beyond the last group": lambda i, h: pure(i) and h["n_hits"] > 0 and ascending(h),
                  "fetch_members of hits without members": lambda i, h: not h["has_members"]}[what]
            fit = [i for i, h in st.hits.items() if ok(i, h)]
            if not fit and what in REFUSALS[1:3] and not [i for i in st.hits if pure(i)]:
                _hits_load(g)
                fit = [i for i, h in st.hits.items() if ok(i, h)]
            if not fit and "top output" in what:  # no such hits alive: the top(3) of hits whose best three do not come in target order, made first
                def unordered(h):
                    o, t, s = SR.ref_top(h["offsets"], h["target"], h["shared"], 3)
                    return not ascending(dict(offsets=o, target=t))
                srcs = [i for i, h in st.hits.items() if pure(i) and unordered(h)]
                if srcs:
                    src = g.choice(srcs)
                    g.emit(dict(kind="top", hits=src, n=3, input_kind=st.hmeta[src]["kind"], slot=g.new_id("h"), into=False, eng=st.hmeta[src]["eng"], was=None))
                    fit = [g.steps[-1]["slot"]]
            if not fit:
                continue
            src = step["hits"] = g.choice(fit)
            h, step["eng"] = st.hits[src], st.hmeta[src]["eng"]
            if what == "fold into its own input":
                step["hslot"], step["groups"] = src, np.array([0, int(h["target"].max(initial=0)) + 1], U64)
            elif what.startswith("fold"):
                top = int(h["target"].max(initial=0))
                step["groups"] = np.array([0, top + 1] if "top output" in what else [0, top // 2, top], U64)  # (the largest target equals the last offset)
                others = [i for i in st.hits if i != src and st.hmeta[i]["eng"] == step["eng"]]
                step["hslot"] = g.choice(others) if others and rng.random() < 0.7 else None
        elif what in ("fetch_norms with a range outside the targets", "search_counted with queries of the other engine", "search_counted into hits of the other engine"):
            if not st.idx:
                continue
            step["x"] = g.choice(st.idx)
            step["eng"] = st.idx[step["x"]]["eng"]
            pool = st.fsets if step["eng"] else st.objs
            if what == "search_counted into hits of the other engine":
                if not pool:
                    continue
                step["a"] = g.choice(pool)
            elif what.startswith("search_counted"):
                mine = [i for i in st.hits if st.hmeta[i]["eng"] == step["eng"]]
                step["hslot"] = g.choice(mine) if mine and rng.random() < 0.7 else None
        elif what == "window_sets with window == 0 and count == 0":
            step["sslot"] = g.choice(st.objs) if rng.random() < 0.7 else None
        else:
            assert what == "index_build_counted of foreign sets", what
            step["eng"] = int(bool(st.fsets) and rng.random() < 0.5)  # the engine that is asked; the sets are the other one's
            if step["eng"]:
                step["a"] = g.pick()
        return g.emit(step)
    raise AssertionError("no refusal fits")  # (the last two always do)


KINDS = ("op", "op_counted", "reduce", "filter", "bottom", "result_sets", "window_algebra", "windows", "copy", "close_sets", "index", "attach", "close_index", "search", "search_counted",
         "fold", "top", "neighbors", "neighbors_counted", "hits_load")
KIND_WEIGHTS = (0.03, 0.04, 0.02, 0.02, 0.02, 0.03, 0.04, 0.07, 0.03, 0.03, 0.09, 0.06, 0.03, 0.07, 0.11, 0.11, 0.07, 0.04, 0.06, 0.03)


def _step(g, kind):
    if kind in ("op", "op_counted", "reduce", "filter", "bottom", "result_sets"):
        return AP._step(g, kind) if g.pick() is not None else None
    if kind in ("search", "search_counted"):
        return _search(g, counted=kind == "search_counted")
    if kind in ("neighbors", "neighbors_counted"):
        return _neighbors(g, kind == "neighbors_counted")
    return dict(window_algebra=_window_algebra, windows=_windows, copy=_copy, close_sets=_close_sets, index=_index, attach=_attach, close_index=_close_index, fold=_fold, top=_top,
                hits_load=_hits_load)[kind](g)


def program(seed):
    return program_and_records(seed)[0]


def program_and_records(seed):
    """the program of a seed and run_model's records of it (the generator runs the model as it goes).  After the sources the calls come in
    short chains, each after a state the campaign exists for: an index whose source is then overwritten or closed and searched afterwards;
    a window object indexed, searched and the hits folded by its group_offsets; stale counts indexed or searched while they are there; an
    attached handle searched before and after the first one is closed; the queries of a weighted search overwritten before any formula."""
    g = _Gen(seed)
    rng, st = g.rng, g.st
    name, pool = AP._universe(rng)
    n = int(NS[int(rng.integers(0, len(NS)))])
    sketched = int(rng.integers(0, 4))
    counted = [bool(rng.random() < 0.5) for _ in range(4)]
    if len(set(counted)) == 1:  # at least one counted and one uncounted source
        counted[int(rng.integers(0, 4))] ^= True
    for which in range(4):
        ns = n if which < 3 else 1
        if which == sketched:
            whole = which == 3
            mini = bool(rng.random() < 0.5)
            g.emit(dict(kind="sketch", out=g.new_id(), sketch="minimizer" if mini else "nthash", k=15 if mini else 21, w=5 if mini else 0,
                        reads=AP._reads(rng, int(rng.integers(40, 65))), whole=whole, scale=int(rng.choice([1, 3])),
                        counted=counted[which], no_small=bool(rng.random() < 0.4), universe=name))
            continue
        sets, layout = AP._collection(rng, pool, name.startswith("dense"), AP._sizes(rng, ns, which == 3))
        offs, vals = SO.collection(sets)
        g.emit(dict(kind="load", out=g.new_id(), offsets=offs, values=vals, counts=AP._counts(rng, len(vals)) if counted[which] else None, layout=layout,
                    universe=name))
    sources = len(g.steps)
    todo = int(rng.integers(10, 17))
    left = lambda: todo - (len(g.steps) - sources)  # noqa: E731
    chain = lambda *calls: all(left() > 0 and call() is not None for call in calls)  # noqa: E731  (stops at the first call nothing alive fits)
    while left() > 0:
        if rng.random() < 0.11:
            _refused(g)
            continue
        kind = KINDS[int(rng.choice(len(KINDS), p=KIND_WEIGHTS))]
        before = len(g.steps)
        if _step(g, kind) is None:
            continue
        made, r = g.steps[-1], rng.random()
        if kind == "index":
            x, a = made["out"], made["a"]
            if made["windows"] and r < 0.7:  # a window object as targets: searched, and the hits folded by its own group_offsets
                chain(lambda: _search(g, x=x, big=rng.random() < 0.4), lambda: _fold(g, src=g.steps[-1]["slot"]), lambda: _top(g, src=g.steps[-1]["slot"]) if rng.random() < 0.4 else 0)
            elif r < 0.45:  # the source goes, the index stays
                chain(lambda: _overwrite(g, a) if rng.random() < 0.7 else _close_sets(g, a) if len(st.objs) > 3 else _overwrite(g, a), lambda: _search(g, x=x))
            elif r < 0.8 and AP.n_values(st.objs[a]) > SR.SR_CAP:  # one query that holds every value of the targets: the large path, the chunks of the payload pass
                chain(lambda: _union_of_all(g, a), lambda: _search(g, x=x, counted=True, q=g.steps[-1]["out"]) if g.steps[-1].get("keep", True) else None)
            elif r < 0.8:
                chain(lambda: _search(g, x=x, counted=True, big=True))
        elif kind == "attach":
            x, first = made["out"], made["x"]
            if not st.fsets or rng.random() < 0.3:
                chain(lambda: _copy(g))
            chain(lambda: _search(g, x=x), lambda: _close_index(g, first) if rng.random() < 0.6 and first in st.idx else 0, lambda: _search(g, x=x))
        elif kind == "windows" and r < 0.5 and made.get("keep", True) and made["out"] in st.objs:
            a = made["out"]
            if rng.random() < 0.3:
                chain(lambda: _reduce_own(g, a))
            else:
                chain(lambda: _index(g, a=a), lambda: _search(g, x=g.steps[-1]["out"], q=a if rng.random() < 0.3 else None), lambda: _fold(g, src=g.steps[-1]["slot"]))
        elif made["kind"] in SETS_KINDS and made.get("out") in st.stale and r < 0.6:  # stale counts: read while they are there
            a = made["out"]
            if rng.random() < 0.5:
                chain(lambda: _index(g, a=a, counted=True), lambda: _search(g, x=g.steps[-1]["out"], counted=True))
            elif [i for i, v in st.idx.items() if v["eng"] == 0]:
                chain(lambda: _search(g, x=g.choice([i for i, v in st.idx.items() if v["eng"] == 0]), counted=True, q=a))
        elif kind == "search_counted" and r < 0.45:  # the queries go before any formula was asked
            q = made["q"]
            if q in st.fsets or len(st.objs) <= 3 or rng.random() < 0.6:
                chain(lambda: _close_sets(g, q) if q in st.fsets else _overwrite(g, q))
            else:
                chain(lambda: _close_sets(g, q))
        elif kind == "fold" and r < 0.4:
            chain(lambda: _top(g, src=made["slot"]))
        assert len(g.steps) > before
    g.records.append(st.end())
    return g.steps, g.records


def _union_of_all(g, a):
    """one set: the union of all sets of a"""
    return g.finish(g.out(dict(kind="reduce", a=a, groups="all", m=1), (a,)))


def _reduce_own(g, a):
    """a window object reduced by its own group_offsets: the per-sequence sets again"""
    return g.finish(g.out(dict(kind="reduce", a=a, groups="own", m=1, own_groups=True), (a,)))


def _window_algebra(g):
    """set algebra with a window object, or with what was made of one, as an operand: with itself, with a one-set object, with another object
    of the same windows; bottom and filter_counts of it"""
    rng, st = g.rng, g.st
    if not st.shape:
        return None
    a = g.choice(st.shape)
    mates = [i for i, tok in st.shape.items() if tok == st.shape[a] and i != a]
    ones = [i for i, t in st.objs.items() if i not in st.shape and AP.n_sets(t) == 1]
    r = rng.random()
    if r < 0.2:
        return g.finish(g.out(dict(kind="bottom", window_operand=True, a=a, n=int(AP.BOTTOM_NS[int(rng.integers(0, 5))])), (a,)))
    if r < 0.35 and st.objs[a][2] is not None:
        return g.finish(g.out(dict(kind="filter", window_operand=True, a=a, lo=int(rng.integers(1, 3)), hi=None), (a,)))
    b = g.choice(mates) if mates and rng.random() < 0.6 else g.choice(ones) if ones and rng.random() < 0.7 else a
    if rng.random() < 0.5:
        return g.finish(g.out(dict(kind="op", window_operand=True, a=a, b=b, op=int(rng.choice(list(AP.SET_OPS)))), (a, b)))
    return g.finish(g.out(dict(kind="op_counted", window_operand=True, a=a, b=b, op=int(rng.choice(list(AP.COUNT_OPS)))), (a, b)))


# ---- the text of a program ----
def describe_step(i, s):
    k = s["kind"]
    if k == "reduce" and isinstance(s["groups"], str):
        return AP.describe_step(i, dict(s, groups=np.zeros(0, U64))).replace("[]", "its own group_offsets" if s["groups"] == "own" else "[0, n_sets]")
    if k in GP.SETS_KINDS:
        return AP.describe_step(i, s)
    into = " into %s (%s)" % (s.get("slot"), s["was"]) if s.get("into") and "slot" in s else ""
    eng = " on engine %d" % s["eng"] if s.get("eng") else ""
    if k == "windows":
        text = "%s = the sketch result's window_sets(%s, scale=%d, counted=%s)%s%s" % (s["out"], ", ".join("%s=%d" % (x, s[x]) for x in ("window", "step", "count") if x in s),
                                                                                      s["scale"], s["counted"], " into %s (made by %s)" % (s["out"], s["made_by"]) if s["into"] else "",
                                                                                      "; closed after the check" if not s.get("keep", True) else "")
    elif k == "copy":
        text = "%s = the second engine's sets_from_arrays(fetch of %s)" % (s["out"], s["a"])
    elif k == "close_sets":
        text = "%s.close()" % s["a"]
    elif k == "index":
        text = "%s = %s.index%s()%s%s" % (s["out"], s["a"], "_counted" if s["counted"] else "", "; stale counts in it" if s["stale"] else "", "; window sets" if s["windows"] else "")
    elif k == "attach":
        text = "%s = %s.attach(the other engine)" % (s["out"], s["x"])
    elif k == "close_index":
        text = "%s.close()" % s["x"]
    elif k in ("search", "search_counted"):
        text = "%s = %s.%s(%s, min_shared=%d, min_query_cov=%s, min_target_cov=%s)%s%s%s%s" % (
            s["slot"], s["x"], k, s["q"], s["min_shared"], s["min_query_cov"], s["min_target_cov"], into, eng, "; stale counts in the queries" if s["stale_q"] else "",
            "; the index's source is gone" if s["src_gone"] else "")
    elif k == "fold":
        text = "%s = %s.fold(%s, %s)%s%s   [%s made by %s]" % (s["slot"], s["hits"], "the window object's group_offsets" if s["window_fold"] else s["groups"].tolist() if isinstance(s["groups"], np.ndarray) else
                                                             "%d x [0] + n_targets x %s + %d x [n_targets]" % s["groups"],
                                                             s["rule"], into, eng, s["hits"], s["input_kind"])
    elif k == "top":
        text = "%s = %s.top(%d)%s%s   [%s made by %s]" % (s["slot"], s["hits"], s["n"], into, eng, s["hits"], s["input_kind"])
    elif k in ("neighbors", "neighbors_counted"):
        text = "%s = %s.%s(%s, limit=%d, min_shared=%d, min_jaccard=%r, upper=%s)%s%s" % (s["slot"], s["a"], k, s["b"], s["limit"], s["min_shared"], s["min_jaccard"], s["upper"],
                                                                                       into, "; stale counts in %s" % ", ".join(s["stale"]) if s["stale"] else "")
    elif k == "hits_load":
        text = "%s = hits_from_arrays(%s; %d hits, crc %s, %s)%s%s" % (s["slot"], s["graph"], len(s["target"]), AP.digest(s["offsets"], s["target"], s["shared"], s["total"]),
                                                                     "with totals" if s["total"] is not None else "no totals", into, eng)
    else:
        text = "REFUSED (%s): sets=%s sets slot=%s hits=%s hits slot=%s index=%s groups=%s%s" % (s["what"], s["a"], s["sslot"], s["hits"], s["hslot"], s["x"],
                                                                                             None if s["groups"] is None else s["groups"].tolist(), eng)
    return "%2d  %s" % (i, text)


def describe(prog, upto=None):
    return "\n".join(describe_step(i, s) for i, s in enumerate(prog[:upto]))


def message(seed, i, prog, what):
    """what an assertion says: the seed, the step and the program up to it"""
    return "seed %#x, step %d: %s\n%s\n(python -m tests.index_programs %#x)" % (seed, i, what, describe(prog, i + 1), seed)


# ---- what a campaign reaches ----
def tail_figures(tail):
    """(queries of k_sw_row, chunks of k_sw_chunk) of a weighted search's plan tail"""
    m = re.search(r"k_sw_row (\d+) queries .* k_sw_chunk (\d+) chunks", tail)
    return int(m.group(1)), int(m.group(2))


def figures(programs_and_records):
    """counts over programs with their model records: what tests/test_index_programs.py holds the campaign to"""
    f = dict(steps=0, checked=0, chunk_calls=0, row_calls=0, large=0, stale_queries=0, stale_builds=0, source_gone=0, attached=0, attached_first_closed=0, window_folds=0,
             weighted_folds=0, folded_tops=0, window_algebra=0, late_formulas=0, closed_formulas=0, asked_formulas=0, covers=0, window_objects=0, most_sets=0, own_reduces=0, kinds=set(),
             transitions={(a, b): 0 for a in PAYLOADS for b in PAYLOADS if a != b}, refusals={w: 0 for w in REFUSALS}, rules=set(), windows=set())
    for prog, recs in programs_and_records:
        f["checked"] += sum(len(recs[-1][p]) for p in ("pool", "foreign", "indexes", "hits"))
        f["late_formulas"] += sum(h["weighted"] == "stale" for h in recs[-1]["hits"].values())
        f["closed_formulas"] += sum(h["weighted"] == "closed" for h in recs[-1]["hits"].values())
        f["asked_formulas"] += sum(isinstance(h["weighted"], dict) for h in recs[-1]["hits"].values())
        for s, r in zip(prog, recs):
            k = s["kind"]
            f["steps"] += k not in ("load", "sketch")
            f["checked"] += k not in ("refused", "close_sets")
            f["kinds"].add(k)
            f["window_algebra"] += bool(s.get("window_operand"))
            if k == "refused":
                f["refusals"][s["what"]] += 1
            elif k == "windows":
                f["window_objects"] += 1
                f["most_sets"] = max(f["most_sets"], r["n_sets"])
                f["windows"].add(tuple(sorted((x, s[x]) for x in ("window", "step", "count") if x in s)))
            elif k == "reduce":
                f["own_reduces"] += bool(s.get("own_groups"))
            elif k == "index":
                f["stale_builds"] += bool(s["stale"])
            elif k in ("search", "search_counted"):
                f["large"] += r["n_large_queries"] > 0
                f["source_gone"] += s["src_gone"]
                f["attached"] += s["attached"] and s["eng"] == 1
                f["attached_first_closed"] += s["attached"] and s["eng"] == 1 and s["first_closed"]
                f["covers"] += s["min_query_cov"] != 0.0 or s["min_target_cov"] != 0.0
                if k == "search_counted":
                    rows, chunks = tail_figures(r["plan_tail"])
                    f["row_calls"] += rows > 0
                    f["chunk_calls"] += chunks > 0
                    f["stale_queries"] += bool(s["stale_q"])
            elif k == "fold":
                f["window_folds"] += s["window_fold"]
                f["weighted_folds"] += r["input"]["has_weights"]
                f["rules"].add(tuple(sorted(s["rule"])))
            elif k == "top":
                f["folded_tops"] += r["input"]["has_members"]
            if k in HITS_KINDS and s["into"]:
                now = payload(r)
                if now != s["was"]:
                    f["transitions"][(s["was"], now)] += 1
    return f


if __name__ == "__main__":
    for arg in sys.argv[1:]:
        print("program %#x" % int(arg, 0))
        print(describe(program(int(arg, 0))))
