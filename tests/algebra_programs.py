"""Seeded programs over the sets-side entries (sets.hip, search.hip, setops.hip, counts.hip, compare.hip) and their NumPy interpreter.

program(seed) is a list of steps, fully determined by the seed: sources (host-loaded collections, sometimes one made from a sketch
result), then 8 to 14 calls that take their operands from the objects alive at that point and write into a new object or `into` one
that another entry made.  run_model(program) gives what every step must yield, with the references the entries' own suites use
(setops_cases.ref_op / ref_reduce, counts_cases.ref_op / ref_filter / ref_totals, compare_cases.ref_bottom / ref_compare / plan_figures,
search_cases.ref_search / ref_top); same(want, got) is the one comparison, used by tests/test_gpu_algebra_fuzz.py on the device's
records and by tests/test_algebra_programs.py on the records of the SABOTAGES -- small wrong variants of one reference each, named
after the kernel mistake they stand for.  Nothing here imports the engine.  Kernel constants are read from the sources.

    python -m tests.algebra_programs SEED      prints the program of that seed, call by call"""
import sys
import zlib

import numpy as np

from tests import compare_cases as CC
from tests import counts_cases as CN
from tests import search_cases as SR
from tests import setops_cases as SO
from tests import sets_cases as ST

U64, U32 = np.uint64, np.uint32
SAT, MAX64, MEMBERS_ALL = CN.SAT, SO.MAX64, SO.MEMBERS_ALL
CAPS, CMP, CNT_CHUNK = SO.read_caps(), CC.read_caps(), CN.read_chunk()
TILE = CAPS["SO_TILE"]

BASE, BLOCKS, PER_BLOCK = 0xA16EB000, 12, 20
NS = (1, 3, 16, 17, 33, 40)
BOTTOM_NS = (1, 5, 16, 17, 128, 129, 1 << 40)
LIMITS = (0, 1, 7, 128, 129, 1000)
SET_OPS = {SO.UNION: "union", SO.INTERSECT: "intersect", SO.DIFF: "diff", SO.SYMDIFF: "symdiff"}
COUNT_OPS = {CN.ADD: "add", CN.KEEP: "keep", CN.DROP: "drop"}
ENTRIES = ("bsk_result_sets", "bsk_result_sets_reuse", "bsk_result_sets_counted", "bsk_sets_from_host", "bsk_index_build", "bsk_index_search",
           "bsk_hits_top", "bsk_sets_op", "bsk_sets_op_counted", "bsk_sets_reduce", "bsk_sets_from_host_counted", "bsk_sets_filter_counts",
           "bsk_sets_totals", "bsk_sets_bottom", "bsk_sets_compare")
REFUSALS = ("into is an operand", "set numbers mismatched", "filter_counts of uncounted sets", "fetch_counts of uncounted sets", "bottom(0)",
            "min_count of 0", "operand of the other engine")
VALUE_BUDGET = 100_000   # values a program makes, about
COMPARE_WORK = 150_000   # values the pairs of one comparison walk together: beyond it the limit is one of the small ones


def seeds(block):
    return [BASE + PER_BLOCK * block + i for i in range(PER_BLOCK)]


def size_classes():
    """(lo, hi) of every set-size class: 0, small, and one class around each threshold of the kernels"""
    g, w, win, chunk = CAPS["SO_GROUP_CAP"], CAPS["SO_WAVE_CAP"], CMP["CMP_WINDOW"], ST.SCAN_CHUNK
    assert g == ST.SMALL_CAP and chunk == CNT_CHUNK == CAPS["RD_CHUNK"] and TILE == w
    return [(0, 0), (1, 20), (25, 40), (g - 4, g + 6), (win - 8, win + 8), (500, 530), (w - 24, w + 76), (chunk - 8, chunk + 12)]


CLASS_WEIGHTS = (0.10, 0.22, 0.13, 0.15, 0.11, 0.08, 0.11, 0.10)
ONE_SET_WEIGHTS = (0.05, 0.10, 0.10, 0.10, 0.15, 0.15, 0.20, 0.15)  # the broadcast operand is mostly a large set


def size_class(n):
    """the class a set of n values falls into (None: between two classes)"""
    for i, (lo, hi) in enumerate(size_classes()):
        if lo <= n <= hi:
            return i
    return None


# ---- objects: (offsets, values, counts or None) ----
def n_sets(t):
    return len(t[0]) - 1


def n_values(t):
    return int(t[0][-1])


def digest(*arrays):
    c = 0
    for a in arrays:
        if a is not None:
            c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return "%08x" % c


# ---- the references, one method per entry; a sabotage overrides one ----
def pairwise(a, b, fn):
    """fn(x, cx, y, cy) -> (values, counts) for every pair, a side of one set combined with every set of the other"""
    ca = CN.ones(a[0]) if a[2] is None else a[2]
    cb = CN.ones(b[0]) if b[2] is None else b[2]
    sa, sb = list(zip(SO.split(a[0], a[1]), SO.split(a[0], ca))), list(zip(SO.split(b[0], b[1]), SO.split(b[0], cb)))
    if len(sa) != len(sb):
        assert len(sa) == 1 or len(sb) == 1
        sa, sb = (sa, sb * len(sa)) if len(sb) == 1 else (sa * len(sb), sb)
    out = [fn(x, cx, y, cy) for (x, cx), (y, cy) in zip(sa, sb)]
    offs, vals = SO.collection([v for v, _ in out])
    return offs, vals, (np.concatenate([c for _, c in out]).astype(U32) if n_values((offs,)) else np.zeros(0, U32))


class Model:
    name = "the references"
    kinds = ()

    def op(self, a, b, op):
        o, v = SO.ref_op(a[:2], b[:2], op)
        return o, v, None

    def op_counted(self, a, b, op):
        return CN.ref_op(a, b, op)

    def reduce(self, a, go, m):
        o, v = SO.ref_reduce(a[:2], go, m)
        return o, v, None

    def filter(self, a, lo, hi):
        return CN.ref_filter(a, lo, hi)

    def bottom(self, a, n):
        o, v = SO.collection(CC.ref_bottom(SO.split(a[0], a[1]), n))
        c = None if a[2] is None else np.concatenate([x[:n] for x in SO.split(a[0], a[2])] + [np.zeros(0, U32)]).astype(U32)
        return o, v, c

    def compare(self, a, b, limit):
        return CC.ref_compare(SO.split(a[0], a[1]), SO.split(b[0], b[1]), limit)

    def search(self, t, q, min_shared):
        return SR.ref_search(t[0], t[1], q[0], q[1], min_shared)

    def top(self, hits, n):
        return SR.ref_top(*hits, n)

    def totals(self, t):
        return CN.ref_totals(t)

    def counts_after(self, before, new):
        """the counts of an object after an entry wrote `new` into it (before: what it held, None for a new object)"""
        return new[2]


def _tiled(x, cx, y, cy, fn):
    """fn on every tile of SO_TILE merged ranks of the pair on its own"""
    mv, from_a = SO.merged(x, y)
    ia, ib = np.cumsum(from_a) - 1, np.cumsum(~from_a) - 1
    vs, cs = [], []
    for r0 in range(0, len(mv), TILE):
        fa = from_a[r0:r0 + TILE]
        xa, xb = ia[r0:r0 + TILE][fa], ib[r0:r0 + TILE][~fa]
        v, c = fn(x[xa], cx[xa], y[xb], cy[xb])
        vs.append(v)
        cs.append(c)
    return np.concatenate(vs).astype(U64), np.concatenate(cs).astype(U32)


class TilesOnTheirOwn(Model):
    name = "1 so_rank ignores SoEdge: every tile of a tiled pair on its own"
    kinds = ("op", "op_counted")  # the steps it can change

    def _pair(self, fn):
        return lambda x, cx, y, cy: _tiled(x, cx, y, cy, fn) if len(x) + len(y) > CAPS["SO_WAVE_CAP"] else fn(x, cx, y, cy)

    def op(self, a, b, op):
        o, v, _ = pairwise(a, b, self._pair(lambda x, cx, y, cy: (SO.ref_pair(x, y, op).astype(U64), np.zeros(0, U32))))
        return o, v, None

    def op_counted(self, a, b, op):
        return pairwise(a, b, self._pair(lambda x, cx, y, cy: CN.ref_pair(x, cx, y, cy, op)))


def _add(x, cx, y, cy, finish):
    u, inv = np.unique(np.concatenate([x, y]), return_inverse=True)
    s = np.zeros(len(u), U64)
    np.add.at(s, inv, np.concatenate([cx, cy]).astype(U64))
    return u.astype(U64), finish(s).astype(U32)


class AddWraps(Model):
    name = "2 ADD without saturation"
    kinds = ("op_counted",)  # the steps it can change

    def op_counted(self, a, b, op):
        if op != CN.ADD:
            return CN.ref_op(a, b, op)
        return pairwise(a, b, lambda x, cx, y, cy: _add(x, cx, y, cy, lambda s: s & U64(SAT)))


class UncountedCountsZero(Model):
    name = "3 an uncounted operand counts 0"
    kinds = ("op_counted",)  # the steps it can change

    def op_counted(self, a, b, op):
        zero = lambda t: (t[0], t[1], np.zeros(n_values(t), U32) if t[2] is None else t[2])  # noqa: E731
        return CN.ref_op(zero(a), zero(b), op)


class PartnerAtTheSameIndex(Model):
    name = "4 ADD takes its partner's count from the same index"
    kinds = ("op_counted",)  # the steps it can change

    def op_counted(self, a, b, op):
        if op != CN.ADD:
            return CN.ref_op(a, b, op)

        def add(x, cx, y, cy):
            u = np.union1d(x, y).astype(U64)
            ix, iy = np.searchsorted(x, u), np.searchsorted(y, u)
            in_x = (ix < len(x)) & (x[np.minimum(ix, len(x) - 1)] == u) if len(x) else np.zeros(len(u), bool)
            in_y = (iy < len(y)) & (y[np.minimum(iy, len(y) - 1)] == u) if len(y) else np.zeros(len(u), bool)
            s = np.zeros(len(u), U64)
            s[in_x] += cx[ix[in_x]].astype(U64)
            s[in_y & ~in_x] += cy[iy[in_y & ~in_x]].astype(U64)
            both = in_x & in_y
            s[both] += cy[np.minimum(ix[both], len(y) - 1)].astype(U64)  # (the index of a's copy, not of b's)
            return u, np.minimum(s, U64(SAT)).astype(U32)

        return pairwise(a, b, add)


class _ComparePairs(Model):
    def compare(self, a, b, limit):
        A, B = SO.split(a[0], a[1]), SO.split(b[0], b[1])
        sh, tt = np.zeros((len(A), len(B)), U32), np.zeros((len(A), len(B)), U32)
        for i, x in enumerate(A):
            for j, y in enumerate(B):
                sh[i, j], tt[i, j] = self.pair(x, y, limit)
        return sh, tt


class SharedOverThePrefixes(_ComparePairs):
    name = "5 compare counts shared over both prefixes, not up to the union's limit-th value"
    kinds = ("compare",)  # the steps it can change

    def pair(self, x, y, limit):
        if limit:
            x, y = x[:limit], y[:limit]
        total = len(np.union1d(x, y))
        return len(np.intersect1d(x, y)), min(total, limit) if limit else total


class OneWindowOnly(_ComparePairs):
    name = "6 compare stops a set at its first CMP_WINDOW values"
    kinds = ("compare",)  # the steps it can change

    def pair(self, x, y, limit):
        return CC.ref_pair(x[:CMP["CMP_WINDOW"]], y[:CMP["CMP_WINDOW"]], limit)


class BottomCountsByOutputIndex(Model):
    name = "7 bottom takes the counts from the output index"
    kinds = ("bottom",)  # the steps it can change

    def bottom(self, a, n):
        o, v, c = Model.bottom(self, a, n)
        return o, v, None if c is None else a[2][:len(v)].copy()


class TrailingEmptySetAtZero(Model):
    name = "8 filter_counts gives a trailing empty set the offset 0"
    kinds = ("filter",)  # the steps it can change

    def filter(self, a, lo, hi):
        o, v, c = CN.ref_filter(a, lo, hi)
        o = o.copy()
        o[:-1][a[0][:-1] >= a[0][-1]] = 0
        return o, v, c

    def totals(self, t):
        cs = np.concatenate([np.zeros(1, U64), np.cumsum(t[2].astype(U64))]) if t[2] is not None else np.arange(len(t[1]) + 1, dtype=U64)
        return cs[t[0][1:].astype(np.int64)] - cs[t[0][:-1].astype(np.int64)]  # (offsets that decrease: the difference wraps)


class RunsAcrossGroups(Model):
    name = "9 reduce lets a run continue across a group border"
    kinds = ("reduce",)  # the steps it can change

    def reduce(self, a, go, m):
        sets, G = SO.split(a[0], a[1]), len(go) - 1
        members = [sets[int(go[g]):int(go[g + 1])] for g in range(G)]
        per = [np.sort(np.concatenate(ms + [np.zeros(0, U64)])) for ms in members]
        allv = np.concatenate(per + [np.zeros(0, U64)])
        gid = np.repeat(np.arange(G), [len(p) for p in per])
        need = np.array([len(ms) if m == MEMBERS_ALL else m for ms in members] + [0], np.int64)
        out = [[] for _ in range(G)]
        if len(allv):
            head = np.flatnonzero(np.concatenate([[True], allv[1:] != allv[:-1]]))
            length = np.diff(np.concatenate([head, [len(allv)]]))
            for h, n in zip(head[length >= need[gid[head]]], length[length >= need[gid[head]]]):
                out[gid[h]].append(allv[h])
        o, v = SO.collection([np.array(x, U64) for x in out])
        return o, v, None


class CountedStaysSet(Model):
    name = "10 `into` leaves counted set after an uncounted entry wrote the object"
    kinds = ("op", "reduce", "bottom", "result_sets")

    def counts_after(self, before, new):
        if new[2] is None and before is not None and before[2] is not None:
            return np.resize(np.concatenate([before[2], np.ones(1, U32)]), n_values(new)).astype(U32)
        return new[2]


class TopTiesByShared(Model):
    name = "11 top(n) breaks ties between hits by shared alone"
    kinds = ("search",)  # the steps it can change

    def top(self, hits, n):
        o, t, s = hits
        no, _, _ = SR.ref_top(o, t, s, n)
        cnt = np.diff(o).astype(np.int64)
        q = np.repeat(np.arange(len(o) - 1, dtype=np.int64), cnt)
        order = np.lexsort((-t.astype(np.int64), -s.astype(np.int64), q))  # (equal shared counts: the larger target first)
        rank = np.arange(len(t), dtype=np.int64) - np.repeat(o[:-1].astype(np.int64), cnt)
        idx = order[rank < n]
        return no, t[idx], s[idx]


SABOTAGES = (TilesOnTheirOwn, AddWraps, UncountedCountsZero, PartnerAtTheSameIndex, SharedOverThePrefixes, OneWindowOnly, BottomCountsByOutputIndex,
             TrailingEmptySetAtZero, RunsAcrossGroups, CountedStaysSet, TopTiesByShared)


# ---- the interpreter ----
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def standin_values(step):
    """Per read the hash values a sketch of it might give, without an engine: every k-mer's 2-bit code through search_cases.mix64
    (ntHash's place), or the minimum of every window of w of them (the minimizers' place).  Only the generator and the CPU test use
    it; on the device the values are the result's own (BatchResult.read)."""
    k, w, out = step["k"], step["w"], []
    for r in step["reads"]:
        code = (np.frombuffer(r.encode(), np.uint8) >> 1) & 3
        if len(code) < k + (w - 1 if step["sketch"] == "minimizer" else 0):
            out.append(np.zeros(0, U64))
            continue
        win = np.lib.stride_tricks.sliding_window_view(code.astype(U64), k)
        h = SR.mix64((win << (U64(2) * np.arange(k, dtype=U64))[None, :]).sum(1).astype(U64))
        if step["sketch"] == "minimizer":
            h = np.lib.stride_tricks.sliding_window_view(h, w).min(1)
            h = h[np.concatenate([[True], h[1:] != h[:-1]])]
        out.append(h.astype(U64))
    return out


def sets_of_values(values, whole, scale, counted):
    """np.unique(values, return_counts=True) with the maxhash cut, per read or for all reads together"""
    o, v, c = CN.ref_counted(values, scale, whole)
    return o, v, c if counted else None


class State:
    def __init__(self, model, read_values=None):
        self.model, self.read_values = model, read_values
        self.objs, self.maker, self.cmps, self.hits = {}, {}, {}, {}
        self.sketch = None

    def snap(self, ids):
        return {i: self.objs[i] for i in ids}


def _sets_record(st, step, new, entry, operands, paths=None):
    """an entry wrote `new` into step["out"]: the record to compare, and the object's new state"""
    out = step["out"]
    before = st.objs.get(out)
    new = (new[0], new[1], st.model.counts_after(before, new))
    rec = dict(n_sets=n_sets(new), n_values=n_values(new), offsets=new[0], values=new[1], counted=new[2] is not None,
               counts=new[2], totals=st.model.totals(new), operands=st.snap(operands))
    if paths is not None:
        rec["paths"] = paths
    st.objs[out], st.maker[out] = new, entry
    if not step.get("keep", True):
        del st.objs[out], st.maker[out]
    return rec


_figures = {}


def plan_figures(a, b, limit):
    key = (digest(a[0], a[1]), digest(b[0], b[1]), len(a[1]), len(b[1]), limit)
    if key not in _figures:
        _figures[key] = tuple(int(x) for x in CC.plan_figures(SO.split(a[0], a[1]), SO.split(b[0], b[1]), limit, CMP))
    return _figures[key]


def apply(st, step):
    """one step on the model's state -> what the step must yield"""
    M, k = st.model, step["kind"]
    if k == "load":
        entry = "bsk_sets_from_host" if step["counts"] is None else "bsk_sets_from_host_counted"
        return _sets_record(st, step, (step["offsets"], step["values"], step["counts"]), entry, [])
    if k == "sketch":
        st.sketch = step
        if st.read_values is None:
            st.read_values = standin_values(step)
        entry = "bsk_result_sets_counted" if step["counted"] else "bsk_result_sets"
        return _sets_record(st, step, sets_of_values(st.read_values, step["whole"], step["scale"], step["counted"]), entry, [])
    if k == "result_sets":
        entry = "bsk_result_sets_counted" if step["counted"] else "bsk_result_sets_reuse"
        return _sets_record(st, step, sets_of_values(st.read_values, step["whole"], step["scale"], step["counted"]), entry, [])
    if k == "refused":
        ids = [step[x] for x in ("a", "b", "into") if step.get(x) is not None]
        return dict(rc="ERR_ARG", operands=st.snap(dict.fromkeys(ids)))
    a = st.objs[step["a"]]
    if k == "op":
        b = st.objs[step["b"]]
        return _sets_record(st, step, M.op(a, b, step["op"]), "bsk_sets_op", [step["a"], step["b"]], SO.path_counts(a[0], b[0], CAPS))
    if k == "op_counted":
        b = st.objs[step["b"]]
        return _sets_record(st, step, M.op_counted(a, b, step["op"]), "bsk_sets_op_counted", [step["a"], step["b"]], CN.path_counts(a[0], b[0], CAPS))
    if k == "reduce":
        return _sets_record(st, step, M.reduce(a, step["groups"], step["m"]), "bsk_sets_reduce", [step["a"]])
    if k == "filter":
        return _sets_record(st, step, M.filter(a, step["lo"], SAT if step["hi"] is None else step["hi"]), "bsk_sets_filter_counts", [step["a"]])
    if k == "bottom":
        return _sets_record(st, step, M.bottom(a, step["n"]), "bsk_sets_bottom", [step["a"]])
    if k == "compare":
        b = st.objs[step["b"]]
        sh, tt = M.compare(a, b, step["limit"])
        st.cmps[step["cmp"]] = (sh, tt)
        return dict(n_a=n_sets(a), n_b=n_sets(b), limit=step["limit"], shared=sh, total=tt, figures=plan_figures(a, b, step["limit"]),
                    operands=st.snap([step["a"], step["b"]]))
    assert k == "search", k
    q = st.objs[step["q"]]
    hits = M.search(a, q, step["min_shared"])
    rec = dict(n_queries=n_sets(q), n_hits=int(hits[0][-1]), offsets=hits[0], targets=hits[1], shared=hits[2], operands=st.snap([step["a"], step["q"]]))
    if step["top"]:
        top = M.top(hits, step["top"])
        st.hits[step["hits"]] = top
        rec.update(top_offsets=top[0], top_targets=top[1], top_shared=top[2])
    return rec


def run_model(program, model=None, read_values=None):
    """-> one record per step and a last one, {"pool": every object alive at the end, "compares", "tops"}.  read_values: the values of
    the sketch step's reads (from the device; None: standin_values)"""
    st = State(model or Model(), read_values)
    records = [apply(st, step) for step in program]
    records.append(dict(pool=dict(st.objs), compares=dict(st.cmps), tops=dict(st.hits)))
    return records


def _replay(st, step, rec):
    """the state after a step whose record is known"""
    k = step["kind"]
    if k == "sketch":
        st.sketch, st.read_values = step, standin_values(step)
    if "out" in step and step.get("keep", True):
        st.objs[step["out"]] = (rec["offsets"], rec["values"], rec["counts"])
    elif "out" in step:
        st.objs.pop(step["out"], None)
    if k == "compare":
        st.cmps[step["cmp"]] = (rec["shared"], rec["total"])
    if k == "search" and step["top"]:
        st.hits[step["hits"]] = (rec["top_offsets"], rec["top_targets"], rec["top_shared"])


def first_difference(program, want, model):
    """the first step at which `model` yields something else than the records `want` -> (step, differences), or None"""
    st = State(model)
    for i, step in enumerate(program):
        if step["kind"] not in model.kinds:  # nothing differed so far and this step cannot: its record is the wanted one
            _replay(st, step, want[i])
            continue
        diff = same(want[i], apply(st, step))
        if diff:
            return i, diff
    diff = same(want[-1], dict(pool=dict(st.objs), compares=dict(st.cmps), tops=dict(st.hits)))
    return (len(program), diff) if diff else None


def same(want, got, path=""):
    """every difference between two records, as text; [] when they agree.  Arrays must agree in type, length and every element."""
    if isinstance(want, dict):
        if not isinstance(got, dict) or set(want) != set(got):
            return ["%s: keys %s != %s" % (path, sorted(map(str, want)), sorted(map(str, got)) if isinstance(got, dict) else got)]
        return [d for key in want for d in same(want[key], got[key], "%s.%s" % (path, key) if path else str(key))]
    if isinstance(want, (tuple, list)):
        if not isinstance(got, (tuple, list)) or len(want) != len(got):
            return ["%s: %r != %r" % (path, type(want), type(got))]
        return [d for i, (w, g) in enumerate(zip(want, got)) for d in same(w, g, "%s[%d]" % (path, i))]
    if isinstance(want, np.ndarray):
        if not isinstance(got, np.ndarray) or want.dtype != got.dtype or want.shape != got.shape:
            return ["%s: %s%s != %s" % (path, want.dtype, want.shape, "%s%s" % (got.dtype, got.shape) if isinstance(got, np.ndarray) else type(got))]
        if not np.array_equal(want, got):
            at = np.argwhere(want != got)[0]
            return ["%s: first difference at %s of %d: want %s, got %s" % (path, at.tolist(), len(np.argwhere(want != got)), want[tuple(at)], got[tuple(at)])]
        return []
    return [] if (want is None) == (got is None) and want == got else ["%s: want %r, got %r" % (path, want, got)]


# ---- the generator ----
def _universe(rng):
    kind = ("dense", "wide", "extremes")[int(rng.integers(0, 3))]
    if kind == "dense":
        u = int(rng.choice([64, 700, 5000]))
        return "dense U=%d" % u, np.arange(u, dtype=U64)
    pool = np.unique(rng.integers(0, MAX64, size=6000, dtype=U64, endpoint=True))
    if kind == "extremes":
        pool = np.unique(np.concatenate([pool, np.array([0, 1, MAX64 - 1, MAX64], U64)]))
    return "%s, %d values" % (kind, len(pool)), rng.permutation(pool)


def _sizes(rng, n, one_set=False):
    classes = size_classes()
    w = np.array(ONE_SET_WEIGHTS if one_set else CLASS_WEIGHTS if n <= 17 else CLASS_WEIGHTS[:4])
    pick = rng.choice(len(w), size=n, p=w / w.sum())
    return [int(rng.integers(classes[c][0], classes[c][1] + 1)) for c in pick]


def _collection(rng, pool, dense, sizes):
    """sets of the given sizes: each drawn from the first values of the pool's order -- four times its size of them, so two sets of
    a kind share a quarter; a dense universe sometimes gives `stairs`, ascending windows that meet in one value (the largest value
    of a set is the smallest of the next)"""
    sizes = [min(s, len(pool)) for s in sizes]
    if dense and rng.random() < 0.4:
        sets, lo = [], 0
        for s in sizes:
            if s == 0:
                sets.append(np.zeros(0, U64))
                continue
            width = s + int(rng.integers(0, s + 1))
            inner = rng.choice(np.arange(lo + 1, lo + width - 1), size=s - 2, replace=False) if s > 2 else np.zeros(0, np.int64)
            sets.append(np.unique(np.concatenate([np.array([lo, lo + width - 1][:min(s, 2)], np.int64), inner]).astype(U64)))
            lo += width - 1
        return sets, "stairs"
    return [np.sort(rng.choice(pool[:max(4 * s, 48)], size=s, replace=False)).astype(U64) for s in sizes], "drawn"


def _counts(rng, n):
    c = rng.integers(1, 6, size=n).astype(U32)
    if n and rng.random() < 0.5:
        at = rng.choice(n, size=max(1, n // 100), replace=False)
        c[at] = (SAT - rng.integers(0, 4, size=len(at))).astype(U32)
    return c


def _reads(rng, n):
    """n short reads: pieces of one 300-base sequence (whole-batch counts above 1) and a few tandem repeats (per-read counts above 1)"""
    genome = _ACGT[rng.integers(0, 4, 300)].tobytes().decode()
    reads = []
    for _ in range(n):
        r = rng.random()
        if r < 0.15:
            unit = _ACGT[rng.integers(0, 4, int(rng.integers(2, 8)))].tobytes().decode()
            reads.append((unit * 60)[:int(rng.integers(30, 100))])
        elif r < 0.25:
            reads.append(genome[:int(rng.integers(0, 21))])  # too short for any k here
        else:
            at = int(rng.integers(0, 240))
            reads.append(genome[at:at + int(rng.integers(25, 121))])
    return reads


class _Gen:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.st = State(Model())
        self.steps, self.records, self.next_id, self.made = [], [], 0, 0

    def new_id(self, prefix="s"):
        self.next_id += 1
        return "%s%d" % (prefix, self.next_id - 1)

    def emit(self, step):
        rec = apply(self.st, step)
        self.steps.append(step)
        self.records.append(rec)
        self.made += rec.get("n_values", 0)
        return rec

    def pick(self, ok=lambda i, t: True, exclude=()):
        """a live object: one that holds values if three more draws find one, and one that fits what is left of the program's share of values"""
        ids = [i for i, t in self.st.objs.items() if i not in exclude and ok(i, t)]
        room = max(2500, (VALUE_BUDGET - self.made) // 2)  # (a result holds at most its two operands' values)
        if any(n_values(self.st.objs[i]) <= room for i in ids):
            ids = [i for i in ids if n_values(self.st.objs[i]) <= room]
        if not ids:
            return None
        for _ in range(4):
            i = ids[int(self.rng.integers(0, len(ids)))]
            if n_values(self.st.objs[i]):
                break
        return i

    def out(self, step, operands):
        """where the result goes: half the time into a live object that is no operand"""
        others = [i for i in self.st.objs if i not in operands]
        if others and self.rng.random() < 0.5:
            step["out"], step["into"] = others[int(self.rng.integers(0, len(others)))], True
        else:
            step["out"], step["into"] = self.new_id(), False
        step["made_by"] = self.st.maker.get(step["out"])
        return step

    def finish(self, step):
        """a result without values is checked, and stays in the pool one time in four"""
        rec = self.emit(step)
        if rec["n_values"] == 0 and self.rng.random() < 0.75:
            step["keep"] = False
            del self.st.objs[step["out"]], self.st.maker[step["out"]]
        return rec


def _step(g, kind):
    rng, objs = g.rng, g.st.objs
    if kind in ("op", "op_counted"):
        a = g.pick()
        if kind == "op":
            partner = lambda i, t: n_sets(t) in (n_sets(objs[a]), 1)  # noqa: E731
            op = int(rng.choice(list(SET_OPS), p=[0.3, 0.2, 0.25, 0.25]))
        else:
            partner = lambda i, t: n_sets(objs[a]) == 1 or n_sets(t) in (n_sets(objs[a]), 1)  # noqa: E731
            op = int(rng.choice(list(COUNT_OPS), p=[0.5, 0.25, 0.25]))
        b = a if rng.random() < 0.08 else g.pick(partner, exclude=(a,)) or a
        if kind == "op_counted" and rng.random() < 0.3 and n_sets(objs[b]) == 1 and n_sets(objs[a]) != 1:
            a, b = b, a  # (the one-set operand as a)
        na, nb = n_sets(objs[a]), n_sets(objs[b])
        most = n_values(objs[a]) * (nb if na == 1 else 1) + n_values(objs[b]) * (na if nb == 1 else 1)
        if g.made + most > 3 * VALUE_BUDGET // 2:  # a large set against every set of many: only what stays within the many sets' own values
            a, b = (b, a) if na == 1 and nb != 1 else (a, b)
            op = int(rng.choice([SO.INTERSECT, SO.DIFF]))  # (= KEEP, DROP)
        return g.finish(g.out(dict(kind=kind, a=a, b=b, op=op), (a, b)))
    if kind == "reduce":
        a = g.pick()
        ns = n_sets(objs[a])
        cuts = np.sort(rng.integers(0, ns + 1, size=int(rng.integers(0, min(ns, 34) + 2))))
        lead, trail = int(rng.integers(0, 3)) // 2, int(rng.integers(0, 3)) // 2
        groups = np.concatenate([[0] * (1 + lead), cuts, [ns] * (1 + trail)]).astype(U64)
        m = int(rng.choice([1, 2, MEMBERS_ALL], p=[0.35, 0.35, 0.3]))
        return g.finish(g.out(dict(kind="reduce", a=a, groups=groups, m=m), (a,)))
    if kind == "filter":
        a = g.pick(lambda i, t: t[2] is not None)
        if a is None:
            return None
        lo = int(rng.integers(1, 4))
        hi = [lo, 5, None][int(rng.integers(0, 3))]
        return g.finish(g.out(dict(kind="filter", a=a, lo=lo, hi=hi), (a,)))
    if kind == "bottom":
        a = g.pick()
        return g.finish(g.out(dict(kind="bottom", a=a, n=int(BOTTOM_NS[int(rng.integers(0, len(BOTTOM_NS)))])), (a,)))
    if kind == "compare":
        a = g.pick()
        b = a if rng.random() < 0.25 else g.pick()
        limit = int(LIMITS[int(rng.integers(0, len(LIMITS)))])
        cut = lambda t: np.minimum(np.diff(t[0]).astype(np.int64), limit or (1 << 62))  # noqa: E731
        work = lambda: int(cut(objs[a]).sum()) * n_sets(objs[b]) + int(cut(objs[b]).sum()) * n_sets(objs[a])  # noqa: E731
        if work() > COMPARE_WORK:
            limit = int((1, 7, 128, 129)[int(rng.integers(0, 4))])
        if work() > COMPARE_WORK:
            limit = 7
        cmp = list(g.st.cmps)[int(rng.integers(0, len(g.st.cmps)))] if g.st.cmps and rng.random() < 0.4 else g.new_id("c")
        return g.emit(dict(kind="compare", a=a, b=b, limit=limit, cmp=cmp))
    if kind == "search":
        a, q = g.pick(), g.pick()
        step = dict(kind="search", a=a, q=q, min_shared=int(rng.choice([1, 2, 5])), top=0, hits=None)
        if rng.random() < 0.5:
            step["top"] = int(rng.choice([1, 3]))
            step["hits"] = list(g.st.hits)[int(rng.integers(0, len(g.st.hits)))] if g.st.hits and rng.random() < 0.5 else g.new_id("h")
        return g.emit(step)
    assert kind == "result_sets"
    if g.st.sketch is None:
        return None
    step = dict(kind="result_sets", whole=bool(rng.random() < 0.4), scale=int(rng.choice([1, 3])), counted=bool(rng.random() < 0.5),
                no_small=bool(rng.random() < 0.3))
    ids = list(objs)
    step["out"], step["into"] = ids[int(rng.integers(0, len(ids)))], True
    step["made_by"] = g.st.maker[step["out"]]
    return g.finish(step)


def _refused(g):
    """a call the library refuses on the host, before any launch; `into` (if any) and every operand must stay what they were"""
    rng, objs = g.rng, g.st.objs
    what = REFUSALS[int(rng.integers(0, len(REFUSALS)))]
    counted = lambda i, t: t[2] is not None  # noqa: E731
    plain = lambda i, t: t[2] is None  # noqa: E731
    a = g.pick(counted if what == "min_count of 0" else plain if "uncounted" in what else (lambda i, t: True))
    if a is None:
        what, a = "bottom(0)", g.pick()
    step = dict(kind="refused", what=what, a=a, b=None, into=None)
    if what in ("into is an operand", "set numbers mismatched", "operand of the other engine"):
        step["b"] = g.pick(lambda i, t: n_sets(t) in (n_sets(objs[a]), 1)) if what == "into is an operand" else None
    if what == "into is an operand":
        step["into"] = a if rng.random() < 0.5 else step["b"]
    elif what != "fetch_counts of uncounted sets":
        others = [i for i in objs if i not in (a, step["b"])]
        if others and rng.random() < 0.7:
            step["into"] = others[int(rng.integers(0, len(others)))]
    return g.emit(step)


KINDS = ("op", "op_counted", "reduce", "filter", "bottom", "compare", "search", "result_sets")
KIND_WEIGHTS = (0.18, 0.22, 0.13, 0.11, 0.08, 0.12, 0.08, 0.08)


def program(seed):
    return program_and_records(seed)[0]


def program_and_records(seed):
    """the program of a seed and run_model's records of it (the generator runs the model as it goes: an operand without values is
    drawn again, a result without values mostly leaves the pool)"""
    g = _Gen(seed)
    rng = g.rng
    name, pool = _universe(rng)
    n = int(NS[int(rng.integers(0, len(NS)))])
    sketched = int(rng.integers(0, 4)) if rng.random() < 1 / 3 else None  # which source comes from a sketch result (3: the one-set one)
    for which in range(4):
        ns = n if which < 3 else 1
        if which == sketched:
            whole = which == 3
            mini = bool(rng.random() < 0.5)
            g.emit(dict(kind="sketch", out=g.new_id(), sketch="minimizer" if mini else "nthash", k=15 if mini else 21, w=5 if mini else 0,
                        reads=_reads(rng, int(rng.integers(24, 49)) if whole else ns), whole=whole, scale=int(rng.choice([1, 3])),
                        counted=bool(rng.random() < 0.5), no_small=bool(rng.random() < 0.4), universe=name))
            continue
        sets, layout = _collection(rng, pool, name.startswith("dense"), _sizes(rng, ns, which == 3))
        offs, vals = SO.collection(sets)
        g.emit(dict(kind="load", out=g.new_id(), offsets=offs, values=vals, counts=_counts(rng, len(vals)) if rng.random() < 0.5 else None,
                    layout=layout, universe=name))
    todo = int(rng.integers(8, 15))
    while todo:
        if rng.random() < 1 / 15:
            _refused(g)
            todo -= 1
        elif _step(g, KINDS[int(rng.choice(len(KINDS), p=KIND_WEIGHTS))]) is not None:
            todo -= 1
    g.records.append(dict(pool=dict(g.st.objs), compares=dict(g.st.cmps), tops=dict(g.st.hits)))
    return g.steps, g.records


# ---- the text of a program ----
def _sizes_text(offs):
    s = np.diff(offs).astype(np.int64).tolist()
    return "%d sets of %s values" % (len(s), s if len(s) <= 8 else "%s ... %s" % (str(s[:5])[:-1], str(s[-2:])[1:]))


def describe_step(i, s):
    k = s["kind"]
    into = " into %s (made by %s)" % (s["out"], s["made_by"]) if s.get("into") is True else ""
    drop = "; closed after the check" if not s.get("keep", True) else ""
    if k == "load":
        c = s["counts"]
        text = "%s = sets_from_arrays%s(%s; %s of %s; crc %s%s)" % (s["out"], "" if c is None else "_counted", _sizes_text(s["offsets"]), s["layout"], s["universe"],
                                                                  digest(s["offsets"], s["values"], c), "" if c is None else ", counts up to %d" % c.max(initial=0))
    elif k == "sketch":
        text = "%s = run(%d reads, crc %s; %s k=%d w=%d).%s(whole_batch=%s, scale=%d)%s" % (
            s["out"], len(s["reads"]), digest(np.frombuffer("/".join(s["reads"]).encode(), np.uint8)), s["sketch"], s["k"], s["w"],
            "counted_sets" if s["counted"] else "device_sets", s["whole"], s["scale"], " under BSK_SETS_NO_SMALL" if s["no_small"] and not s["counted"] else "")
    elif k == "result_sets":
        text = "the sketch result's %s(whole_batch=%s, scale=%d)%s%s" % ("counted_sets" if s["counted"] else "bsk_result_sets_reuse", s["whole"], s["scale"],
                                                                        " under BSK_SETS_NO_SMALL" if s["no_small"] and not s["counted"] else "", into)
    elif k == "op":
        text = "%s = %s.op(%s, %s)%s" % (s["out"], s["a"], s["b"], SET_OPS[s["op"]], into)
    elif k == "op_counted":
        text = "%s = %s.op_counted(%s, %s)%s" % (s["out"], s["a"], s["b"], COUNT_OPS[s["op"]], into)
    elif k == "reduce":
        text = "%s = %s.reduce(%s, min_members=%s)%s" % (s["out"], s["a"], s["groups"].tolist(), "MEMBERS_ALL" if s["m"] == MEMBERS_ALL else s["m"], into)
    elif k == "filter":
        text = "%s = %s.filter_counts(%d, %s)%s" % (s["out"], s["a"], s["lo"], s["hi"], into)
    elif k == "bottom":
        text = "%s = %s.bottom(%d)%s" % (s["out"], s["a"], s["n"], into)
    elif k == "compare":
        text = "%s = %s.compare(%s, limit=%d)" % (s["cmp"], s["a"], s["b"], s["limit"])
    elif k == "search":
        text = "%s.index().search(%s, min_shared=%d)" % (s["a"], s["q"], s["min_shared"]) + (".top(%d) as %s" % (s["top"], s["hits"]) if s["top"] else "")
    else:
        text = "REFUSED (%s): a=%s b=%s into=%s" % (s["what"], s["a"], s["b"], s["into"])
    return "%2d  %s%s" % (i, text, drop)


def describe(prog, upto=None):
    return "\n".join(describe_step(i, s) for i, s in enumerate(prog[:upto]))


def message(seed, i, prog, what):
    """what an assertion says: the seed, the step and the program up to it"""
    return "seed %#x, step %d: %s\n%s\n(python -m tests.algebra_programs %#x)" % (seed, i, what, describe(prog, i + 1), seed)


# ---- what a campaign reaches ----
def figures(programs_and_records):
    """counts over programs with their model records: what tests/test_algebra_programs.py holds the campaign to"""
    f = dict(checked=0, empty=0, paths=[0, 0, 0], multi_round=0, filters=0, strict_reduces=0, into_other=0, refused=0, entries=set(), bottoms=set(),
             limits=set(), classes=set(), saturated=0, big_totals=0, a_broadcast=0, refusals=set(), steps=0)
    for prog, recs in programs_and_records:
        objs = {}
        for s, r in zip(prog, recs):
            k = s["kind"]
            f["steps"] += k not in ("load", "sketch")
            if k == "refused":
                f["refused"] += 1
                f["refusals"].add(s["what"])
                continue
            if "offsets" in r and "targets" not in r:
                f["entries"].add("bsk_sets_totals")
                f["big_totals"] += int((r["totals"] > U64(1 << 32)).any())
                if k in ("load", "sketch"):
                    f["classes"] |= {size_class(int(x)) for x in np.diff(r["offsets"]).astype(np.int64)}
                    f["entries"].add("bsk_sets_from_host" + ("_counted" if r["counted"] else "") if k == "load" else
                                     "bsk_result_sets" + ("_counted" if r["counted"] else ""))
                else:
                    f["checked"] += 1
                    f["empty"] += r["n_values"] == 0
                    f["into_other"] += bool(s.get("into")) and s["made_by"] != _entry(s)
                    f["entries"].add(_entry(s))
            if k in ("op", "op_counted"):
                f["paths"] = [x + y for x, y in zip(f["paths"], r["paths"])]
                a, b = objs[s["a"]], objs[s["b"]]
                f["a_broadcast"] += k == "op_counted" and n_sets(a) == 1 and n_sets(b) > 1
                if k == "op_counted" and s["op"] == CN.ADD and r["n_values"]:
                    f["saturated"] += bool(pairwise(a, b, lambda x, cx, y, cy: _add(x, cx, y, cy, lambda t: t > U64(SAT)))[2].any())
            elif k == "reduce":
                f["strict_reduces"] += s["m"] != 1
            elif k == "filter":
                f["filters"] += 1
            elif k == "bottom":
                f["bottoms"].add(s["n"])
            elif k == "compare":
                f["entries"].add("bsk_sets_compare")
                f["limits"].add(s["limit"])
                f["multi_round"] += r["figures"][2] > 1
            elif k == "search":
                f["entries"] |= {"bsk_index_build", "bsk_index_search"} | ({"bsk_hits_top"} if s["top"] else set())
            if "out" in s:
                objs[s["out"]] = (r["offsets"], r["values"], r["counts"])
    return f


def _entry(s):
    return {"op": "bsk_sets_op", "op_counted": "bsk_sets_op_counted", "reduce": "bsk_sets_reduce", "filter": "bsk_sets_filter_counts", "bottom": "bsk_sets_bottom",
            "result_sets": "bsk_result_sets_counted" if s.get("counted") else "bsk_result_sets_reuse"}[s["kind"]]


if __name__ == "__main__":
    for arg in sys.argv[1:]:
        print("program %#x" % int(arg, 0))
        print(describe(program(int(arg, 0))))
