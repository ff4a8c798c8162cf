"""NumPy model of the merged hits (include/biosketch.h "merged hits") and the cases its tests run.

merge_model: the parts' hits concatenated with their rows, lexsort by (row, target'), runs of one (row, target') combined in Python
integers and saturated at the end.  path_of: the path predicate of the header.  Records are those of tests/select_cases.py."""
import numpy as np

from tests import select_cases as SC
from tests import transpose_cases as TC

U64, U32 = np.uint64, np.uint32
PAYLOADS = SC.PAYLOADS
MAX32, MAX64 = (1 << 32) - 1, (1 << 64) - 1
MAX_PARTS = 64
MERGED_ROW_LENGTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000)
PAYLOAD_SETS = ((), ("total",), ("total", "dot"), ("dot",), ("members",))  # as random_record names them: "dot" brings msum
LIMITS = dict(s=MAX32, total=MAX32, members=MAX32, dot=MAX64, msum=MAX64)


class Duplicate(SC.BadHits):
    """BSK_ERR_ARG: a row names a target' twice and BSK_MERGE_ADD is not set"""


class Unsupported(ValueError):
    """BSK_ERR_UNSUPPORTED: a target_base + target of 2^32 or more"""


def carried(recs):
    """the payloads every part carries"""
    return tuple(p for p in PAYLOADS if all(r[p] is not None for r in recs))


def ascending(rec):
    """every row strictly ascending by target"""
    t, o = rec["t"].astype(np.int64), rec["o"].astype(np.int64)
    if len(t) < 2:
        return True
    inner = np.ones(len(t), bool)
    inner[o[:-1][o[:-1] < len(t)]] = False  # a row's first hit has no predecessor in its row
    return bool(np.all((np.diff(t) > 0) | ~inner[1:]))


def path_of(recs, bases):
    """'concat' when every part has ascending rows and the shifted target ranges of the non-empty parts are disjoint and increase with
    p, else 'sort'"""
    top = -1
    for r, b in zip(recs, bases):
        if not len(r["t"]):
            continue
        if not ascending(r) or int(r["t"].min()) + int(b) <= top:
            return "sort"
        top = int(r["t"].max()) + int(b)
    return "concat"


def merge_model(recs, bases=None, add=False):
    """-> (record, figures): figures = dict(path, parts, hits, combined) as bsk_hits_plan reports them"""
    bases = [0] * len(recs) if bases is None else [int(b) for b in bases]
    nq = len(recs[0]["o"]) - 1
    assert all(len(r["o"]) - 1 == nq for r in recs)
    keep = carried(recs)
    rows = np.concatenate([TC.rows_of(r["o"]) for r in recs])
    tgt = np.concatenate([r["t"].astype(np.int64) + b for r, b in zip(recs, bases)])
    if len(tgt) and int(tgt.max()) > MAX32:
        raise Unsupported("target_base + target >= 2^32")
    cols = {k: np.concatenate([r[k] for r in recs]) for k in ("s",) + keep}
    order = np.lexsort((tgt, rows))
    rows, tgt = rows[order], tgt[order]
    head = np.ones(len(tgt), bool)
    head[1:] = (rows[1:] != rows[:-1]) | (tgt[1:] != tgt[:-1])
    combined = int(len(tgt) - head.sum())
    if combined and not add:
        raise Duplicate("a row names a target twice")
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], len(tgt))
    out = dict(o=np.concatenate([[0], np.cumsum(np.bincount(rows[head], minlength=nq))]).astype(U64), t=tgt[head].astype(U32))
    for k in ("s",) + PAYLOADS:
        if k != "s" and k not in keep:
            out[k] = None
            continue
        col = [int(x) for x in cols[k][order]]
        sums = [min(sum(col[a:b]), LIMITS[k]) for a, b in zip(starts, ends)]  # Python integers, saturated at the end
        out[k] = np.asarray(sums, U32 if LIMITS[k] == MAX32 else U64)
    return out, dict(path=path_of(recs, bases), parts=len(recs), hits=int(len(tgt)), combined=combined)


def merge_brute(recs, bases=None, add=False):
    """the same through a dict of dicts: row -> target' -> the fields' sums"""
    bases = [0] * len(recs) if bases is None else [int(b) for b in bases]
    nq, keep = len(recs[0]["o"]) - 1, carried(recs)
    table = [dict() for _ in range(nq)]
    for r, b in zip(recs, bases):
        for q in range(nq):
            for i in range(int(r["o"][q]), int(r["o"][q + 1])):
                t = int(r["t"][i]) + b
                if t > MAX32:
                    raise Unsupported("target_base + target >= 2^32")
                if t in table[q] and not add:
                    raise Duplicate("a row names a target twice")
                cell = table[q].setdefault(t, {k: 0 for k in ("s",) + keep})
                for k in cell:
                    cell[k] = min(cell[k] + int(r[k][i]), LIMITS[k])  # (a saturating sum does not depend on where it is clipped)
    o, cols = [0], {k: [] for k in ("t", "s") + keep}
    for q in range(nq):
        for t in sorted(table[q]):
            cols["t"].append(t)
            for k, v in table[q][t].items():
                cols[k].append(v)
        o.append(len(cols["t"]))
    return SC.record(o, cols["t"], cols["s"], **{k: cols[k] for k in keep})


def self_merge_plans(n_targets):
    """a record merged with itself takes both paths: behind itself (concat), and onto itself under ADD (sort, every hit combined)
    -> ((bases, add, path), ...)"""
    return (((0, n_targets), False, "concat"), ((0, 0), True, "sort"))


# ---- the case builders ----
def split_unevenly(k, L):
    """how the three parts share a merged row of L hits: row k decides.  Some rows come whole from the last part, some are empty in
    the middle part"""
    if k % 4 == 0:
        return (0, 0, L)
    if k % 4 == 1:
        return (L - L // 3, 0, L // 3)
    a = L // 5
    return (a, L - a - L // 2, L // 2)


def row_length_parts(interleaved, seed=43, span=6000):
    """three parts whose merged rows have the lengths of MERGED_ROW_LENGTHS (and two rows nobody hits), with totals.
    interleaved False: every part draws from its own 0 .. span - 1 -> (parts, bases (0, span, 2 span)): the shards by target.
    interleaved True: part p draws the ids = p mod 3 of 0 .. 3 span - 1 -> (parts, equal bases): no pair twice, rows interleave."""
    rng = np.random.default_rng(seed)
    lens = list(MERGED_ROW_LENGTHS) + [0, 7]
    rows = [[], [], []]
    for k, L in enumerate(lens):
        for p, c in enumerate(split_unevenly(k, L)):
            ids = np.sort(rng.choice(span, size=c, replace=False))
            rows[p].append(3 * ids + p if interleaved else ids)
    parts = []
    for p in range(3):
        t = np.concatenate(rows[p] + [np.zeros(0, np.int64)]).astype(U32)
        s = rng.integers(1, 1000, len(t)).astype(U32)
        parts.append(SC.record(np.concatenate([[0], np.cumsum([len(x) for x in rows[p]])]), t, s, total=s + rng.integers(0, 50, len(t)).astype(U32)))
    return parts, ((0, 0, 0) if interleaved else (0, span, 2 * span))


def many_parts(n_parts, seed=47, nq=9, per_part=40):
    """n_parts small parts of per_part targets each, a few hits per row, the odd parts empty in the odd rows -> (parts, running bases)"""
    rng = np.random.default_rng(seed + n_parts)
    parts = []
    for p in range(n_parts):
        rec = TC.random_record(rng, nq, per_part, 5)
        if p % 2:
            keep = np.repeat(np.arange(nq) % 2 == 0, np.diff(rec["o"]).astype(np.int64))
            lens = np.where(np.arange(nq) % 2 == 0, np.diff(rec["o"]).astype(np.int64), 0)
            rec = SC.record(np.concatenate([[0], np.cumsum(lens)]), rec["t"][keep], rec["s"][keep], total=rec["total"][keep])
        parts.append(rec)
    return parts, tuple(per_part * p for p in range(n_parts))


def duplicate_parts():
    """the pair (row 1, target 5) in two parts; a pair twice inside part 2 (row 2, target 9); shared and total of 2^32 - 1 plus 1 in row 0
    -> (across, inside, saturating): lists of parts for equal bases"""
    a = SC.record([0, 1, 3, 3], [2, 4, 5], [MAX32, 7, 8], total=[MAX32, 9, 10])
    b = SC.record([0, 1, 2, 3], [2, 5, 9], [1, 11, 12], total=[1, 13, 14])
    c = SC.record([0, 0, 0, 3], [9, 3, 9], [20, 21, 22], total=[30, 31, 32])  # (not ascending, and 9 twice)
    return [a, b], [a, c], [a, b, c]


def caps_parts(interleaved, seed=53, nq=600, per_row=3):
    """600 rows, three parts of per_row hits a row each: more than 3 * 256 * 2 hits"""
    rng = np.random.default_rng(seed)
    parts = []
    for p in range(3):
        ids = np.sort(np.stack([rng.choice(50, size=per_row, replace=False) for _ in range(nq)]), axis=1)
        t = (3 * ids + p if interleaved else ids).reshape(-1).astype(U32)
        s = rng.integers(1, 9, len(t)).astype(U32)
        parts.append(SC.record(np.arange(nq + 1) * per_row, t, s, total=s + U32(3)))
    return parts, ((0, 0, 0) if interleaved else (0, 50, 100))


def value_shards(coll, counts, n_shards):
    """a collection (offsets, values) with counts split by value modulo n_shards -> [(collection, counts)]: every shard holds all sets"""
    o, v = np.asarray(coll[0], np.int64), np.asarray(coll[1], U64)
    sets = np.repeat(np.arange(len(o) - 1), np.diff(o))
    out = []
    for k in range(n_shards):
        m = (v % U64(n_shards)) == U64(k)
        oo = np.concatenate([[0], np.cumsum(np.bincount(sets[m], minlength=len(o) - 1))]).astype(U64)
        out.append(((oo, v[m]), None if counts is None else np.asarray(counts, U32)[m]))
    return out


def target_shards(coll, counts, cuts):
    """a collection split by set at `cuts` -> [(collection, counts)]: shard p holds the sets cuts[p] .. cuts[p + 1] - 1"""
    o, v = np.asarray(coll[0], np.int64), np.asarray(coll[1], U64)
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        lo, hi = int(o[a]), int(o[b])
        out.append((((o[a:b + 1] - lo).astype(U64), v[lo:hi]), None if counts is None else np.asarray(counts, U32)[lo:hi]))
    return out


def search_sets(seed=59, n_targets=37, n_queries=40):
    """37 counted target sets in families and 40 counted query sets drawn from them -> (targets, t_counts, queries, q_counts)"""
    rng = np.random.default_rng(seed)

    def coll(n, size):
        offs, vals, cnts = [0], [], []
        for i in range(n):
            fam = 1000 * (i % 6)
            v = np.unique(np.concatenate([fam + rng.choice(50, size=size, replace=False), 9000 + rng.choice(40, size=5, replace=False)])).astype(U64)
            vals.append(v), cnts.append(rng.integers(1, 7, len(v)).astype(U32)), offs.append(offs[-1] + len(v))
        return (np.asarray(offs, U64), np.concatenate(vals)), np.concatenate(cnts)

    t, tc = coll(n_targets, 22)
    q, qc = coll(n_queries, 16)
    return t, tc, q, qc


# ---- wrong models the cases must catch ----
def wrong_no_shift(recs, bases=None, add=False):
    return merge_model(recs, None, True)[0]


def wrong_part_order(recs, bases=None, add=False):
    """rows concatenated part after part, not sorted"""
    bases = [0] * len(recs) if bases is None else bases
    shifted = [dict(r, t=(r["t"].astype(np.int64) + int(b)).astype(U32)) for r, b in zip(recs, bases)]
    nq, keep = len(recs[0]["o"]) - 1, carried(recs)
    idx = [[(p, i) for p, r in enumerate(shifted) for i in range(int(r["o"][q]), int(r["o"][q + 1]))] for q in range(nq)]
    flat = [x for row in idx for x in row]
    return SC.record(np.concatenate([[0], np.cumsum([len(r) for r in idx])]), [shifted[p]["t"][i] for p, i in flat], [shifted[p]["s"][i] for p, i in flat],
                     **{k: [shifted[p][k][i] for p, i in flat] for k in keep})


def wrong_wraps(recs, bases=None, add=False):
    """sums modulo 2^32 / 2^64 instead of saturating"""
    out, _ = merge_model(recs, bases, add)
    out.update(merge_brute_wrapping(recs, bases))
    return out


def merge_brute_wrapping(recs, bases):
    bases = [0] * len(recs) if bases is None else [int(b) for b in bases]
    nq, keep = len(recs[0]["o"]) - 1, carried(recs)
    table = [dict() for _ in range(nq)]
    for r, b in zip(recs, bases):
        for q in range(nq):
            for i in range(int(r["o"][q]), int(r["o"][q + 1])):
                cell = table[q].setdefault(int(r["t"][i]) + b, {k: 0 for k in ("s",) + keep})
                for k in cell:
                    cell[k] = (cell[k] + int(r[k][i])) & LIMITS[k]
    return {k: np.asarray([table[q][t][k] for q in range(nq) for t in sorted(table[q])], U32 if LIMITS[k] == MAX32 else U64) for k in ("s",) + keep}


def wrong_keeps_all_payloads(recs, bases=None, add=False):
    """the payloads of the first part, not the intersection"""
    out, _ = merge_model(recs, bases, add)
    for k in PAYLOADS:
        if out[k] is None and recs[0][k] is not None:
            out[k] = np.zeros(len(out["t"]), recs[0][k].dtype)
    return out
