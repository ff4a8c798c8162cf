"""NumPy model of the hits by target (include/biosketch.h "hits by target") and the cases its tests run.

transpose_model: a stable argsort of target over the CSR order, every payload gathered by it; a hit's query becomes its target.
tally_model: three bincounts.  Records are those of tests/select_cases.py (record / same / take)."""
import numpy as np

from tests import select_cases as SC

U64, U32 = np.uint64, np.uint32
PAYLOADS = SC.PAYLOADS
TALLY_LDS_TARGETS = 2048  # transpose.hip TL_LDS_TARGETS: up to here the counters live in LDS
TARGET_ROW_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000)
KEY_WIDTH_TARGETS = (1, 2, 3, 256, 257, 65536, 65537, 70000)


def rows_of(o):
    """the query of every hit"""
    o = np.asarray(o, U64)
    return np.repeat(np.arange(len(o) - 1, dtype=np.int64), np.diff(o).astype(np.int64))


def transpose_model(rec, n_targets):
    t = rec["t"].astype(np.int64)
    if len(t) and int(t.max()) >= n_targets:
        raise SC.BadHits("a target >= n_targets")
    order = np.argsort(t, kind="stable")
    o = np.concatenate([[0], np.cumsum(np.bincount(t, minlength=n_targets))]).astype(U64)
    out = dict(o=o, t=rows_of(rec["o"])[order].astype(U32), s=rec["s"][order])
    for p in PAYLOADS:
        out[p] = None if rec[p] is None else rec[p][order]
    return out


def transpose_brute(rec, n_targets):
    """the same by a double loop: for every target, every query in order, every hit of the row in order"""
    o, idx, offs = rec["o"], [], [0]
    qs = []
    for t in range(n_targets):
        for q in range(len(o) - 1):
            for i in range(int(o[q]), int(o[q + 1])):
                if int(rec["t"][i]) == t:
                    idx.append(i), qs.append(q)
        offs.append(len(idx))
    out = SC.take(rec, idx, offs)
    out["t"] = np.asarray(qs, U32)
    return out


def tally_model(rec, n_targets, into=None):
    """(rows, unique, shared) u64 per target; into: the table to add to (modulo 2^64), left unchanged"""
    t = rec["t"].astype(np.int64)
    if len(t) and int(t.max()) >= n_targets:
        raise SC.BadHits("a target >= n_targets")
    lens = np.diff(rec["o"]).astype(np.int64)
    alone = np.repeat(lens == 1, lens)
    rows = np.bincount(t, minlength=n_targets).astype(U64)
    unique = np.bincount(t[alone], minlength=n_targets).astype(U64)
    shared = np.zeros(n_targets, U64)
    np.add.at(shared, t, rec["s"].astype(U64))  # (bincount's weights are doubles: not exact beyond 2^53)
    got = (rows, unique, shared)
    return got if into is None else tuple(a + b for a, b in zip(into, got))  # (u64 arrays wrap)


def tally_brute(rec, n_targets):
    o = rec["o"]
    rows, unique, shared = [0] * n_targets, [0] * n_targets, [0] * n_targets
    for q in range(len(o) - 1):
        a, b = int(o[q]), int(o[q + 1])
        for i in range(a, b):
            t = int(rec["t"][i])
            rows[t] += 1
            shared[t] += int(rec["s"][i])
            unique[t] += b - a == 1
    return tuple(np.asarray(x, U64) for x in (rows, unique, shared))


def same_table(a, b):
    """'' where two tables agree, else what differs"""
    for name, x, y in zip(("rows", "unique", "shared"), a, b):
        if x.dtype != U64 or y.dtype != U64 or not np.array_equal(x, y):
            return name
    return ""


def concat(recs):
    """the rows of several records one after another (the payloads of the first; all must carry the same)"""
    o = np.concatenate([[0]] + [r["o"][1:].astype(np.int64) + sum(len(x["t"]) for x in recs[:k]) for k, r in enumerate(recs)]).astype(U64)
    out = dict(o=o)
    for k in ("t", "s") + PAYLOADS:
        out[k] = None if recs[0][k] is None else np.concatenate([r[k] for r in recs])
    return out


# ---- the case builders ----
def random_record(rng, nq, nt, max_len, payloads=("total",), ascending=True, repeats=False):
    """small random hits; ascending=False shuffles inside the rows (top-n output), repeats lets a row name a target twice"""
    lens = rng.integers(0, max_len + 1, nq)
    t = []
    for c in lens:
        row = rng.integers(0, nt, c) if repeats else rng.choice(nt, size=min(int(c), nt), replace=False)
        t.append(np.sort(row) if ascending else row)
    lens = [len(x) for x in t]
    t = np.concatenate(t + [np.zeros(0, np.int64)]).astype(U32)
    H = len(t)
    rec = SC.record(np.concatenate([[0], np.cumsum(lens)]), t, rng.integers(1, 9, H),
                    total=rng.integers(9, 30, H) if "total" in payloads else None, dot=rng.integers(1, 1 << 40, H) if "dot" in payloads else None,
                    msum=rng.integers(1, 1 << 40, H) if "dot" in payloads else None, members=rng.integers(1, 5, H) if "members" in payloads else None)
    return rec


def row_length_record(with_total=True, seed=19):
    """3 001 queries; the targets 10 k (k = 0 .. 14) are listed by TARGET_ROW_LENGTHS[k] queries -- one target's row is longer than a
    workgroup --, the targets between them by nobody, and neither are the last 50 of the 200 targets.  -> (record, n_targets)"""
    rng = np.random.default_rng(seed)
    nq, nt = 3001, 200
    hit = np.zeros((nq, len(TARGET_ROW_LENGTHS)), bool)
    for k, c in enumerate(TARGET_ROW_LENGTHS):
        hit[rng.choice(nq, size=c, replace=False), k] = True
    qs, ks = np.nonzero(hit)  # row-major: by query, targets ascending inside a row
    t = (10 * ks).astype(U32)
    o = np.concatenate([[0], np.cumsum(hit.sum(1))]).astype(U64)
    s = rng.integers(1, 1000, len(t)).astype(U32)
    return SC.record(o, t, s, total=s + rng.integers(0, 50, len(t)).astype(U32) if with_total else None), nt


def key_width_record(n_targets, seed=23):
    """a handful of hits that include target n_targets - 1, in 5 rows (one of them empty)"""
    rng = np.random.default_rng(seed + n_targets)
    rows = [sorted({n_targets - 1, 0}), [], sorted(set(rng.integers(0, n_targets, 4).tolist())), [n_targets - 1], sorted(set(rng.integers(0, n_targets, 7).tolist()))]
    t = np.asarray([x for r in rows for x in r], U32)
    return SC.record(np.concatenate([[0], np.cumsum([len(r) for r in rows])]), t, rng.integers(1, 1 << 32, len(t), dtype=np.uint64), total=rng.integers(1, 1 << 32, len(t), dtype=np.uint64))


def unique_record():
    """rows of 0, 1 and 2 hits: unique counts the rows of one"""
    return SC.record([0, 0, 1, 3, 4, 4, 6, 7], [2, 0, 2, 2, 1, 2, 0], [5, 1, 2, 3, 4, 6, 7])


def spread_record(nt, per_target=3, one_target=None, seed=29):
    """hits spread evenly over nt targets, per_target each, in rows of one or two hits -- or every hit on one target, a row each, with
    rows without hits between them.  shared is near 2^32: a target's sum passes 32 bits."""
    rng = np.random.default_rng(seed)
    H = nt * per_target
    if one_target is None:  # pass p lists the targets from 7 p on, cyclically: neighbours in the list differ, a row is cut from neighbours
        t = np.concatenate([(np.arange(nt) + 7 * p) % nt for p in range(per_target)]).astype(U32)
        cut = np.cumsum(rng.integers(1, 3, H))
        o = np.concatenate([[0], cut[cut < H], [H]]).astype(U64)
        for a, b in zip(o[:-1], o[1:]):
            t[int(a):int(b)] = np.sort(t[int(a):int(b)])
    else:
        t = np.full(H, one_target, U32)
        lens = rng.permutation(np.concatenate([np.ones(H, np.int64), np.zeros(H // 3, np.int64)]))  # a quarter of the rows are empty, the others hold one hit
        o = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    return SC.record(o, t, rng.integers(1 << 31, 1 << 32, H, dtype=np.uint64))


def symmetric_sets(seed=31, n=40):
    """two counted collections of n sets with crafted overlaps: set i of either side draws from family i % 5, so that pairs of a family
    share many values and pairs across families few or none.  -> ((offsets, values, counts) of a, of b)"""
    rng = np.random.default_rng(seed)
    out = []
    for side in range(2):
        offs, vals, cnts = [0], [], []
        for i in range(n + 2 * side):  # the sides differ in length: rectangular hits
            fam = 1000 * (i % 5)
            v = np.unique(np.concatenate([fam + rng.choice(60, size=24, replace=False), 9000 + rng.choice(200, size=4, replace=False)])).astype(U64)
            vals.append(v), cnts.append(rng.integers(1, 7, len(v)).astype(U32)), offs.append(offs[-1] + len(v))
        out.append((np.asarray(offs, U64), np.concatenate(vals), np.concatenate(cnts)))
    return tuple(out)


# ---- wrong models the cases must catch ----
def wrong_unstable(rec, nt):
    """equal targets in reverse CSR order"""
    out = transpose_model(rec, nt)
    o = out["o"]
    for a, b in zip(o[:-1], o[1:]):
        for k in ("t", "s") + PAYLOADS:
            if out[k] is not None:
                out[k][int(a):int(b)] = out[k][int(a):int(b)][::-1].copy()
    return out


def wrong_payload_stays(rec, nt):
    out = transpose_model(rec, nt)
    out["s"] = rec["s"].copy()
    return out


def wrong_drops_trailing(rec, nt):
    out = transpose_model(rec, nt)
    last = int(rec["t"].max()) + 1 if len(rec["t"]) else 0
    out["o"] = out["o"][:last + 1]
    return out


def wrong_total_stays(rec, nt):
    out = transpose_model(rec, nt)
    out["total"] = None if rec["total"] is None else rec["total"].copy()
    return out


def wrong_unique_per_hit(rec, nt, into=None):
    rows, _, shared = tally_model(rec, nt)
    got = (rows, rows.copy(), shared)
    return got if into is None else tuple(a + b for a, b in zip(into, got))


def wrong_add_overwrites(rec, nt, into=None):
    return tally_model(rec, nt)
