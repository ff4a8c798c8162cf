"""The model of bsk_hits_filter and bsk_hits_top_by (include/biosketch.h "hits selected by a measure") in Python integers, and the
generators of the crafted hits the GPU test runs.  A record is a dict: o (offsets), t (target), s (shared) and the payloads total, dot,
msum, members -- an array, or None where the hits carry none."""
import functools

import numpy as np

U64, U32 = np.uint64, np.uint32
TOP64 = (1 << 64) - 1
MEASURES = ("shared", "members", "dot", "min_sum", "query_cov", "target_cov", "jaccard", "cosine", "weighted_jaccard", "bray_curtis_similarity", "weighted_containment")
PAYLOADS = ("total", "dot", "msum", "members")
ROW_LENGTHS = (0, 1, 15, 16, 17, 64, 65, 1023, 1024, 1025, 2049)  # both sides of 16 and 1 024, a non-power-of-two on the global path
TOP_NS = (1, 3, 16, 17, 1000, 5000)


class BadHits(ValueError):
    """what the library answers with BSK_ERR_ARG from its device pass: a target beyond tnorm, a denominator that is not positive"""


def record(o, t, s, total=None, dot=None, msum=None, members=None):
    return dict(o=np.asarray(o, U64), t=np.asarray(t, U32), s=np.asarray(s, U32), total=None if total is None else np.asarray(total, U32),
                dot=None if dot is None else np.asarray(dot, U64), msum=None if msum is None else np.asarray(msum, U64),
                members=None if members is None else np.asarray(members, U32))


def needs(measure, rec):
    """(payloads, norms) the measure reads: a tuple of payload names, a string of 'q' and 't'"""
    return {"shared": ((), ""), "members": (("members",), ""), "dot": (("dot",), ""), "min_sum": (("msum",), ""), "query_cov": ((), "q"), "target_cov": ((), "t"),
            "jaccard": ((), "" if rec["total"] is not None else "qt"), "cosine": (("dot",), "qt"), "weighted_jaccard": (("msum",), "qt"),
            "bray_curtis_similarity": (("msum",), "qt"), "weighted_containment": (("dot",), "q")}[measure]


def applies(measure, rec):
    return all(rec[p] is not None for p in needs(measure, rec)[0])


def nd(measure, rec, q, i, qnorm=None, tnorm=None):
    """(N, D) of hit i of row q: the header's table, in Python integers"""
    sides = needs(measure, rec)[1]
    t = int(rec["t"][i])
    if "t" in sides and t >= len(tnorm):
        raise BadHits("target >= n_tnorm")
    Q = int(qnorm[q]) if "q" in sides else 0
    T = int(tnorm[t]) if "t" in sides else 0
    s = int(rec["s"][i])
    if measure == "shared":
        N, D = s, 1
    elif measure == "members":
        N, D = int(rec["members"][i]), 1
    elif measure == "dot":
        N, D = int(rec["dot"][i]), 1
    elif measure == "min_sum":
        N, D = int(rec["msum"][i]), 1
    elif measure == "query_cov":
        N, D = s, Q
    elif measure == "target_cov":
        N, D = s, T
    elif measure == "jaccard":
        N, D = s, (int(rec["total"][i]) if rec["total"] is not None else Q + T - s)
    elif measure == "cosine":
        N, D = int(rec["dot"][i]) ** 2, Q * T
    elif measure == "weighted_jaccard":
        N, D = int(rec["msum"][i]), Q + T - int(rec["msum"][i])
    elif measure == "bray_curtis_similarity":
        N, D = 2 * int(rec["msum"][i]), Q + T
    elif measure == "weighted_containment":
        N, D = int(rec["dot"][i]), Q
    else:
        raise KeyError(measure)
    if D <= 0:
        raise BadHits("D <= 0")
    return N, D


def all_nd(measure, rec, qnorm=None, tnorm=None):
    o = rec["o"]
    return [nd(measure, rec, q, i, qnorm, tnorm) for q in range(len(o) - 1) for i in range(int(o[q]), int(o[q + 1]))]


def kept(measure, N, D, num, den):
    """the filter's rule; the cosine's bound is on the cosine itself, N / D is its square"""
    if measure == "cosine":
        return N * den * den >= num * num * D
    return N * den >= num * D


def before(a, b):
    """hit a = (N, D, target) is better than hit b"""
    x, y = a[0] * b[1], b[0] * a[1]
    return x > y or (x == y and a[2] < b[2])


def take(rec, idx, offsets):
    idx = np.asarray(idx, np.int64)
    return dict(o=np.asarray(offsets, U64), **{k: (None if rec[k] is None else rec[k][idx]) for k in ("t", "s") + PAYLOADS})


def filter_model(rec, measure, num, den, qnorm=None, tnorm=None, fractions_=None):
    fr = fractions_ if fractions_ is not None else all_nd(measure, rec, qnorm, tnorm)
    o, idx, offs = rec["o"], [], [0]
    for q in range(len(o) - 1):
        idx += [i for i in range(int(o[q]), int(o[q + 1])) if kept(measure, fr[i][0], fr[i][1], num, den)]
        offs.append(len(idx))
    return take(rec, idx, offs)


def ranked_rows(rec, measure, qnorm=None, tnorm=None, fractions_=None):
    """per row its hit indices, best first: what every n of top_by_model cuts its prefix from"""
    fr = fractions_ if fractions_ is not None else all_nd(measure, rec, qnorm, tnorm)
    o, t = rec["o"], rec["t"]
    key = functools.cmp_to_key(lambda i, j: -1 if before((fr[i][0], fr[i][1], int(t[i])), (fr[j][0], fr[j][1], int(t[j]))) else 1)
    return [sorted(range(int(o[q]), int(o[q + 1])), key=key) for q in range(len(o) - 1)]


def top_by_model(rec, measure, n, qnorm=None, tnorm=None, rows=None):
    rows = rows if rows is not None else ranked_rows(rec, measure, qnorm, tnorm)
    idx, offs = [], [0]
    for r in rows:
        idx += r[:n]
        offs.append(len(idx))
    return take(rec, idx, offs)


def same(a, b):
    """'' where two records agree in every array, else what differs"""
    for k in ("o", "t", "s") + PAYLOADS:
        if (a[k] is None) != (b[k] is None):
            return "%s: carried by one only" % k
        if a[k] is not None and not (a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k])):
            return "%s differs" % k
    return ""


def step_above(N, D):
    """(num, den) u64 with num / den the smallest fraction above N / D that a denominator D * M < 2^64 can express: the threshold
    the hit itself must fail.  M is as large as fits, so the parts come near 2^64."""
    M = TOP64 // max(N + 1, D)
    return (N * M + 1, D * M) if M >= 1 else None


# ---- crafted hits ----
def shape_record(seed=7, with_total=True):
    """one object of a few thousand hits with every row length of ROW_LENGTHS (and a second 1 025 row, so that the global path has
    two rows).  shared comes from a handful of values, so every row is full of ties; total is crafted so that equal fractions come
    from different N and D (2/4 and 3/6), equal measure meets different shared, and one row is tied as a whole."""
    rng = np.random.default_rng(seed)
    lengths = list(ROW_LENGTHS) + [1025, 16, 0, 33]
    o, t, s, tot = [0], [], [], []
    for r, c in enumerate(lengths):
        tg = np.sort(rng.choice(4200, size=c, replace=False)).astype(U32)
        sh = rng.integers(1, 7, c).astype(U32)
        mult = rng.integers(2, 5, c).astype(U32)  # total = shared * {2, 3, 4}: 2/4 = 3/6 = 1/2, 1/3 = 2/6, ...
        if r == 5:  # a whole row tied: one shared, one total
            sh[:], mult[:] = 3, 2
        t.append(tg), s.append(sh), tot.append(sh * mult)
        o.append(o[-1] + c)
    return record(o, np.concatenate(t), np.concatenate(s), np.concatenate(tot) if with_total else None)


def shape_sizes(rec, seed=11):
    """set sizes consistent with the record (|q| >= shared, |t| >= shared), from a few values: ties in the covers and the Jaccard"""
    rng = np.random.default_rng(seed)
    return (rng.integers(6, 12, len(rec["o"]) - 1).astype(U64), rng.integers(6, 12, 4200).astype(U64))


def weighted_sets(seed=3, n_targets=2100):
    """counted sets whose neighbours have every row length of ROW_LENGTHS: target t holds the values 2t and 2t + 1 and no other set of
    the targets holds them, query j holds one or both values of its first L_j targets -- a row of exactly L_j hits with shared 1 or 2
    and, counts coming from 1 .. 3, dot and min_sum full of ties.  -> (offsets, values, counts) of the queries and of the targets"""
    rng = np.random.default_rng(seed)
    tv = np.arange(2 * n_targets, dtype=U64)
    to = np.arange(0, 2 * n_targets + 1, 2, dtype=U64)
    tc = rng.integers(1, 4, 2 * n_targets).astype(U32)
    qo, qv, qc = [0], [], []
    for L_j in list(ROW_LENGTHS) + [1025, 40]:
        both = rng.integers(0, 2, L_j).astype(bool)
        v = np.sort(np.concatenate([2 * np.arange(L_j, dtype=U64), (2 * np.arange(L_j, dtype=U64) + U64(1))[both]]))
        qv.append(v), qc.append(rng.integers(1, 4, len(v)).astype(U32))
        qo.append(qo[-1] + len(v))
    return (np.array(qo, U64), np.concatenate(qv), np.concatenate(qc)), (to, tv, tc)


def wide_sets():
    """counts at the edge of the formats, two queries against four targets:
    query 0, target 0: one value of count 2^32-1 on both sides, the only one of both sets -- dot = (2^32-1)^2 = both norms: a cosine of exactly 1;
    query 1, target 1: two such values -- the true dot is 2 (2^32-1)^2 >= 2^64: saturated;
    query 1, targets 2 and 3: dot = 3 * 2^32 and 5 * 2^32 -- N = dot^2 is a multiple of 2^64."""
    m, k = (1 << 32) - 1, 1 << 16
    q = (np.array([0, 1, 5], U64), np.array([10, 20, 21, 30, 40], U64), np.array([m, m, m, 3 * k, 5 * k], U32))
    t = (np.array([0, 1, 3, 4, 5], U64), np.array([10, 20, 21, 30, 40], U64), np.array([m, m, m, k, k], U32))
    return q, t
