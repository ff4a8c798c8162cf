"""The weighted containment search's host-side restatement and its crafted cases (include/biosketch.h "weighted containment search",
search.hip: bsk_index_build_counted, bsk_index_search_counted).

ref_search_counted is tests/search_cases.ref_search -- the rows are the unweighted search's, the thresholds read shared alone -- plus
dot and min_sum of every listed pair by a dict walk over the postings in Python ints, saturated at the end.  SW_ROW and SW_CHUNK restate
the two caps of the payload pass; paths() says which kernel every query takes, so a GPU test can hold the plan text against it.
tests/test_search_counted_cases.py checks all of it without a device."""
import os
import re

import numpy as np

from tests import search_cases as SC

U64 = np.uint64
MAX = (1 << 64) - 1
M32 = (1 << 32) - 1
SR_CAP = SC.SR_CAP
SW_ROW = 512    # search.hip: hits of a small-path query's row that one wavefront of k_sw_row holds in LDS
SW_CHUNK = 256  # search.hip: query values one wavefront of k_sw_chunk walks
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read_caps(path=os.path.join(ROOT, "bio_amd", "csrc", "search.hip")):
    """the #defines of search.hip by name"""
    return {k: int(v) for k, v in re.findall(r"^#define (S[RW]_\w+) (\d+)\b", open(path).read(), re.M)}


# ---- the reference ----
def postings(t_offs, t_vals, t_cnt=None):
    """value -> (targets ascending, their counts of the value); t_cnt None: every count 1"""
    tid = np.repeat(np.arange(len(t_offs) - 1, dtype=np.int64), np.diff(t_offs).astype(np.int64))
    cnt = np.ones(len(t_vals), np.int64) if t_cnt is None else np.asarray(t_cnt, np.int64)
    post = {}
    for v, t, c in zip(t_vals.tolist(), tid.tolist(), cnt.tolist()):
        post.setdefault(v, ([], []))
        post[v][0].append(t)
        post[v][1].append(c)
    return post


def ref_weights(post, q_offs, q_vals, q_cnt, offsets, target):
    """dot (min(sum, 2^64 - 1)) and min_sum of the listed pairs (offsets, target): for every posting (t, ct) of every query value (v, cq)
    whose t the query's row lists, cq * ct and min(cq, ct) added in Python ints"""
    dot, ms = [0] * len(target), [0] * len(target)
    qc = np.ones(len(q_vals), np.int64) if q_cnt is None else np.asarray(q_cnt, np.int64)
    qv, qc, o, qo = q_vals.tolist(), qc.tolist(), offsets.astype(np.int64).tolist(), q_offs.astype(np.int64).tolist()
    for q in range(len(qo) - 1):
        if o[q] == o[q + 1]:
            continue
        at = {t: o[q] + j for j, t in enumerate(target[o[q]:o[q + 1]].tolist())}
        for i in range(qo[q], qo[q + 1]):
            hit = post.get(qv[i])
            if hit is None:
                continue
            cq = qc[i]
            for t, ct in zip(*hit):
                k = at.get(t)
                if k is not None:
                    dot[k] += cq * ct
                    ms[k] += min(cq, ct)
    return np.array([min(d, MAX) for d in dot], U64), np.array(ms, U64)


def ref_search_counted(tg, t_cnt, qs, q_cnt, min_shared=1, qc=0.0, tc=0.0):
    """-> (offsets, target, shared, dot, min_sum) by the contract, computed on the host"""
    o, t, s = SC.ref_search(*tg, *qs, min_shared, qc, tc)
    d, m = ref_weights(postings(*tg, t_cnt), qs[0], qs[1], q_cnt, o, t)
    return o, t, s, d, m


def brute(tg, t_cnt, qs, q_cnt, min_shared=1, qc=0.0, tc=0.0, bug=None):
    """the same numbers pair by pair -- every (query, target) intersected as two dicts, the header's rule applied to the pair -- and,
    with `bug`, one of the wrong models a test of the model must tell from the right one"""
    (to, tv), (qo, qv) = tg, qs
    tcn = np.ones(len(tv), np.int64) if t_cnt is None else np.asarray(t_cnt, np.int64)
    qcn = np.ones(len(qv), np.int64) if q_cnt is None else np.asarray(q_cnt, np.int64)
    if bug == "uncounted is 0":
        tcn = tcn * (t_cnt is not None)
        qcn = qcn * (q_cnt is not None)
    to, qo = to.astype(np.int64), qo.astype(np.int64)
    tsets = [dict(zip(tv[to[t]:to[t + 1]].tolist(), tcn[to[t]:to[t + 1]].tolist())) for t in range(len(to) - 1)]
    if bug == "permuted postings":  # the counts of a value's holders rotated by one holder
        holders = {}
        for t, d in enumerate(tsets):
            for v in d:
                holders.setdefault(v, []).append(t)
        for v, hs in holders.items():
            cs = [tsets[t][v] for t in hs]
            for t, c in zip(hs, cs[1:] + cs[:1]):
                tsets[t][v] = c
    offs, tgt, sh, dot, ms = [0], [], [], [], []
    stray = 0
    for q in range(len(qo) - 1):
        qd = dict(zip(qv[qo[q]:qo[q + 1]].tolist(), qcn[qo[q]:qo[q + 1]].tolist()))
        for t, td in enumerate(tsets):
            common = [v for v in qd if v in td]
            s = len(common)
            d = sum((qd[v] * qd[v] if bug == "wrong operand" else qd[v] * td[v]) for v in common)
            m = sum((qd[v] * td[v] if bug == "product for min" else min(qd[v], td[v])) for v in common)
            if s >= max(min_shared, 1) and float(s) >= qc * float(len(qd)) and float(s) >= tc * float(len(td)):
                tgt.append(t), sh.append(s)
                dot.append((d + stray) & MAX if bug == "wrap" else min(d + stray, MAX))
                ms.append(m & MAX)
                stray = 0
            elif bug == "unlisted pairs":  # the weights of a dropped pair land on the next listed one
                stray += d
        offs.append(len(tgt))
    return np.array(offs, U64), np.array(tgt, np.uint32), np.array(sh, np.uint32), np.array(dot, U64), np.array(ms, U64)


BUGS = ("wrong operand", "product for min", "wrap", "unlisted pairs", "uncounted is 0", "permuted postings")


def paths(sums, q_offs, offsets):
    """which kernel of the payload pass every query takes -> (in_row bool[nq], chunks int[nq]): k_sw_row for a query with hits whose
    posting sum is at most SR_CAP and whose row holds at most SW_ROW hits, else ceil(|q| / SW_CHUNK) chunks of k_sw_chunk"""
    h, n = np.diff(offsets.astype(np.int64)), np.diff(q_offs.astype(np.int64))
    in_row = (h > 0) & (np.asarray(sums) <= SR_CAP) & (h <= SW_ROW)
    chunks = np.where((h > 0) & ~in_row, (n + SW_CHUNK - 1) // SW_CHUNK, 0)
    return in_row, chunks


def plan_tail(sums, q_offs, offsets):
    """what bsk_hits_plan appends to the search's own text"""
    in_row, chunks = paths(sums, q_offs, offsets)
    return "; weights: k_sw_row %d queries (<= %d hits), k_sw_chunk %d chunks of %d values" % (int(in_row.sum()), SW_ROW, int(chunks.sum()), SW_CHUNK)


# ---- counts for the crafted cases of tests/search_cases.py ----
def seeded_counts(n, seed, kind="mixed"):
    """n counts (u32, never 0): "small" 1..9; "mixed" small ones with a tenth of 1 and a tenth of 2^32 - 1; "max" all 2^32 - 1"""
    rng = np.random.default_rng(seed)
    if kind == "max":
        return np.full(n, M32, np.uint32)
    c = rng.integers(1, 10, n).astype(np.uint32)
    if kind == "mixed":
        r = rng.random(n)
        c[r < 0.1] = 1
        c[r > 0.9] = M32
    return c


def with_counts(tg, qs, seed, kind="mixed"):
    """seeded counts for a case's targets and queries -> (t_cnt, q_cnt)"""
    return seeded_counts(len(tg[1]), seed, kind), seeded_counts(len(qs[1]), seed + 1, kind)


# ---- crafted cases of the payload pass's own caps ----
ROW_EDGES = (SW_ROW - 1, SW_ROW, SW_ROW + 1)


def row_edge_case():
    """small-path queries whose rows hold SW_ROW - 1, SW_ROW and SW_ROW + 1 hits.  Target t < 600 holds A + t; the even targets below 400
    also hold C (a posting list of 200: walked by the whole wavefront) and the targets t < 500 with t % 5 == 0 hold D.  Query n is
    A .. A + n - 1 plus C and D: n hits (n > 500), shared 1 to 3, posting sum n + 200 + 100 <= SR_CAP.  A fourth query holds C alone."""
    A, C, D = 1 << 30, 7, 9
    tsets = [[A + t] + ([C] if t % 2 == 0 and t < 400 else []) + ([D] if t % 5 == 0 and t < 500 else []) for t in range(600)]
    qsets = [[C, D] + [A + i for i in range(n)] for n in ROW_EDGES] + [[C]]
    sums = [n + 300 for n in ROW_EDGES] + [200]
    return SC.collection(tsets), SC.collection(qsets), SC.claims(sums), dict(hits=list(ROW_EDGES) + [200])


CHUNK_EDGES = (SW_CHUNK - 1, SW_CHUNK, SW_CHUNK + 1, 2 * SW_CHUNK, 2 * SW_CHUNK + 1)


def chunk_edge_case(seed=71):
    """large-path queries of SW_CHUNK - 1, SW_CHUNK, SW_CHUNK + 1, 2 SW_CHUNK and 2 SW_CHUNK + 1 values: each holds H, which 2 100 of
    2 600 targets hold (so its posting sum exceeds SR_CAP), and values held by 0 to 3 targets; between them small queries"""
    b = SC.Builder(2600, seed)
    h = b.value(2100)
    for n in CHUNK_EDGES:
        b.query(sorted([h] + [b.value(int(c)) for c in b.rng.integers(0, 4, n - 1)]))
        b.query_counts([int(c) for c in b.rng.integers(0, 4, 5)])
    tg, qs, cl = b.build()
    return tg, qs, cl, dict(values=[n for n in CHUNK_EDGES for _ in (0, 1)])


def saturation_case(large):
    """dot at the edge of u64, with M = 2^32 - 1 (M * M = 2^64 - 2^33 + 1, so M * M + 2 * M = 2^64 - 1).  Four targets against one
    query of the values 1 .. 4 with counts (M, 2, 1, M):
      target 0 holds 1, 2 with (M, M):          dot = M*M + 2M     = 2^64 - 1 exactly, min_sum = M + 2
      target 1 holds 1, 3 with (M, M):          dot = M*M + M      < 2^64 - 1,         min_sum = M + 1
      target 2 holds 1, 2, 3 with (M, M, 1):    dot = M*M + 2M + 1 = 2^64: saturates,  min_sum = M + 3
      target 3 holds 1, 4 with (M, M):          dot = 2 M*M: wraps once, saturates,    min_sum = 2M > 2^32
      target 4 holds 1, 2, 3, 4 with M each:    dot = 2 M*M + 3M wraps, saturates,     min_sum = 2M + 3
    large: the query also holds H, which targets 5 .. 2 104 hold with count 1 (posting sum > SR_CAP: the atomics of k_sw_chunk)."""
    M = M32
    tsets = [([1, 2], [M, M]), ([1, 3], [M, M]), ([1, 2, 3], [M, M, 1]), ([1, 4], [M, M]), ([1, 2, 3, 4], [M, M, M, M])]
    q, qc = [1, 2, 3, 4], [M, 2, 1, M]
    if large:
        tsets += [([100], [1])] * 2100
        q, qc = q + [100], qc + [3]
    tg = SC.collection([s for s, _ in tsets])
    t_cnt = np.array([c for _, cs in tsets for c in cs], np.uint32)
    qs = SC.collection([q])
    want = dict(dot=[MAX, M * M + M, MAX, MAX, MAX], min_sum=[M + 2, M + 1, M + 3, 2 * M, 2 * M + 3])
    return tg, t_cnt, qs, np.array(qc, np.uint32), SC.claims([13 + (2100 if large else 0)]), want
