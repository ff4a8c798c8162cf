"""The NumPy model of bsk_result_sets_windows and bsk_hits_fold (include/biosketch.h "window sets and folded hits"), fed with HOST tuples
(BatchResult.fetch) and host hits, so that it shares no code with the device path.  tests/test_window_cases.py checks it against a second
formulation; the GPU tests compare the device against it, integer for integer."""
import numpy as np

U64, U32, I64 = np.uint64, np.uint32, np.int64
POS_MASK = 0x7FFFFFFF
SAT = 0xFFFFFFFF


def positions(offsets, pos):
    """position of every tuple: pos without the strand bit, or the tuple's index inside its sequence for the every-position kinds"""
    offsets = np.asarray(offsets, I64)
    if pos is not None:
        return (np.asarray(pos, I64) & POS_MASK)
    T = int(offsets[-1])
    return np.arange(T, dtype=I64) - np.repeat(offsets[:-1], np.diff(offsets))


def window_rule(p_last, window, step, count):
    """(W, S) per sequence from the sequences' last positions"""
    p_last = np.asarray(p_last, I64)
    if count:
        W = np.maximum(1, -(-(p_last + 1) // count))
        return W, W.copy()
    W = np.full(len(p_last), window, I64)
    return W, np.full(len(p_last), step if step else window, I64)


def first_window(p, W, S):
    return np.where(p < W, 0, (p - W) // S + 1)


def windows_model(offsets, hash_, pos, window=0, step=0, count=0, scale=1):
    """-> (seq_offsets[n + 1], set_offsets[n_sets + 1], values, counts): the window sets of host tuples, values ascending and distinct inside a
    set, counts = their run lengths inside the window (what BSK_WINDOWS_COUNTED carries)"""
    offsets = np.asarray(offsets, I64)
    hash_ = np.asarray(hash_, U64)
    n, c = len(offsets) - 1, np.diff(offsets)
    p = positions(offsets, pos)
    has = c > 0
    p_last = np.zeros(n, I64)
    p_last[has] = p[offsets[1:][has] - 1]
    W, S = window_rule(p_last, window, step, count)
    nwin = np.where(has, first_window(p_last, W, S) + 1, 0)
    seq_off = np.concatenate([[0], np.cumsum(nwin)]).astype(I64)
    n_sets = int(seq_off[-1])
    seq = np.repeat(np.arange(n, dtype=I64), c)
    w0 = first_window(p, W[seq], S[seq])
    w1 = np.minimum(p // S[seq], nwin[seq] - 1)  # window w holds p iff first(p) <= w <= p / S
    mult = w1 - w0 + 1
    assert (mult >= 1).all()  # every tuple lies in at least one window
    idx = np.repeat(np.arange(len(p), dtype=I64), mult)
    k = np.arange(int(mult.sum()), dtype=I64) - np.repeat(np.cumsum(mult) - mult, mult)
    sid = seq_off[seq[idx]] + w0[idx] + k
    hv = hash_[idx]
    keep = hv <= U64(0xFFFFFFFFFFFFFFFF // scale) if scale > 1 else np.ones(len(hv), bool)
    sid, hv = sid[keep], hv[keep]
    order = np.lexsort((hv, sid))
    sid, hv = sid[order], hv[order]
    head = np.ones(len(hv), bool)
    head[1:] = (sid[1:] != sid[:-1]) | (hv[1:] != hv[:-1])
    at = np.flatnonzero(head)
    counts = np.diff(np.concatenate([at, [len(hv)]])).astype(U32)
    set_off = np.concatenate([[0], np.cumsum(np.bincount(sid[head], minlength=n_sets))]).astype(U64)
    return seq_off.astype(U64), set_off, hv[head], counts


def sets_per_sequence(offsets, hash_, scale=1):
    """bsk_result_sets(PER_SEQUENCE) of host tuples -> (set_offsets, values): what reducing a sequence's windows must give back"""
    maxhash = U64(0xFFFFFFFFFFFFFFFF // scale if scale > 1 else 0xFFFFFFFFFFFFFFFF)
    parts = [np.unique(np.asarray(hash_[int(a):int(b)], U64)) for a, b in zip(offsets[:-1], offsets[1:])]
    parts = [v[v <= maxhash] for v in parts]
    return np.concatenate([[0], np.cumsum([len(v) for v in parts])]).astype(U64), (np.concatenate(parts) if parts else np.zeros(0, U64))


def fold_model(offsets, target, shared, group_offsets, min_members=1, frac=None):
    """-> (offsets, target = group, shared, members) of bsk_hits_fold: per row one hit for every group with a hit target that passes the rule;
    shared summed and saturated, members = the DISTINCT targets of the group the row hit"""
    offsets, go = np.asarray(offsets, I64), np.asarray(group_offsets, I64)
    target, shared = np.asarray(target, I64), np.asarray(shared, U64)
    nq = len(offsets) - 1
    row = np.repeat(np.arange(nq, dtype=I64), np.diff(offsets))
    grp = np.searchsorted(go, target, side="right") - 1  # the last g with go[g] <= t: empty groups are passed over
    assert ((target >= 0) & (target < go[-1])).all()
    order = np.lexsort((target, grp, row))
    row, grp, target, shared = row[order], grp[order], target[order], shared[order]
    head = np.ones(len(row), bool)
    head[1:] = (row[1:] != row[:-1]) | (grp[1:] != grp[:-1])
    at = np.flatnonzero(head)
    total = np.add.reduceat(shared, at) if len(at) else np.zeros(0, U64)
    newt = np.ones(len(row), bool)
    newt[1:] = head[1:] | (target[1:] != target[:-1])
    members = np.add.reduceat(newt.astype(I64), at) if len(at) else np.zeros(0, I64)
    g, r = grp[head], row[head]
    size = go[g + 1] - go[g]
    keep = members >= max(min_members, 1)
    if frac is not None and frac[1] != 0:
        keep &= members * int(frac[1]) >= int(frac[0]) * size
    out_off = np.concatenate([[0], np.cumsum(np.bincount(r[keep], minlength=nq))]).astype(U64)
    return out_off, g[keep].astype(U32), np.minimum(total[keep], U64(SAT)).astype(U32), members[keep].astype(U32)


def top1_model(offsets, target, shared):
    """bsk_hits_top(1) -> (offsets, target, shared): per row the hit of the largest shared count, ties to the smaller target"""
    offsets = np.asarray(offsets, I64)
    ot, os_, cnt = [], [], []
    for q in range(len(offsets) - 1):
        a, b = int(offsets[q]), int(offsets[q + 1])
        cnt.append(1 if b > a else 0)
        if b > a:
            s = np.asarray(shared[a:b], I64)
            j = a + int(np.flatnonzero(s == s.max())[0])  # targets ascend: the first is the smallest
            ot.append(int(target[j]))
            os_.append(int(shared[j]))
    return np.concatenate([[0], np.cumsum(cnt)]).astype(U64), np.array(ot, U32), np.array(os_, U32)


# ---- the second formulation: per tuple and per hit, in plain Python.  `wrong` switches in ONE wrong reading of the contract ----
WINDOW_MISREADINGS = ("strand_bit", "first_at_w", "nwin_from_p_over_s", "last_window_dropped", "count_floor")
FOLD_MISREADINGS = ("no_saturation", "hits_not_targets", "fraction_rounded")


def windows_brute(offsets, hash_, pos, window=0, step=0, count=0, scale=1, wrong=None):
    maxhash = 0xFFFFFFFFFFFFFFFF // scale if scale > 1 else 0xFFFFFFFFFFFFFFFF
    seq_off, sets = [0], []
    for i in range(len(offsets) - 1):
        a, b = int(offsets[i]), int(offsets[i + 1])
        if pos is None:
            ps = list(range(b - a))
        else:
            ps = [int(x) if wrong == "strand_bit" else int(x) & POS_MASK for x in pos[a:b]]
        nwin = 0
        if b > a:
            P = ps[-1]
            if count:
                W = max(1, (P + 1) // count) if wrong == "count_floor" else max(1, -(-(P + 1) // count))
                S = W
            else:
                W, S = window, (step if step else window)
            first = 0 if (P <= W if wrong == "first_at_w" else P < W) else (P - W) // S + 1
            nwin = first + 1
            if wrong == "nwin_from_p_over_s":
                nwin = P // S + 1
            if wrong == "last_window_dropped":
                nwin -= 1
        if nwin > 100000:  # (a misreading that leaves the strand bit in: no need to build 2^31 windows to see that it differs)
            return (np.array([nwin], U64),) * 4
        wins = [dict() for _ in range(nwin)]
        for j, p in enumerate(ps):
            h = int(hash_[a + j])
            if h > maxhash:
                continue
            for w in range(nwin):
                if w * S <= p < w * S + W:
                    wins[w][h] = wins[w].get(h, 0) + 1
        sets.extend(wins)
        seq_off.append(seq_off[-1] + nwin)
    set_off, values, counts = [0], [], []
    for d in sets:
        for v in sorted(d):
            values.append(v)
            counts.append(d[v])
        set_off.append(len(values))
    return np.array(seq_off, U64), np.array(set_off, U64), np.array(values, U64), np.array(counts, U32)


def fold_brute(offsets, target, shared, group_offsets, min_members=1, frac=None, wrong=None):
    go = [int(x) for x in group_offsets]
    out_off, ot, os_, om = [0], [], [], []
    for q in range(len(offsets) - 1):
        acc = {}
        for i in range(int(offsets[q]), int(offsets[q + 1])):
            t = int(target[i])
            g = max(k for k in range(len(go) - 1) if go[k] <= t < go[k + 1])
            s, ts, nh = acc.get(g, (0, set(), 0))
            acc[g] = (s + int(shared[i]), ts | {t}, nh + 1)
        for g in sorted(acc):
            s, ts, nh = acc[g]
            m, size = (nh if wrong == "hits_not_targets" else len(ts)), go[g + 1] - go[g]
            ok = m >= max(min_members, 1)
            if frac is not None and frac[1] != 0:
                ok = ok and (m >= (frac[0] * size) // frac[1] if wrong == "fraction_rounded" else m * frac[1] >= frac[0] * size)
            if ok:
                ot.append(g)
                os_.append(s & SAT if wrong == "no_saturation" else min(s, SAT))
                om.append(m)
        out_off.append(len(ot))
    return np.array(out_off, U64), np.array(ot, U32), np.array(os_, U32), np.array(om, U32)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x, U64), np.asarray(y, U64)) for x, y in zip(a, b))
