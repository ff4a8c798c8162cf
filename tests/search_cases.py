"""The containment search's host-side restatement and its crafted cases (include/biosketch.h "containment search", search.hip).

ref_search is the header's rule in NumPy.  mix64 / unmix64 / directory restate the index's keys and directory, so a test can pick a
key -- and with it a bucket -- and turn it back into a value.  Every builder returns its collections with what it claims about them
(posting sums, which queries take the large path, bucket occupancy); tests/test_search_cases.py re-derives each claim from the sets
alone, and tests/test_gpu_search_edges.py asserts that the device reached it before it compares the hits."""
import numpy as np

U64 = np.uint64
SR_CAP = 2048  # search.hip: the target ids one wavefront sorts in LDS; a query whose posting sum exceeds it takes the large path
_C1, _C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_I1, _I2 = pow(_C1, -1, 1 << 64), pow(_C2, -1, 1 << 64)


# ---- the reference ----
def collection(sets):
    """list of value arrays -> (offsets, values), every set sorted and distinct"""
    sets = [np.unique(np.asarray(s, U64)) for s in sets]
    offs = np.zeros(len(sets) + 1, U64)
    offs[1:] = np.cumsum([len(s) for s in sets])
    vals = np.concatenate(sets) if sets and offs[-1] else np.zeros(0, U64)
    return offs, vals.astype(U64)


def ref_counts(t_offs, t_vals, q_offs, q_vals):
    """-> (query, target, shared) of every pair that shares a value, ascending by (query, target)"""
    nt, nq = len(t_offs) - 1, len(q_offs) - 1
    tsz, qsz = np.diff(t_offs).astype(np.int64), np.diff(q_offs).astype(np.int64)
    tid = np.repeat(np.arange(nt, dtype=U64), tsz)
    order = np.argsort(t_vals, kind="stable")
    sv, st = t_vals[order], tid[order]
    qid = np.repeat(np.arange(nq, dtype=U64), qsz)
    lo = np.searchsorted(sv, q_vals, "left")
    cnt = np.searchsorted(sv, q_vals, "right") - lo
    tot = int(cnt.sum())
    starts = np.repeat(lo - (np.cumsum(cnt) - cnt), cnt) + np.arange(tot)
    key = (np.repeat(qid, cnt) << U64(32)) | st[starts]
    uk, c = np.unique(key, return_counts=True)
    return (uk >> U64(32)).astype(np.int64), (uk & U64(0xFFFFFFFF)).astype(np.int64), c.astype(np.int64)


def ref_select(counts, t_offs, q_offs, min_shared=1, qc=0.0, tc=0.0):
    """the header's threshold, term for term in float64 -> (offsets, target, shared)"""
    q, t, c = counts
    tsz, qsz = np.diff(t_offs).astype(np.int64), np.diff(q_offs).astype(np.int64)
    nq = len(q_offs) - 1
    keep = (c >= max(min_shared, 1)) & (c.astype(np.float64) >= qc * qsz[q].astype(np.float64)) & \
        (c.astype(np.float64) >= tc * tsz[t].astype(np.float64))
    q, t, c = q[keep], t[keep], c[keep]
    offs = np.zeros(nq + 1, U64)
    offs[1:] = np.cumsum(np.bincount(q, minlength=nq))
    return offs, t.astype(np.uint32), c.astype(np.uint32)


def ref_search(t_offs, t_vals, q_offs, q_vals, min_shared=1, qc=0.0, tc=0.0):
    """-> (offsets, target, shared) by the contract, computed on the host"""
    return ref_select(ref_counts(t_offs, t_vals, q_offs, q_vals), t_offs, q_offs, min_shared, qc, tc)


def ref_top(o, t, s, n):
    """np.lexsort((target, -shared)) inside every query (the query as the outermost key does all of them at once), cut at n"""
    nq = len(o) - 1
    cnt = np.diff(o).astype(np.int64)
    q = np.repeat(np.arange(nq, dtype=np.int64), cnt)
    order = np.lexsort((t, -s.astype(np.int64), q))
    rank = np.arange(len(t), dtype=np.int64) - np.repeat(o[:-1].astype(np.int64), cnt)
    idx = order[rank < n]
    no = np.zeros(nq + 1, U64)
    no[1:] = np.cumsum(np.minimum(cnt, n))
    return no, t[idx], s[idx]


def posting_sums(t_offs, t_vals, q_offs, q_vals):
    """every query's sum of posting counts: how many targets hold each of its values, added up"""
    sv = np.sort(t_vals)
    cnt = np.searchsorted(sv, q_vals, "right") - np.searchsorted(sv, q_vals, "left")
    c = np.zeros(len(q_vals) + 1, np.int64)
    c[1:] = np.cumsum(cnt)
    o = q_offs.astype(np.int64)
    return c[o[1:]] - c[o[:-1]]


# ---- the index's key and directory ----
def mix64(x):
    """splitmix64's finalizer, as search.hip keys every value"""
    x = np.array(x, U64)
    with np.errstate(over="ignore"):
        x ^= x >> U64(30)
        x *= U64(_C1)
        x ^= x >> U64(27)
        x *= U64(_C2)
        x ^= x >> U64(31)
    return x


def _unxorshift(y, s):
    x = y.copy()
    for _ in range(64 // s):  # each round fixes s more of the top bits
        x = y ^ (x >> U64(s))
    return x


def unmix64(k):
    """the value whose key is k: each xor-shift undone, each odd multiplier's inverse mod 2^64"""
    x = np.array(k, U64)
    with np.errstate(over="ignore"):
        x = _unxorshift(x, 31)
        x *= U64(_I2)
        x = _unxorshift(x, 27)
        x *= U64(_I1)
        x = _unxorshift(x, 30)
    return x


def dir_bits(u):
    """bsk_index_build's directory width: 2^bits <= U < 2^(bits + 1) (0 for U <= 1)"""
    bits = 0
    while bits < 62 and (2 << bits) <= u:
        bits += 1
    return bits


def bucket(keys, bits):
    keys = np.asarray(keys, U64)
    return (keys >> U64(64 - bits)).astype(np.int64) if bits else np.zeros(keys.shape, np.int64)


def directory(values):
    """the directory bsk_index_build makes of these target values -> dict(n_distinct, bits, keys ascending, counts of every
    bucket, max_bucket)"""
    keys = np.unique(mix64(np.unique(np.asarray(values, U64))))
    u = len(keys)
    bits = dir_bits(u)
    counts = np.bincount(bucket(keys, bits), minlength=1 << bits)
    return dict(n_distinct=u, bits=bits, keys=keys, counts=counts, max_bucket=int(counts.max()) if u else 0)


# ---- builders ----
class Builder:
    """Targets and queries made value by value.  value(c) is a new value that exactly c targets hold, so a query's posting sum is
    the sum of its values' counts; values are handed out ascending, so a query's values sit in the order they were made."""

    def __init__(self, n_targets, seed, lead_empty=0, trail_empty=0):
        self.T = n_targets
        self.rng = np.random.default_rng(seed)
        self.tv, self.tt = [], []      # postings: value, target
        self.queries, self.sums = [], []
        self.count = {}
        self.next = 1 << 40
        self.first = lead_empty        # targets lead_empty .. T - trail_empty - 1 hold values
        self.span = n_targets - lead_empty - trail_empty

    def value(self, c):
        v = self.next
        self.next += 3  # (gaps: misses between held values)
        if c:
            t = self.first + self.rng.choice(self.span, c, replace=False)
            self.tv.append(np.full(c, v, U64))
            self.tt.append(t.astype(np.int64))
        self.count[v] = c
        return v

    def query(self, vals):
        self.queries.append(np.asarray(vals, U64))
        self.sums.append(sum(self.count[int(v)] for v in vals))

    def query_counts(self, counts):
        """a query whose value i is held by counts[i] targets"""
        self.query([self.value(c) for c in counts])

    def split(self, n, parts):
        """counts of `parts` values that add up to n"""
        cut = np.sort(self.rng.choice(np.arange(1, n), parts - 1, replace=False)) if parts > 1 else np.zeros(0, np.int64)
        return list(np.diff(np.concatenate([[0], cut, [n]])).astype(int))

    def build(self):
        tv = np.concatenate(self.tv) if self.tv else np.zeros(0, U64)
        tt = np.concatenate(self.tt) if self.tt else np.zeros(0, np.int64)
        order = np.lexsort((tv, tt))
        tg_offs = np.zeros(self.T + 1, U64)
        tg_offs[1:] = np.cumsum(np.bincount(tt, minlength=self.T))
        sums = np.array(self.sums, np.int64)
        return (tg_offs, tv[order]), collection(self.queries), claims(sums)


def claims(sums):
    sums = np.asarray(sums, np.int64)
    return dict(sums=sums, large=sums > SR_CAP, n_large=int((sums > SR_CAP).sum()))


SUM_EDGES = (1, 63, 64, 65, 2047, 2048, 2049, 5000)


def posting_edge_case(seed=41):
    """queries of posting sum 1, 63, 64, 65, 2047, 2048, 2049 and 5 000, each made several ways (one value in n targets, n values
    in one target each, mixes, with misses); then 4 runs of 8..40 consecutive sums of exactly 2048 between runs of tiny queries"""
    b = Builder(6000, seed, lead_empty=3, trail_empty=4)
    for n in SUM_EDGES:
        b.query_counts([n])
        b.query_counts([1] * n)
        b.query_counts([0] + b.split(n, min(n, 2)) + [0])
        b.query_counts(b.split(n, min(n, 7)))
        if n > 64:
            b.query_counts(b.split(n - 40, 3) + [1] * 40)
    for run in (8, 40, 32, 9):
        for _ in range(run):
            b.query_counts(b.split(SR_CAP, int(b.rng.integers(1, 40))))
        for _ in range(int(b.rng.integers(1, 6))):
            b.query_counts(list(b.rng.integers(0, 3, int(b.rng.integers(0, 4)))))
    return b.build()


def clamp_case(n_targets, seed=43):
    """T = 1, 2 or 3 targets and posting sums far above T on both paths: a query lists at most T hits, whatever its sum"""
    b = Builder(n_targets, seed)
    for m in (1, 7, 300, 2048 // n_targets, 2048 // n_targets + 1, 3000):
        b.query_counts([n_targets] * m)
        b.query_counts([int(c) for c in b.rng.integers(0, n_targets + 1, m)])
    return b.build()


LIST_LENGTHS = (63, 64, 65, 128, 129)
LIST_PLACES = (0, 63, 64, 100, 129)


def list_length_case(seed=47):
    """large queries, each with one posting list of 63, 64, 65, 128 or 129 target ids at value index 0, 63 (the last lane of the
    first 64-value chunk) or >= 64 among lists of at most 40; then queries with long lists at several lanes of one chunk"""
    b = Builder(3000, seed)
    for n in LIST_LENGTHS:
        for at in LIST_PLACES:
            c = [int(x) for x in b.rng.integers(0, 41, 140)]
            c[at] = n
            b.query_counts(c)
    for long_at in ((0, 63), (1, 2, 62), (64, 127), (0, 63, 64, 127, 139)):
        c = [int(x) for x in b.rng.integers(0, 41, 140)]
        for at in long_at:
            c[at] = int(b.rng.integers(65, 400))
        b.query_counts(c)
    b.query_counts([int(x) for x in b.rng.integers(0, 41, 140)])  # and a small one (or not) beside them
    return b.build()


def nl_case(n_large, last_only=False, seed=53):
    """n_large large queries among small ones: the first query, the last, and the rest interleaved (last_only: one, last).  Query 1
    (large when n_large > 2) holds only the value H, which every one of 2 100 targets holds: it shares one value with each, so
    min_shared = 2 rejects every pair of it; the other large queries hold H and values of the pool, so they keep some."""
    b = Builder(2600, seed + n_large)
    h = b.value(2100)
    pool = [b.value(int(c)) for c in b.rng.integers(1, 60, 300)]
    n_small = 2 * n_large + 5
    is_large = np.zeros(n_large + n_small, bool)
    if last_only:
        is_large[-1] = True
    else:
        is_large[0] = True
        is_large[-1] = n_large > 1
        rest = n_large - 1 - (n_large > 1)
        if rest:
            is_large[1] = True
            rest -= 1
        is_large[2 + b.rng.choice(len(is_large) - 3, rest, replace=False)] = True
    for i, big in enumerate(is_large):
        vals = [pool[j] for j in b.rng.choice(len(pool), int(b.rng.integers(3 if big else 0, 25)), replace=False)]
        if big and i == 1:
            vals = []
        b.query(sorted(vals + [h]) if big else sorted(vals))
    return b.build()


def edge_large_case():
    """test_gpu_search.edge_collection's query (j, size, s) -- s values of target j and misses -- with one value that 2 049 extra
    targets hold in place of one miss: |q| and the pairs' shared counts stay the edge set's, and every query's posting sum exceeds
    SR_CAP.  Extra target i holds that value and i % 7 values of its own."""
    X = 5 * 10**9
    tsets = [np.arange(100, dtype=U64) + U64(1000 * j) for j in range(8)]
    tsets += [np.concatenate([[X], np.arange(i % 7, dtype=U64) + U64(6 * 10**9 + 10 * i)]) for i in range(2049)]
    qsets, sums = [], []
    j = 0
    for size in (10, 30, 60, 90, 100):
        for s in range(0, size):
            qsets.append(np.concatenate([np.arange(s, dtype=U64) + U64(1000 * j), np.arange(size - 1 - s, dtype=U64) + U64(10**9 + 1000 * j),
                                         [X]]))
            sums.append(s + 2049)
            j = (j + 1) % 8
    return collection(tsets), collection(qsets), claims(sums)


def boundary_case(n_large, n_small, seed=59):
    """posting sums that straddle SR_CAP: 24 values H_k held by 2 036 + k targets each, 3 000 values held by 1-3 targets; a query
    is one H_k and 0-4 of the others, so its sum lies in 2 036 .. 2 071.  The first n_large large and n_small small candidates are
    kept and shuffled together."""
    rng = np.random.default_rng(seed)
    T, K, J = 4200, 24, 3000
    hc = 2036 + np.arange(K)
    ec = rng.integers(1, 4, J)
    cnt = np.concatenate([hc, ec])
    tt = np.concatenate([rng.choice(T, int(c), replace=False) for c in cnt])
    vid = np.repeat(np.arange(K + J), cnt)
    val = (U64(1) << U64(50)) + (mix64(np.arange(K + J, dtype=U64)) >> U64(20))  # distinct, unordered
    assert len(np.unique(val)) == K + J
    order = np.lexsort((val[vid], tt))
    tg_offs = np.zeros(T + 1, U64)
    tg_offs[1:] = np.cumsum(np.bincount(tt, minlength=T))
    tg = (tg_offs, val[vid][order])
    m = 3 * (n_large + n_small)
    nx = rng.integers(0, 5, m)
    hk = rng.integers(0, K, m)
    ex = K + rng.integers(0, J, (m, 4))
    ex_ok = np.arange(4)[None, :] < nx[:, None]
    dup = np.zeros(m, bool)  # drop candidates that draw one extra value twice
    for a in range(4):
        for c in range(a + 1, 4):
            dup |= ex_ok[:, a] & ex_ok[:, c] & (ex[:, a] == ex[:, c])
    sums = hc[hk] + np.where(ex_ok, cnt[ex], 0).sum(1)
    large = sums > SR_CAP
    big = np.flatnonzero(large & ~dup)[:n_large]
    small = np.flatnonzero(~large & ~dup)[:n_small]
    assert len(big) == n_large and len(small) == n_small
    keep = np.concatenate([big, small])
    rng.shuffle(keep)
    ids = np.concatenate([hk[keep, None], np.where(ex_ok[keep], ex[keep], -1)], 1)
    qv = np.where(ids >= 0, val[np.maximum(ids, 0)], U64(2**64 - 1))
    qv.sort(1)
    n = 1 + nx[keep]
    q_offs = np.zeros(len(keep) + 1, U64)
    q_offs[1:] = np.cumsum(n)
    q_vals = qv[np.arange(5)[None, :] < n[:, None]]  # (row-major: each query's n smallest, its own values)
    return tg, (q_offs, q_vals), claims(sums[keep])


def s2_case(n_sets=2000, size=10_000, pool=1_000_000, seed=61):
    """scripts/perf_search.py's S2: n_sets sets of `size` draws from a pool of `pool` random values (drawn with replacement, so
    slightly fewer distinct)"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 2**64, pool, dtype=U64)
    return collection([p[rng.integers(0, pool, size)] for _ in range(n_sets)])


def s2_matrix(offs, vals):
    """all-vs-all shared counts M[a, b] = |set a & set b|: postings grouped by value, every pair of holders counted"""
    n = len(offs) - 1
    sid = np.repeat(np.arange(n, dtype=np.int64), np.diff(offs).astype(np.int64))
    order = np.argsort(vals, kind="stable")
    v, s = vals[order], sid[order]
    starts = np.flatnonzero(np.concatenate([[True], v[1:] != v[:-1]]))
    lens = np.diff(np.concatenate([starts, [len(v)]]))
    m = np.zeros(n * n, np.int64)
    for c in np.unique(lens):
        g = starts[lens == c]
        hold = s[g[:, None] + np.arange(c)[None, :]]
        step = max(1, (1 << 24) // int(c * c))
        for a in range(0, len(g), step):
            h = hold[a:a + step]
            m += np.bincount((h[:, :, None] * n + h[:, None, :]).ravel(), minlength=n * n)
    return m.reshape(n, n)


# ---- directory layouts ----
def keys_in_bucket(rng, bucket_id, bits, n):
    """n distinct keys whose top `bits` bits are bucket_id"""
    lo = U64(bucket_id) << U64(64 - bits)
    k = np.unique(rng.integers(0, 1 << (64 - bits), 3 * n + 8, dtype=U64))[:n]
    rng.shuffle(k)
    return lo | k


def layout(name, seed=67):
    """target values of a directory layout -> (values, what it claims: dict of n_distinct and more)"""
    rng = np.random.default_rng(seed)
    if name.startswith("u="):
        u = int(name[2:])
        vals = np.unique(rng.integers(0, 2**64, u + 64, dtype=U64))[:u]
        return vals, dict(n_distinct=u)
    if name == "extreme keys":  # value 0 has key 0 (bucket 0); unmix64(2^64 - 1) has the last key of the last bucket
        vals = np.concatenate([np.array([0, int(unmix64(2**64 - 1))], U64), rng.integers(1, 2**64 - 1, 998, dtype=U64)])
        return vals, dict(n_distinct=1000, keys={0, 2**64 - 1})
    if name == "first and last bucket":  # 1 024 keys (bits = 10): 511 in bucket 0, 513 in bucket 1 023, none between
        keys = np.concatenate([keys_in_bucket(rng, 0, 10, 510), np.array([0], U64), keys_in_bucket(rng, 1023, 10, 512), np.array([2**64 - 1], U64)])
        return unmix64(keys), dict(n_distinct=1024, bits=10, occupied={0: 511, 1023: 513})
    if name == "long bucket":  # 4 096 ordinary keys and 600 more in bucket 1 234 of 4 096 (bits = 12)
        keys = np.concatenate([rng.integers(0, 2**64, 4096, dtype=U64), keys_in_bucket(rng, 1234, 12, 600)])
        return unmix64(keys), dict(n_distinct=4696, bits=12, min_bucket_at={1234: 600})
    raise KeyError(name)


LAYOUTS = ("u=1", "u=2", "u=3", "u=1023", "u=1024", "u=1025", "u=131071", "u=131072", "u=131073", "extreme keys",
           "first and last bucket", "long bucket")


def probe_keys(d):
    """keys that a lookup must get right in directory d: the first, a middle and the last key of the fullest bucket; a key just
    below, one between two of its keys and one just above; the first and last key of the first and last non-empty bucket, and a
    key in every empty bucket next to a full one"""
    keys, bits, counts = d["keys"], d["bits"], d["counts"]
    if not len(keys):
        return np.array([0, 2**64 - 1], U64)
    kb = bucket(keys, bits)
    j = int(np.argmax(counts))
    inb = keys[kb == j]
    out = [inb[0], inb[len(inb) // 2], inb[-1], inb[0] - U64(1) if inb[0] else inb[0], inb[-1] + U64(1) if inb[-1] < U64(2**64 - 1) else inb[-1]]
    gap = np.flatnonzero(np.diff(inb) > U64(1))
    if len(gap):
        out.append(inb[gap[len(gap) // 2]] + U64(1))
    full = np.flatnonzero(counts)
    out += [keys[0], keys[-1], keys[kb == full[0]][-1], keys[kb == full[-1]][0]]
    empty = np.flatnonzero(counts == 0)
    nextto = empty[np.isin(empty - 1, full) | np.isin(empty + 1, full)]
    for e in nextto[:64]:
        out += [U64(int(e) << (64 - bits)), U64(((int(e) + 1) << (64 - bits)) - 1)]
    return np.array(out, U64)
