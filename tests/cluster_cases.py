"""Graphs, models and helpers for the clusters of a hits graph (bsk_hits_cluster): shared by tests/test_cluster_cases.py (CPU) and
tests/test_gpu_cluster.py.

A graph is (n, pairs): the nodes 0 .. n - 1 and a list of DIRECTED hits (i, j) as a bsk_hits holds them; the contract reads every hit
with j != i as an undirected edge and ignores the diagonal and repeated directions.  csr() puts a graph into the CSR arrays of a hits
object.  Three models: union-find (components), the sequential loop (greedy) and the two round schemes as the library runs them, which
return the result AND the round count."""
import numpy as np

U64, U32 = np.uint64, np.uint32
SIZES = (1, 2, 63, 64, 65, 257)
METHODS = ("components", "greedy")


# ---- graphs ----
def csr(n, pairs):
    """(n, directed pairs) -> (offsets u64[n + 1], target u32[], shared u32[]): rows ascending, a repeated pair once"""
    rows = [[] for _ in range(n)]
    for i, j in set((int(i), int(j)) for i, j in pairs):
        rows[i].append(j)
    offsets = np.zeros(n + 1, U64)
    target = []
    for i, r in enumerate(rows):
        target += sorted(r)
        offsets[i + 1] = len(target)
    return offsets, np.array(target, U32), np.ones(len(target), U32)


def forms(edges):
    """undirected edges [(u, v)] -> {'full': both directions, 'upper': (min, max) only, 'mixed': one direction or both, by turns}"""
    edges = [(int(u), int(v)) for u, v in edges]
    full = [(u, v) for u, v in edges] + [(v, u) for u, v in edges]
    upper = [(min(u, v), max(u, v)) for u, v in edges]
    mixed = []
    for k, (u, v) in enumerate(edges):
        lo, hi = min(u, v), max(u, v)
        mixed += [[(hi, lo)], [(lo, hi)], [(lo, hi), (hi, lo)]][k % 3]
    return dict(full=full, upper=upper, mixed=mixed)


def path(n, seed=None):
    """a path through all n nodes: in index order, or through a seeded shuffle of them"""
    p = np.arange(n) if seed is None else np.random.default_rng(seed).permutation(n)
    return [(int(p[k]), int(p[k + 1])) for k in range(n - 1)]


def gnp(n, p, seed):
    rng = np.random.default_rng(seed)
    return [(u, v) for u in range(n) for v in range(u + 1, n) if rng.random() < p]


def generators():
    """[(name, n, undirected edges, diagonal hits)]: every shape of the issue, over the sizes where a size applies"""
    out = []
    for n in SIZES:
        out.append((f"no_edges_{n}", n, [], []))
        out.append((f"diagonal_only_{n}", n, [], [(v, v) for v in range(n)]))
        if n >= 2:
            out.append((f"one_edge_{n}", n, [(n - 1, 0)], []))
            out.append((f"path_identity_{n}", n, path(n), []))
            out.append((f"path_shuffled_{n}", n, path(n, seed=n), []))
            out.append((f"star_best_hub_{n}", n, [(0, v) for v in range(1, n)], []))
            out.append((f"star_worst_hub_{n}", n, [(n - 1, v) for v in range(n - 1)], []))
        if n >= 3:
            out.append((f"ring_{n}", n, path(n) + [(n - 1, 0)], []))
            out.append((f"isolated_among_edges_{n}", n, [(u, u + 2) for u in range(0, n - 2, 5)], [(1, 1)]))
            out.append((f"gnp_{n}", n, gnp(n, min(0.5, 1.5 / n), seed=100 + n), [(v, v) for v in range(0, n, 7)]))
    out.append(("k17", 17, [(u, v) for u in range(17) for v in range(u + 1, 17)], []))
    k8 = [(u, v) for u in range(8) for v in range(u + 1, 8)]
    out.append(("two_k8_bridge", 16, k8 + [(u + 8, v + 8) for u, v in k8] + [(7, 8)], []))
    out.append(("gnp_dense_65", 65, gnp(65, 0.2, seed=7), []))
    return out


def cases():
    """[(name, n, directed pairs)]: every generator as full CSR, as upper triangle and with the directions mixed"""
    out = []
    for name, n, edges, diag in generators():
        for form, pairs in forms(edges).items():
            out.append((f"{name}-{form}", n, pairs + diag))
    return out


def random_multigraph(seed):
    """a seeded multigraph with self-loops and repeated edges in both directions -> (n, directed pairs)"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 40))
    m = int(rng.integers(0, 3 * n))
    return n, [(int(rng.integers(n)), int(rng.integers(n))) for _ in range(m)]


def scores(n, seed=0):
    """{name: None or u64[n]}: the priorities every case runs under"""
    rng = np.random.default_rng(1000 + seed)
    top = np.iinfo(U64).max
    return dict(none=None, equal=np.full(n, 5, U64), random=rng.integers(0, 1 << 63, n, dtype=U64) * U64(2) + rng.integers(0, 2, n, dtype=U64),
                descending=np.arange(n, dtype=U64)[::-1].copy(), ascending=np.arange(n, dtype=U64), extremes=np.where(rng.integers(0, 2, n) == 1, top, 0).astype(U64),
                few=rng.integers(0, 3, n, dtype=U64))


# ---- the contract, restated ----
def edge_list(offsets, target, directed=False):
    """CSR -> the sorted undirected edges {(u, v), u < v}: the diagonal dropped, both directions folded (directed: kept as they stand)"""
    out = set()
    for i in range(len(offsets) - 1):
        for p in range(int(offsets[i]), int(offsets[i + 1])):
            j = int(target[p])
            if j != i:
                out.add((i, j) if directed else (min(i, j), max(i, j)))
    return sorted(out)


def n_offdiagonal(offsets, target):
    """the hits with j != i, each direction counted: the edges= figure of the plan"""
    return sum(1 for i in range(len(offsets) - 1) for p in range(int(offsets[i]), int(offsets[i + 1])) if int(target[p]) != i)


def ranking(n, score):
    """-> (order, rank): higher score first, ties to the smaller index; None: index order"""
    order = list(range(n)) if score is None else sorted(range(n), key=lambda v: (-int(score[v]), v))
    rank = [0] * n
    for r, v in enumerate(order):
        rank[v] = r
    return order, rank


def layout(rep_of):
    """the representative of every node -> (label u32[n], rep u32[c], offsets u64[c + 1], members u32[n], largest)"""
    n = len(rep_of)
    reps = sorted(set(rep_of))
    num = {v: c for c, v in enumerate(reps)}
    label = np.array([num[r] for r in rep_of], U32)
    groups = [[] for _ in reps]
    for v in range(n):
        groups[num[rep_of[v]]].append(v)
    offsets = np.zeros(len(reps) + 1, U64)
    offsets[1:] = np.cumsum([len(g) for g in groups], dtype=U64) if reps else []
    members = np.array([v for g in groups for v in g], U32)
    return label, np.array(reps, U32), offsets, members, max([len(g) for g in groups], default=0)


def model_components(n, offsets, target, score=None):
    """union-find, then the member of best rank represents its component"""
    _, rank = ranking(n, score)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u, v in edge_list(offsets, target):
        parent[find(u)] = find(v)
    best = {}
    for v in range(n):
        r = find(v)
        if r not in best or rank[v] < rank[best[r]]:
            best[r] = v
    return layout([best[find(v)] for v in range(n)])


def model_greedy(n, offsets, target, score=None):
    """the sequential definition: by ascending rank, join the best-ranked neighbour that is already a representative, else become one"""
    order, rank = ranking(n, score)
    nbr = [[] for _ in range(n)]
    for u, v in edge_list(offsets, target):
        nbr[u].append(v)
        nbr[v].append(u)
    is_rep, rep_of = [False] * n, [0] * n
    for v in order:
        cands = [u for u in nbr[v] if is_rep[u]]
        if cands:
            rep_of[v] = min(cands, key=lambda u: rank[u])
        else:
            is_rep[v], rep_of[v] = True, v
    return layout(rep_of)


# ---- the round schemes as built (rank space, snapshot reads, min-combined writes) ----
def _rank_edges(n, offsets, target, rank):
    e = edge_list(offsets, target)
    if not e:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    a = np.array([[rank[u], rank[v]] for u, v in e], np.int64)
    return a.min(axis=1), a.max(axis=1)


def rounds_components(n, offsets, target, score=None):
    """k_cl_hook + k_cl_jump -> (layout, rounds); the last, unchanged round is counted"""
    if n == 0:
        return layout([]), 0
    order, rank = ranking(n, score)
    eu, ev = _rank_edges(n, offsets, target, rank)
    f = np.arange(n, dtype=np.int64)
    rounds = 0
    while True:
        assert rounds <= n, "the cap of n + 1 rounds"
        fn = f.copy()
        fu, fv = f[eu], f[ev]
        lo = fu < fv
        np.minimum.at(fn, fv[lo], fu[lo])
        np.minimum.at(fn, ev[lo], fu[lo])
        hi = fv < fu
        np.minimum.at(fn, fu[hi], fv[hi])
        np.minimum.at(fn, eu[hi], fv[hi])
        fn = np.minimum(fn, f[f])
        rounds += 1
        changed = bool((fn != f).any())
        f = fn
        if not changed:
            break
    return layout([order[int(f[rank[v]])] for v in range(n)]), rounds


def rounds_greedy(n, offsets, target, score=None):
    """k_cl_mis_scan + k_cl_mis_apply + k_cl_assign -> (layout, rounds); rounds = the last round that decided a node"""
    if n == 0:
        return layout([]), 0
    order, rank = ranking(n, score)
    eu, ev = _rank_edges(n, offsets, target, rank)  # eu before ev
    UND, REP, OUT = 0, 1, 2
    state = np.zeros(n, np.int64)
    out = np.zeros(n, bool)
    rounds = 0
    while (state == UND).any():
        assert rounds <= n, "the cap of n + 1 rounds"
        rounds += 1
        live = state[ev] == UND
        out[ev[live & (state[eu] == REP)]] = True
        blocked = np.zeros(n, bool)
        blocked[ev[live & (state[eu] == UND)]] = True
        und = state == UND
        state[und & out] = OUT
        state[und & ~out & ~blocked] = REP
    best = np.full(n, n, np.int64)
    a = (state[eu] == REP) & (state[ev] == OUT)
    np.minimum.at(best, ev[a], eu[a])
    b = (state[ev] == REP) & (state[eu] == OUT)
    np.minimum.at(best, eu[b], ev[b])
    root = np.where(state == REP, np.arange(n), best)
    return layout([order[int(root[rank[v]])] for v in range(n)]), rounds


MODELS = dict(components=model_components, greedy=model_greedy)
ROUND_MODELS = dict(components=rounds_components, greedy=rounds_greedy)


def same(x, y):
    """exact equality of two (label, rep, offsets, members, largest) tuples, dtypes aside"""
    return all(np.array_equal(np.asarray(p).astype(U64), np.asarray(q).astype(U64)) for p, q in zip(x[:4], y[:4])) and int(x[4]) == int(y[4])


# ---- a graph encoded as sets ----
def as_sets(n, pairs):
    """set v = {a private value} | {the ids of v's edges}: two sets share a value iff an edge joins them, so
    bsk_sets_neighbors(min_shared=1) lists exactly the graph's edges, both directions, and the diagonal -> (offsets u64[n + 1], values u64[])"""
    und = sorted(set((min(i, j), max(i, j)) for i, j in pairs if i != j))
    sets = [[v] for v in range(n)]  # private values 0 .. n - 1, edge ids from n
    for k, (u, v) in enumerate(und):
        sets[u].append(n + k)
        sets[v].append(n + k)
    offsets = np.zeros(n + 1, U64)
    offsets[1:] = np.cumsum([len(s) for s in sets], dtype=U64) if n else []
    return offsets, np.array([x for s in sets for x in sorted(s)], U64)
