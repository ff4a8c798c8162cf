"""CPU: the models of tests/cluster_cases.py against each other -- the round schemes the library runs (hook + jump, scan + apply)
equal union-find and the sequential greedy rule on every generator and on 200 seeded multigraphs, take the rounds the header
promises, and wrong readings of the contract are caught by the cases."""
import numpy as np
import pytest

from tests import cluster_cases as CL

CASES = CL.cases()


def _all_graphs():
    for name, n, pairs in CASES:
        yield name, n, pairs
    for seed in range(200):
        n, pairs = CL.random_multigraph(seed)
        yield f"multigraph_{seed}", n, pairs


def test_the_generators_cover_the_shapes_and_forms():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names)) and len(names) % 3 == 0
    for shape in ("no_edges", "one_edge", "path_identity", "path_shuffled", "ring", "star_best_hub", "star_worst_hub", "k17", "two_k8_bridge", "diagonal_only",
                  "isolated_among_edges", "gnp"):
        for form in ("full", "upper", "mixed"):
            assert any(nm.startswith(shape) and nm.endswith("-" + form) for nm in names), (shape, form)
    for n in CL.SIZES:
        assert any(c[1] == n for c in CASES)
    # the three forms of one graph are the same graph, stated differently
    for k in range(0, len(CASES), 3):
        e = [CL.edge_list(*CL.csr(n, pairs)[:2]) for _, n, pairs in CASES[k:k + 3]]
        assert e[0] == e[1] == e[2]
    o, t, _ = CL.csr(65, dict(CASES_BY_NAME())["path_identity_65-upper"])
    assert all(int(t[p]) > i for i in range(65) for p in range(int(o[i]), int(o[i + 1])))


def CASES_BY_NAME():
    return [(name, pairs) for name, _, pairs in CASES]


def test_round_models_equal_the_sequential_models():
    checked = 0
    for name, n, pairs in _all_graphs():
        o, t, _ = CL.csr(n, pairs)
        for sname, sc in CL.scores(n, seed=checked).items():
            for m in CL.METHODS:
                want = CL.MODELS[m](n, o, t, sc)
                got, rounds = CL.ROUND_MODELS[m](n, o, t, sc)
                assert CL.same(got, want), (name, sname, m)
                assert 1 <= rounds <= (n if m == "greedy" else n + 1), (name, sname, m, rounds)  # the cap is never reached
                checked += 1
    assert checked >= 2 * 6 * (len(CASES) + 200)


def test_results_have_the_contracts_layout():
    for name, n, pairs in CASES:
        o, t, _ = CL.csr(n, pairs)
        for m in CL.METHODS:
            label, rep, offsets, members, largest = CL.MODELS[m](n, o, t, CL.scores(n)["random"])
            assert list(rep) == sorted(set(rep.tolist())) and len(label) == len(members) == n and int(offsets[-1]) == n
            assert sorted(members.tolist()) == list(range(n)) and largest == int(np.diff(offsets).max())
            for c, r in enumerate(rep):
                mem = members[int(offsets[c]):int(offsets[c + 1])]
                assert list(mem) == sorted(mem.tolist()) and int(r) in mem and all(int(label[v]) == c for v in mem)
            if m == "greedy":  # a member neighbours its representative, and no two representatives are neighbours
                edges = set(CL.edge_list(o, t))
                reps = set(rep.tolist())
                for v in range(n):
                    r = int(rep[label[v]])
                    assert v == r or (min(v, r), max(v, r)) in edges, (name, v)
                assert not any(u in reps and v in reps for u, v in edges), name


def test_rounds_on_paths():
    """components halve the paths: <= 20 rounds on 4 096 nodes; greedy on the path ranked from one end takes n rounds, a handful shuffled"""
    n = 4096
    for seed in (None, 4096):
        o, t, _ = CL.csr(n, CL.forms(CL.path(n, seed))["upper"])
        got, rounds = CL.rounds_components(n, o, t)
        assert rounds <= 20 and len(got[1]) == 1 and got[4] == n, (seed, rounds)
    for n in (63, 257):
        o, t, _ = CL.csr(n, CL.forms(CL.path(n))["full"])
        assert CL.rounds_greedy(n, o, t)[1] == n
        o, t, _ = CL.csr(n, CL.forms(CL.path(n, seed=n))["full"])
        assert CL.rounds_greedy(n, o, t)[1] <= 8


# ---- wrong readings of the contract: each must differ from the model on some case ----
def _caught(wrong, method):
    for name, n, pairs in CASES:
        o, t, _ = CL.csr(n, pairs)
        for sname, sc in CL.scores(n, seed=3).items():
            try:
                if not CL.same(wrong(n, o, t, sc), CL.MODELS[method](n, o, t, sc)):
                    return name, sname
            except AssertionError:
                return name, sname
    return None


def _greedy(n, o, t, sc, pick=None, tie=1, directed=False):
    order = list(range(n)) if sc is None else sorted(range(n), key=lambda v: (-int(sc[v]), tie * v))
    rank = {v: r for r, v in enumerate(order)}
    nbr = [[] for _ in range(n)]
    for u, v in CL.edge_list(o, t, directed=directed):
        nbr[u].append(v)
        if not directed:
            nbr[v].append(u)
    is_rep, rep_of = [False] * n, [0] * n
    for v in order:
        cands = [u for u in nbr[v] if is_rep[u]]
        if cands:
            rep_of[v] = min(cands, key=pick or (lambda u: rank[u]))
        else:
            is_rep[v], rep_of[v] = True, v
    return rep_of, rank


def test_wrong_models_are_caught():
    # a member joins its first representative neighbour by INDEX where rank is meant
    assert _caught(lambda n, o, t, sc: CL.layout(_greedy(n, o, t, sc, pick=lambda u: u)[0]), "greedy")
    # ties go to the LARGER index
    assert _caught(lambda n, o, t, sc: CL.layout(_greedy(n, o, t, sc, tie=-1)[0]), "greedy")

    def comp_ties_larger(n, o, t, sc):
        want = CL.model_components(n, o, t, None)  # the components themselves
        order = list(range(n)) if sc is None else sorted(range(n), key=lambda v: (-int(sc[v]), -v))
        rank = {v: r for r, v in enumerate(order)}
        best = {}
        for v in range(n):
            c = int(want[0][v])
            if c not in best or rank[v] < rank[best[c]]:
                best[c] = v
        return CL.layout([best[int(want[0][v])] for v in range(n)])
    assert _caught(comp_ties_larger, "components")

    # representatives (and so the cluster numbers) ordered by RANK
    def reps_by_rank(n, o, t, sc):
        rep_of, rank = _greedy(n, o, t, sc)
        reps = sorted(set(rep_of), key=lambda v: rank[v])
        num = {v: c for c, v in enumerate(reps)}
        label, _, offsets, members, largest = CL.layout(rep_of)
        return np.array([num[r] for r in rep_of]), np.array(reps), offsets, members, largest
    assert _caught(reps_by_rank, "greedy")

    # the diagonal counted as an edge: a node that neighbours itself waits for itself -- the round scheme never ends (its cap asserts)
    def diagonal_counts(n, o, t, sc):
        edge_list = CL.edge_list
        try:
            CL.edge_list = lambda o_, t_, directed=False: sorted(set(edge_list(o_, t_)) | {(i, i) for i in range(n) for p in range(int(o_[i]), int(o_[i + 1])) if int(t_[p]) == i})
            return CL.rounds_greedy(n, o, t, sc)[0]
        finally:
            CL.edge_list = edge_list
    hit = _caught(diagonal_counts, "greedy")
    assert hit and ("diagonal" in hit[0] or "isolated" in hit[0] or "gnp" in hit[0])
    o, t, _ = CL.csr(3, [(0, 0), (0, 1), (1, 1), (2, 2)])
    assert CL.n_offdiagonal(o, t) == 1 and CL.edge_list(o, t) == [(0, 1)]

    # a directed reading of an upper-triangle graph: row i's hits alone are i's neighbours
    hit = _caught(lambda n, o, t, sc: CL.layout(_greedy(n, o, t, sc, directed=True)[0]), "greedy")
    assert hit and not hit[0].endswith("-full")


def test_the_sets_encoding_reproduces_the_graph():
    for name, n, pairs in CASES[::7]:
        offsets, values = CL.as_sets(n, pairs)
        S = [set(values[int(offsets[v]):int(offsets[v + 1])].tolist()) for v in range(n)]
        assert all(list(values[int(offsets[v]):int(offsets[v + 1])]) == sorted(S[v]) for v in range(n))
        got = sorted((u, v) for u in range(n) for v in range(u + 1, n) if S[u] & S[v])
        assert got == CL.edge_list(*CL.csr(n, pairs)[:2]), name
        assert all(S[v] for v in range(n))  # the private value: every set lists itself on the diagonal
