// C++ test of the clusters of a hits graph through the RAII owners of bio_amd/csrc/sketches.hpp: SearchHits::from_host and
// SearchHits::cluster against a union-find and the sequential greedy rule of include/biosketch.h -- a hand case, seeded random graphs in
// full and upper form under scores with ties, the graph of a DeviceSets::neighbors call, the re-use of a Clusters object and the refusals.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "sketches.hpp"

using namespace sketches;

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                               \
        }                                                          \
    } while (0)

struct Graph {
    uint64_t n = 0;
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> target, shared;
    std::set<std::pair<uint32_t, uint32_t>> edges;  // undirected, u < v
};

// directed hits -> CSR (rows ascending, a repeated hit once) and the undirected edges the contract reads from them
static Graph graph(uint64_t n, const std::vector<std::pair<uint32_t, uint32_t>> &hits) {
    Graph g;
    g.n = n;
    std::vector<std::set<uint32_t>> rows(n);
    for (auto [i, j] : hits) {
        rows[i].insert(j);
        if (i != j) g.edges.insert({std::min(i, j), std::max(i, j)});
    }
    g.offsets.push_back(0);
    for (auto &r : rows) {
        g.target.insert(g.target.end(), r.begin(), r.end());
        g.offsets.push_back(g.target.size());
    }
    g.shared.assign(g.target.size(), 1);
    return g;
}

struct Found {
    std::vector<uint32_t> label, rep, members;
    std::vector<uint64_t> offsets;
    uint64_t largest = 0;
    bool operator==(const Found &o) const { return label == o.label && rep == o.rep && members == o.members && offsets == o.offsets && largest == o.largest; }
};

static std::vector<uint32_t> ranks(uint64_t n, const std::vector<uint64_t> &score, std::vector<uint32_t> &order) {
    order.resize(n);
    std::iota(order.begin(), order.end(), 0u);
    if (!score.empty()) std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return score[a] != score[b] ? score[a] > score[b] : a < b; });
    std::vector<uint32_t> rank(n);
    for (uint32_t r = 0; r < n; ++r) rank[order[r]] = r;
    return rank;
}

static Found layout(const std::vector<uint32_t> &rep_of) {
    Found m;
    const size_t n = rep_of.size();
    std::set<uint32_t> reps(rep_of.begin(), rep_of.end());
    m.rep.assign(reps.begin(), reps.end());
    m.label.resize(n);
    std::vector<std::vector<uint32_t>> groups(m.rep.size());
    for (uint32_t v = 0; v < n; ++v) {
        m.label[v] = (uint32_t)(std::lower_bound(m.rep.begin(), m.rep.end(), rep_of[v]) - m.rep.begin());
        groups[m.label[v]].push_back(v);
    }
    m.offsets.push_back(0);
    for (auto &g : groups) {
        m.members.insert(m.members.end(), g.begin(), g.end());
        m.offsets.push_back(m.members.size());
        m.largest = std::max<uint64_t>(m.largest, g.size());
    }
    return m;
}

static Found model(const Graph &g, uint32_t method, const std::vector<uint64_t> &score) {
    std::vector<uint32_t> order, rank = ranks(g.n, score, order), rep_of(g.n);
    if (method == BSK_CLUSTER_COMPONENTS) {
        std::vector<uint32_t> parent(g.n);
        std::iota(parent.begin(), parent.end(), 0u);
        auto find = [&](uint32_t x) {
            while (parent[x] != x) x = parent[x] = parent[parent[x]];
            return x;
        };
        for (auto [u, v] : g.edges) parent[find(u)] = find(v);
        std::vector<uint32_t> best(g.n, 0xffffffffu);
        for (uint32_t v = 0; v < g.n; ++v) {
            const uint32_t r = find(v);
            if (best[r] == 0xffffffffu || rank[v] < rank[best[r]]) best[r] = v;
        }
        for (uint32_t v = 0; v < g.n; ++v) rep_of[v] = best[find(v)];
    } else {
        std::vector<std::vector<uint32_t>> nbr(g.n);
        for (auto [u, v] : g.edges) nbr[u].push_back(v), nbr[v].push_back(u);
        std::vector<char> is_rep(g.n, 0);
        for (uint32_t v : order) {
            uint32_t pick = 0xffffffffu;
            for (uint32_t u : nbr[v])
                if (is_rep[u] && (pick == 0xffffffffu || rank[u] < rank[pick])) pick = u;
            if (pick == 0xffffffffu) is_rep[v] = 1, pick = v;
            rep_of[v] = pick;
        }
    }
    return layout(rep_of);
}

static Found fetched(Engine &e, const Clusters &c) {
    Found r;
    CHECK(c.fetch(e, r.label, r.rep, r.offsets, r.members) == BSK_OK);
    r.largest = c.largest();
    CHECK(c.n_items() == r.label.size() && c.n_clusters() == r.rep.size());
    return r;
}

int main() {
    Engine e(0);
    // the hand case: 0 - 1 - 2, 3 alone with a diagonal hit, 4 - 5 stated in one direction only
    Graph g = graph(6, {{0, 1}, {1, 0}, {1, 2}, {2, 1}, {3, 3}, {5, 4}});
    SearchHits h;
    CHECK(h.from_host(e, g.offsets, g.target, g.shared) == BSK_OK && h.totals_device() == nullptr);
    const char *hplan = "";
    bsk_hits_plan(h.get(), &hplan, nullptr);
    CHECK(std::string(hplan) == "from host");
    Clusters c;
    CHECK(h.cluster(e, BSK_CLUSTER_COMPONENTS, {}, c) == BSK_OK);
    Found r = fetched(e, c);
    CHECK((r.label == std::vector<uint32_t>{0, 0, 0, 1, 2, 2}) && (r.rep == std::vector<uint32_t>{0, 3, 4}) && (r.offsets == std::vector<uint64_t>{0, 3, 4, 6}) &&
          (r.members == std::vector<uint32_t>{0, 1, 2, 3, 4, 5}) && r.largest == 3);
    CHECK(c.edges() == 5 && c.rounds() >= 1 && c.plan().find("k_cl_hook+k_cl_jump, n=6 edges=5 rounds=") == 0);
    // greedy with node 1 best: it takes 0 and 2; 5 beats 4 by score
    const std::vector<uint64_t> score{1, 9, 1, 0, 2, 3};
    CHECK(h.cluster(e, BSK_CLUSTER_GREEDY, score, c) == BSK_OK);
    r = fetched(e, c);
    CHECK((r.label == std::vector<uint32_t>{0, 0, 0, 1, 2, 2}) && (r.rep == std::vector<uint32_t>{1, 3, 5}) && r == model(g, BSK_CLUSTER_GREEDY, score));
    CHECK(c.plan().find("k_cl_mis, n=6 edges=5 rounds=") == 0);
    // greedy is not transitive: on the path 0 - 1 - 2 - 3 in index order 0 and 2 represent, 3 joins 2
    g = graph(4, {{0, 1}, {1, 2}, {2, 3}});
    CHECK(h.from_host(e, g.offsets, g.target, g.shared) == BSK_OK && h.cluster(e, BSK_CLUSTER_GREEDY, {}, c) == BSK_OK);
    r = fetched(e, c);
    CHECK((r.rep == std::vector<uint32_t>{0, 2}) && (r.label == std::vector<uint32_t>{0, 0, 1, 1}) && c.rounds() == 4);

    // seeded graphs, full and upper form, scores with ties: both methods against the models, into one re-used object
    std::mt19937_64 rng(20262);
    for (int round = 0; round < 24; ++round) {
        const uint64_t n = 1 + rng() % 300;
        std::vector<std::pair<uint32_t, uint32_t>> full, upper;
        const uint64_t m = rng() % (2 * n);
        for (uint64_t k = 0; k < m; ++k) {
            const uint32_t u = (uint32_t)(rng() % n), v = (uint32_t)(rng() % n);
            full.push_back({u, v}), full.push_back({v, u});
            upper.push_back({std::min(u, v), std::max(u, v)});
        }
        std::vector<uint64_t> sc(n);
        for (auto &x : sc) x = round % 3 == 0 ? ~0ull * (rng() & 1) : rng() % 4;
        const Graph gf = graph(n, full), gu = graph(n, upper);
        SearchHits hf, hu;
        CHECK(hf.from_host(e, gf.offsets, gf.target, gf.shared) == BSK_OK && hu.from_host(e, gu.offsets, gu.target, gu.shared, gu.shared) == BSK_OK);
        CHECK(gu.target.empty() || hu.totals_device() != nullptr);  // (an empty total[] stands for "no totals")
        for (uint32_t method : {(uint32_t)BSK_CLUSTER_COMPONENTS, (uint32_t)BSK_CLUSTER_GREEDY}) {
            for (int scored = 0; scored < 2; ++scored) {
                const std::vector<uint64_t> s = scored ? sc : std::vector<uint64_t>{};
                const Found want = model(gf, method, s);
                CHECK(hf.cluster(e, method, s, c) == BSK_OK && fetched(e, c) == want);
                CHECK(hu.cluster(e, method, s, c) == BSK_OK && fetched(e, c) == want);
                CHECK(c.rounds() >= 1 && c.rounds() <= n + 1);
            }
        }
    }

    // the graph of a neighbours call: 12 families of 3 sets that share most of their values
    std::vector<uint64_t> so{0}, sv;
    for (uint64_t s = 0; s < 36; ++s) {
        for (uint64_t k = 0; k < 40; ++k) sv.push_back((s % 12) * 1000 + k);  // the family's values
        for (uint64_t k = 0; k < 5; ++k) sv.push_back(100000 + s * 10 + k);   // the set's own
        so.push_back(sv.size());
    }
    DeviceSets ds;
    CHECK(ds.from_host(e, so, sv) == BSK_OK);
    bsk_neighbor_params np{1, BSK_NEIGHBORS_UPPER, 1, 2};
    SearchHits nb;
    CHECK(ds.neighbors(e, ds, 0, &np, nb) == BSK_OK && h.cluster(e, BSK_CLUSTER_GREEDY, {}, c) == BSK_OK);
    CHECK(nb.cluster(e, BSK_CLUSTER_COMPONENTS, {}, c) == BSK_OK);
    r = fetched(e, c);
    CHECK(r.rep.size() == 12 && r.largest == 3 && c.edges() == 36);
    for (uint32_t v = 0; v < 36; ++v) CHECK(r.label[v] == v % 12 && r.rep[r.label[v]] == v % 12);

    // refusals leave the object as it was: an unknown method, a flag, a score of the wrong length, a target that is no node
    bsk_clusters *before = c.get();
    CHECK(nb.cluster(e, 2, {}, c) == BSK_ERR_ARG && c.get() == before);
    const bsk_cluster_params flagged{0, 4};
    CHECK(bsk_hits_cluster(e.ctx(), nb.get(), &flagged, nullptr, &c.handle()) == BSK_ERR_ARG && c.get() == before);
    CHECK(nb.cluster(e, 0, std::vector<uint64_t>(35, 1), c) == BSK_ERR_ARG && c.get() == before);
    SearchHits rect;
    CHECK(rect.from_host(e, {0, 1, 2}, {1, 2}, {1, 1}) == BSK_OK);
    CHECK(rect.cluster(e, BSK_CLUSTER_COMPONENTS, {}, c) == BSK_ERR_ARG && c.get() == before && fetched(e, c) == r);
    bsk_hits *hb = rect.get();
    CHECK(rect.from_host(e, {0, 2, 1}, {1, 2}, {1, 1}) == BSK_ERR_ARG && rect.from_host(e, {0, 2, 2}, {2, 2}, {1, 1}) == BSK_ERR_ARG && rect.get() == hb);
    // no nodes
    SearchHits none;
    CHECK(none.from_host(e, {0}, {}, {}) == BSK_OK && none.cluster(e, BSK_CLUSTER_GREEDY, {}, c) == BSK_OK && c.n_items() == 0 && c.n_clusters() == 0 && c.rounds() == 0);

    std::printf(fails ? "FAILED %d checks\n" : "all C++ cluster checks passed\n", fails);
    return fails ? 1 : 0;
}
