// C++ test of the sparse all-pairs comparison through the RAII owners of bio_amd/csrc/sketches.hpp: DeviceSets::neighbors against a
// std::set_union walk and the rule of include/biosketch.h -- one hand case, one BSK_NEIGHBORS_UPPER case of more than one tile, one re-use
// (hits of a search taken over, then a search into them again) -- and SearchHits::totals_device / fetch_totals.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <iterator>
#include <random>
#include <string>
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

using Set = std::vector<uint64_t>;
struct Collection {
    std::vector<uint64_t> offsets{0}, values;
    void add(const Set &s) {
        values.insert(values.end(), s.begin(), s.end());
        offsets.push_back(values.size());
    }
    size_t n() const { return offsets.size() - 1; }
    Set set(size_t i) const { return Set(values.begin() + offsets[i], values.begin() + offsets[i + 1]); }
};

// the walk: the first `limit` values of the union (0: all), and how many of them both sets hold
static void walk(const Set &a, const Set &b, uint64_t limit, uint32_t &shared, uint32_t &total) {
    Set u, both;
    std::set_union(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(u));
    std::set_intersection(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(both));
    if (limit && u.size() > limit) u.resize(limit);
    total = (uint32_t)u.size();
    shared = 0;
    for (uint64_t v : both)
        if (!u.empty() && v <= u.back()) ++shared;
}

struct Csr {
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> target, shared, total;
    bool operator==(const Csr &o) const { return offsets == o.offsets && target == o.target && shared == o.shared && total == o.total; }
};

static Csr model(const Collection &a, const Collection &b, uint64_t limit, const bsk_neighbor_params &np) {
    Csr m;
    m.offsets.push_back(0);
    for (size_t i = 0; i < a.n(); ++i) {
        for (size_t j = 0; j < b.n(); ++j) {
            uint32_t s = 0, t = 0;
            walk(a.set(i), b.set(j), limit, s, t);
            const bool keep = s >= std::max<uint32_t>(np.min_shared, 1) && (np.jaccard_den == 0 || (uint64_t)s * np.jaccard_den >= (uint64_t)np.jaccard_num * t) &&
                              (!(np.flags & BSK_NEIGHBORS_UPPER) || j > i);
            if (keep) {
                m.target.push_back((uint32_t)j);
                m.shared.push_back(s);
                m.total.push_back(t);
            }
        }
        m.offsets.push_back(m.target.size());
    }
    return m;
}

static Csr fetched(Engine &e, const SearchHits &h) {
    Csr g;
    CHECK(h.fetch(e, g.offsets, g.target, g.shared) == BSK_OK);
    CHECK(h.fetch_totals(e, g.total) == BSK_OK);
    return g;
}

static Set random_set(std::mt19937_64 &rng, size_t n, uint64_t pool) {
    Set s;
    while (s.size() < n) {
        s.push_back(rng() % pool * 0x9E3779B97F4A7C15ull);
        std::sort(s.begin(), s.end());
        s.erase(std::unique(s.begin(), s.end()), s.end());
    }
    return s;
}

int main() {
    Engine e(0);
    // the hand case: 3 x 2 with an empty set
    Collection a, b;
    a.add({1, 3, 5, 7});
    a.add({});
    a.add({2, 3});
    b.add({3, 4, 5});
    b.add({7});
    DeviceSets da, db;
    CHECK(da.from_host(e, a.offsets, a.values) == BSK_OK && db.from_host(e, b.offsets, b.values) == BSK_OK);
    SearchHits h;
    CHECK(da.neighbors(e, db, 0, nullptr, h) == BSK_OK);
    Csr g = fetched(e, h);
    CHECK((g.offsets == std::vector<uint64_t>{0, 2, 2, 3}) && (g.target == std::vector<uint32_t>{0, 1, 0}) && (g.shared == std::vector<uint32_t>{2, 1, 1}) &&
          (g.total == std::vector<uint32_t>{5, 4, 4}));
    CHECK(h.totals_device() != nullptr && h.large_queries() == 0);
    for (uint64_t limit : {0ull, 1ull, 2ull, 3ull, 100ull}) {
        bsk_neighbor_params np{};
        CHECK(da.neighbors(e, db, limit, &np, h) == BSK_OK && fetched(e, h) == model(a, b, limit, np));
        np.jaccard_num = 1, np.jaccard_den = 4;  // met exactly by the pairs of one shared value in four
        CHECK(da.neighbors(e, db, limit, &np, h) == BSK_OK && fetched(e, h) == model(a, b, limit, np));
        np.min_shared = 2;
        CHECK(da.neighbors(e, db, limit, &np, h) == BSK_OK && fetched(e, h) == model(a, b, limit, np));
    }

    // more than one tile, a == b, with and without the triangle
    std::mt19937_64 rng(20261);
    Collection c;
    for (int i = 0; i < 37; ++i) c.add(random_set(rng, i == 5 ? 0 : 1 + rng() % 300, 900));
    DeviceSets dc;
    CHECK(dc.from_host(e, c.offsets, c.values) == BSK_OK);
    for (uint64_t limit : {0ull, 64ull}) {
        bsk_neighbor_params np{3, BSK_NEIGHBORS_UPPER, 1, 10};
        CHECK(dc.neighbors(e, dc, limit, &np, h) == BSK_OK);
        g = fetched(e, h);
        CHECK(g == model(c, c, limit, np) && !g.target.empty());
        for (size_t i = 0; i < c.n(); ++i)
            for (uint64_t p = g.offsets[i]; p < g.offsets[i + 1]; ++p) CHECK(g.target[p] > i);
        const char *plan = "";
        bsk_hits_plan(h.get(), &plan, nullptr);
        CHECK(std::string(plan).find("k_cmp_tile_nb") != std::string::npos && std::string(plan).find("tiles=6 skipped=3") != std::string::npos);  // 3 x 3 tiles
        np.flags = 0;
        CHECK(dc.neighbors(e, dc, limit, &np, h) == BSK_OK && fetched(e, h) == model(c, c, limit, np));
    }

    // re-use: the hits of a search taken over, the n best of the result, then a search into the object again
    SearchIndex ix;
    CHECK(ix.build(e, dc) == BSK_OK);
    bsk_search_params sp{1, 0, 0.0, 0.0};
    SearchHits s;
    CHECK(ix.search(e, dc, sp, s) == BSK_OK && s.totals_device() == nullptr);
    std::vector<uint32_t> none;
    CHECK(s.fetch_totals(e, none) == BSK_ERR_ARG);
    bsk_neighbor_params all{};
    CHECK(dc.neighbors(e, dc, 0, &all, s) == BSK_OK && s.totals_device() != nullptr && fetched(e, s) == model(c, c, 0, all));
    Csr whole = fetched(e, s);
    SearchHits top;
    CHECK(s.top(e, 1, top) == BSK_OK && top.totals_device() == nullptr);
    std::vector<uint64_t> to;
    std::vector<uint32_t> tt, ts;
    CHECK(top.fetch(e, to, tt, ts) == BSK_OK);
    for (size_t i = 0; i < c.n(); ++i) {  // the row's largest shared count, at its smallest target (an empty set has no neighbour)
        uint64_t best = whole.offsets[i];
        for (uint64_t p = whole.offsets[i]; p < whole.offsets[i + 1]; ++p)
            if (whole.shared[p] > whole.shared[best]) best = p;
        if (c.set(i).empty()) CHECK(to[i + 1] == to[i] && whole.offsets[i + 1] == whole.offsets[i]);
        else CHECK(to[i + 1] == to[i] + 1 && tt[to[i]] == whole.target[best] && ts[to[i]] == whole.shared[best] && ts[to[i]] == c.set(i).size());
    }
    CHECK(ix.search(e, dc, sp, s) == BSK_OK && s.totals_device() == nullptr);
    std::vector<uint64_t> so;
    std::vector<uint32_t> st, ss;
    CHECK(s.fetch(e, so, st, ss) == BSK_OK && so == whole.offsets && st == whole.target && ss == whole.shared);  // whole sets: the search lists the same pairs

    // the owners' rules: a refused call leaves the object as it was
    bsk_hits *before = s.get();
    bsk_neighbor_params bad{1, 2, 0, 0};
    CHECK(dc.neighbors(e, dc, 0, &bad, s) == BSK_ERR_ARG && s.get() == before);
    bad = bsk_neighbor_params{1, 0, 3, 2};
    CHECK(dc.neighbors(e, dc, 0, &bad, s) == BSK_ERR_ARG && s.get() == before);
    DeviceSets empty;
    CHECK(dc.neighbors(e, empty, 0, nullptr, s) == BSK_ERR_ARG && s.get() == before);

    std::printf(fails ? "FAILED %d checks\n" : "all C++ neighbors checks passed\n", fails);
    return fails ? 1 : 0;
}
