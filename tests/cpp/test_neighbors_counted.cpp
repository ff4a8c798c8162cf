// C++ test of the weighted sparse all-pairs comparison through the RAII owners of bio_amd/csrc/sketches.hpp: DeviceSets::neighbors_counted
// against a per-pair walk with counts and the rule of include/biosketch.h -- the hand case at limits 0, 1, 2, 3 and 100 with its numbers
// written out, and one object re-used through search, neighbors_counted, top and neighbors -- and SearchHits::weights_device /
// fetch_weights.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
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

struct Collection {
    std::vector<uint64_t> offsets{0}, values;
    std::vector<uint32_t> counts;
    void add(const std::vector<uint64_t> &s, const std::vector<uint32_t> &c) {
        values.insert(values.end(), s.begin(), s.end());
        counts.insert(counts.end(), c.begin(), c.end());
        offsets.push_back(values.size());
    }
    size_t n() const { return offsets.size() - 1; }
    std::map<uint64_t, uint32_t> set(size_t i) const {
        std::map<uint64_t, uint32_t> m;
        for (uint64_t p = offsets[i]; p < offsets[i + 1]; ++p) m[values[p]] = counts[p];
        return m;
    }
};

struct Cell {
    uint32_t shared = 0, total = 0;
    uint64_t dot = 0, min_sum = 0;
};

// the walk: the first `limit` values of the union (0: all); over those both sets hold, the products (saturating) and the minima
static Cell walk(const std::map<uint64_t, uint32_t> &a, const std::map<uint64_t, uint32_t> &b, uint64_t limit) {
    std::map<uint64_t, int> u;
    for (auto &kv : a) u[kv.first] |= 1;
    for (auto &kv : b) u[kv.first] |= 2;
    Cell c;
    for (auto &kv : u) {
        if (limit && c.total >= limit) break;
        ++c.total;
        if (kv.second == 3) {
            const uint64_t ca = a.at(kv.first), cb = b.at(kv.first), p = ca * cb;
            ++c.shared;
            c.dot = c.dot + p < p ? ~0ull : c.dot + p;
            c.min_sum += std::min(ca, cb);
        }
    }
    return c;
}

struct Csr {
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> target, shared, total;
    std::vector<uint64_t> dot, min_sum;
    bool operator==(const Csr &o) const {
        return offsets == o.offsets && target == o.target && shared == o.shared && total == o.total && dot == o.dot && min_sum == o.min_sum;
    }
};

static Csr model(const Collection &a, const Collection &b, uint64_t limit, const bsk_neighbor_params &np) {
    Csr m;
    m.offsets.push_back(0);
    for (size_t i = 0; i < a.n(); ++i) {
        for (size_t j = 0; j < b.n(); ++j) {
            const Cell c = walk(a.set(i), b.set(j), limit);
            const bool keep = c.shared >= std::max<uint32_t>(np.min_shared, 1) &&
                              (np.jaccard_den == 0 || (uint64_t)c.shared * np.jaccard_den >= (uint64_t)np.jaccard_num * c.total) &&
                              (!(np.flags & BSK_NEIGHBORS_UPPER) || j > i);  // the weights take no part
            if (keep) {
                m.target.push_back((uint32_t)j);
                m.shared.push_back(c.shared);
                m.total.push_back(c.total);
                m.dot.push_back(c.dot);
                m.min_sum.push_back(c.min_sum);
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
    CHECK(h.fetch_weights(e, g.dot, g.min_sum) == BSK_OK);
    return g;
}

static bool weighted(const SearchHits &h) { return h.weights_device().first != nullptr && h.weights_device().second != nullptr; }
static bool unweighted(const SearchHits &h) { return h.weights_device().first == nullptr && h.weights_device().second == nullptr; }

int main() {
    Engine e(0);
    // the hand case: A = {1 3 5 7} {} {2 3}, B = {3 4 5} {7}, with counts
    Collection a, b;
    a.add({1, 3, 5, 7}, {2, 3, 1, 4});
    a.add({}, {});
    a.add({2, 3}, {5, 2});
    b.add({3, 4, 5}, {2, 7, 6});
    b.add({7}, {3});
    DeviceSets da, db;
    CHECK(da.from_host_counted(e, a.offsets, a.values, a.counts) == BSK_OK && db.from_host_counted(e, b.offsets, b.values, b.counts) == BSK_OK);
    SearchHits h;
    CHECK(da.neighbors_counted(e, db, 0, nullptr, h) == BSK_OK && weighted(h) && h.totals_device() != nullptr && h.large_queries() == 0);
    Csr g = fetched(e, h);
    CHECK((g.offsets == std::vector<uint64_t>{0, 2, 2, 3}) && (g.target == std::vector<uint32_t>{0, 1, 0}) && (g.shared == std::vector<uint32_t>{2, 1, 1}) &&
          (g.total == std::vector<uint32_t>{5, 4, 4}) && (g.dot == std::vector<uint64_t>{3 * 2 + 1 * 6, 4 * 3, 2 * 2}) && (g.min_sum == std::vector<uint64_t>{2 + 1, 3, 2}));
    CHECK(da.neighbors_counted(e, db, 1, nullptr, h) == BSK_OK && fetched(e, h).target.empty() && weighted(h));  // one value walked, never a shared one
    CHECK(da.neighbors_counted(e, db, 2, nullptr, h) == BSK_OK);
    g = fetched(e, h);
    CHECK((g.offsets == std::vector<uint64_t>{0, 1, 1, 2}) && (g.target == std::vector<uint32_t>{0, 0}) && (g.dot == std::vector<uint64_t>{6, 4}) &&
          (g.min_sum == std::vector<uint64_t>{2, 2}) && (g.total == std::vector<uint32_t>{2, 2}));
    for (uint64_t limit : {0ull, 1ull, 2ull, 3ull, 100ull}) {
        bsk_neighbor_params np{};
        CHECK(da.neighbors_counted(e, db, limit, &np, h) == BSK_OK && fetched(e, h) == model(a, b, limit, np));
        np.jaccard_num = 1, np.jaccard_den = 4;
        CHECK(da.neighbors_counted(e, db, limit, &np, h) == BSK_OK && fetched(e, h) == model(a, b, limit, np));
        np.min_shared = 2;
        CHECK(da.neighbors_counted(e, db, limit, &np, h) == BSK_OK && fetched(e, h) == model(a, b, limit, np));
    }
    const char *plan = "";
    bsk_hits_plan(h.get(), &plan, nullptr);
    CHECK(std::string(plan).find("bsk_sets_neighbors_counted: k_cmp_tile_nb_w") == 0 && std::string(plan).find("tiles=1 skipped=0") != std::string::npos);

    // one object through a chain: neighbors_counted -> search -> neighbors_counted on smaller operands -> top -> neighbors
    Collection c;
    for (uint64_t i = 0; i < 37; ++i) {  // 37 sets against themselves: 3 x 3 tiles; set i holds the multiples of 1 + i % 5 below 60
        std::vector<uint64_t> s;
        std::vector<uint32_t> k;
        for (uint64_t v = 1 + i % 5; v < 60; v += 1 + i % 5) s.push_back(v), k.push_back((uint32_t)(1 + (v * 7 + i) % 9));
        c.add(s, k);
    }
    DeviceSets dc;
    CHECK(dc.from_host_counted(e, c.offsets, c.values, c.counts) == BSK_OK);
    bsk_neighbor_params all{}, up{2, BSK_NEIGHBORS_UPPER, 1, 3};
    SearchHits s;
    CHECK(dc.neighbors_counted(e, dc, 0, &all, s) == BSK_OK && weighted(s) && fetched(e, s) == model(c, c, 0, all));
    const Csr whole = fetched(e, s);
    const uint64_t *o0 = nullptr;
    const uint32_t *t0 = nullptr, *s0 = nullptr, *tt0 = s.totals_device();
    CHECK(bsk_hits_device(s.get(), &o0, &t0, &s0) == BSK_OK);
    const auto w0 = s.weights_device();
    SearchIndex ix;
    CHECK(ix.build(e, dc) == BSK_OK);
    bsk_search_params sp{1, 0, 0.0, 0.0};
    CHECK(ix.search(e, dc, sp, s) == BSK_OK && unweighted(s) && s.totals_device() == nullptr);
    std::vector<uint64_t> nd, nm;
    CHECK(s.fetch_weights(e, nd, nm) == BSK_ERR_ARG);
    CHECK(da.neighbors_counted(e, db, 0, nullptr, s) == BSK_OK && weighted(s));  // smaller operands: no array moves
    const uint64_t *o1 = nullptr;
    const uint32_t *t1 = nullptr, *s1 = nullptr;
    CHECK(bsk_hits_device(s.get(), &o1, &t1, &s1) == BSK_OK && o1 == o0 && t1 == t0 && s1 == s0 && s.totals_device() == tt0 && s.weights_device() == w0);
    CHECK(dc.neighbors_counted(e, dc, 64, &up, s) == BSK_OK);
    g = fetched(e, s);
    CHECK(g == model(c, c, 64, up) && !g.target.empty());
    bsk_hits_plan(s.get(), &plan, nullptr);
    CHECK(std::string(plan).find("tiles=6 skipped=3") != std::string::npos);
    SearchHits top;
    CHECK(s.top(e, 2, top) == BSK_OK && unweighted(top) && top.totals_device() == nullptr);
    CHECK(top.fetch_weights(e, nd, nm) == BSK_ERR_ARG);
    CHECK(dc.neighbors(e, dc, 0, &all, s) == BSK_OK && unweighted(s) && s.totals_device() != nullptr);
    std::vector<uint64_t> so;
    std::vector<uint32_t> st, ss, stt;
    CHECK(s.fetch(e, so, st, ss) == BSK_OK && s.fetch_totals(e, stt) == BSK_OK && so == whole.offsets && st == whole.target && ss == whole.shared && stt == whole.total);
    CHECK(s.fetch_weights(e, nd, nm) == BSK_ERR_ARG);

    // the owners' rules: a refused call leaves the object as it was
    bsk_hits *before = s.get();
    bsk_neighbor_params bad{1, 2, 0, 0};
    CHECK(dc.neighbors_counted(e, dc, 0, &bad, s) == BSK_ERR_ARG && s.get() == before);
    bad = bsk_neighbor_params{1, 0, 3, 2};
    CHECK(dc.neighbors_counted(e, dc, 0, &bad, s) == BSK_ERR_ARG && s.get() == before);
    DeviceSets empty;
    CHECK(dc.neighbors_counted(e, empty, 0, nullptr, s) == BSK_ERR_ARG && s.get() == before);

    std::printf(fails ? "FAILED %d checks\n" : "all C++ neighbors_counted checks passed\n", fails);
    return fails ? 1 : 0;
}
