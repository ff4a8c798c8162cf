// C++ test of the containment search through the RAII owners of bio_amd/csrc/sketches.hpp: random target and query sets drawn from a
// shared value pool (the values 0 and 2^64-1 included), searched on the device, compared with a std::unordered_map count.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <unordered_map>
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
    void add(std::vector<uint64_t> s) {
        std::sort(s.begin(), s.end());
        s.erase(std::unique(s.begin(), s.end()), s.end());
        values.insert(values.end(), s.begin(), s.end());
        offsets.push_back(values.size());
    }
    size_t n() const { return offsets.size() - 1; }
    uint64_t size(size_t i) const { return offsets[i + 1] - offsets[i]; }
};

static Collection random_sets(std::mt19937_64 &rng, const std::vector<uint64_t> &pool, size_t n, size_t max_size) {
    Collection c;
    for (size_t i = 0; i < n; ++i) {
        const size_t sz = rng() % (max_size + 1);
        std::vector<uint64_t> s(sz);
        for (auto &v : s) v = pool[rng() % pool.size()];
        c.add(std::move(s));
    }
    return c;
}

// the contract's listing rule and order, on the host
static void expected(const Collection &tg, const Collection &q, const bsk_search_params &sp, std::vector<uint64_t> &offs, std::vector<uint32_t> &tgt,
                     std::vector<uint32_t> &sh) {
    std::unordered_map<uint64_t, std::vector<uint32_t>> post;
    for (size_t t = 0; t < tg.n(); ++t)
        for (uint64_t i = tg.offsets[t]; i < tg.offsets[t + 1]; ++i) post[tg.values[i]].push_back((uint32_t)t);
    const uint32_t ms = sp.min_shared ? sp.min_shared : 1;
    offs.assign(1, 0);
    tgt.clear();
    sh.clear();
    for (size_t k = 0; k < q.n(); ++k) {
        std::unordered_map<uint32_t, uint32_t> count;
        for (uint64_t i = q.offsets[k]; i < q.offsets[k + 1]; ++i) {
            auto it = post.find(q.values[i]);
            if (it != post.end())
                for (uint32_t t : it->second) ++count[t];
        }
        std::vector<std::pair<uint32_t, uint32_t>> hits(count.begin(), count.end());
        std::sort(hits.begin(), hits.end());
        for (auto &h : hits) {
            const uint32_t s = h.second;
            if (s >= ms && (double)s >= sp.min_query_cov * (double)q.size(k) && (double)s >= sp.min_target_cov * (double)tg.size(h.first)) {
                tgt.push_back(h.first);
                sh.push_back(s);
            }
        }
        offs.push_back(tgt.size());
    }
}

int main() {
    Engine e(0);
    std::mt19937_64 rng(0x5EA2C4);
    std::vector<uint64_t> pool(6000);
    for (auto &v : pool) v = rng();
    pool[0] = 0;
    pool[1] = ~0ULL;
    for (int i = 2; i < 200; ++i) pool[i] = (uint64_t)i;  // clustered small values
    Collection tg = random_sets(rng, pool, 400, 500);
    tg.add({});          // an empty target
    tg.add({0, ~0ULL});  // the extreme values
    Collection q = random_sets(rng, pool, 3000, 60);
    q.add({});
    q.add(std::vector<uint64_t>(tg.values.begin() + tg.offsets[7], tg.values.begin() + tg.offsets[8]));  // a query equal to a target
    for (int i = 0; i < 4; ++i) {  // queries beyond the LDS budget: the large path
        std::vector<uint64_t> s(pool.begin(), pool.end());
        std::shuffle(s.begin(), s.end(), rng);
        s.resize(2500 + 500 * i);
        q.add(std::move(s));
    }
    DeviceSets dt, dq;
    CHECK(dt.from_host(e, tg.offsets, tg.values) == BSK_OK && dt.n_sets() == tg.n());
    CHECK(dq.from_host(e, q.offsets, q.values) == BSK_OK && dq.n_sets() == q.n());
    SearchIndex ix;
    CHECK(ix.build(e, dt) == BSK_OK);
    CHECK(ix.max_bucket() >= 1 && ix.max_bucket() <= 32);
    dt = DeviceSets();  // the index owns what it needs
    const bsk_search_params params[3] = {{0, 0, 0.0, 0.0}, {2, 0, 0.25, 0.0}, {1, 0, 0.0, 0.05}};
    SearchHits hits;  // one object, re-used by every search
    for (const auto &sp : params) {
        CHECK(ix.search(e, dq, sp, hits) == BSK_OK);
        std::vector<uint64_t> o, eo;
        std::vector<uint32_t> t, s, et, es;
        CHECK(hits.fetch(e, o, t, s) == BSK_OK);
        expected(tg, q, sp, eo, et, es);
        CHECK(o == eo);
        CHECK(t == et);
        CHECK(s == es);
        CHECK(hits.large_queries() >= 4);
        std::printf("min_shared %u qcov %.2f tcov %.2f: %zu hits (expected %zu), %llu large queries\n", sp.min_shared, sp.min_query_cov, sp.min_target_cov,
                    t.size(), et.size(), (unsigned long long)hits.large_queries());
    }
    // bad arguments
    bsk_search_params bad{1, 1, 0.0, 0.0};
    CHECK(ix.search(e, dq, bad, hits) == BSK_ERR_ARG);
    bad = {1, 0, 1.5, 0.0};
    CHECK(ix.search(e, dq, bad, hits) == BSK_ERR_ARG);
    DeviceSets unsorted;
    CHECK(unsorted.from_host(e, {0, 2}, {5, 3}) == BSK_ERR_ARG && unsorted.get() == nullptr);
    std::printf(fails ? "FAILED %d checks\n" : "all C++ search checks passed\n", fails);
    return fails ? 1 : 0;
}
