// C++ test of the weighted containment search through the RAII owners of bio_amd/csrc/sketches.hpp: SearchIndex::build_counted / counted /
// fetch_norms / search_counted against a std::map walk over every (query, target) pair and the rule of include/biosketch.h -- a hand case
// with its numbers written out, the four combinations of counted and uncounted operands, a collection with a query on the large path, and
// one object re-used through search_counted, search and top.
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
    size_t size(size_t i) const { return offsets[i + 1] - offsets[i]; }
    // value -> count; counted == false: every count 1
    std::map<uint64_t, uint64_t> set(size_t i, bool counted) const {
        std::map<uint64_t, uint64_t> m;
        for (uint64_t p = offsets[i]; p < offsets[i + 1]; ++p) m[values[p]] = counted ? counts[p] : 1;
        return m;
    }
};

struct Csr {
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> target, shared;
    std::vector<uint64_t> dot, min_sum;
    bool operator==(const Csr &o) const { return offsets == o.offsets && target == o.target && shared == o.shared && dot == o.dot && min_sum == o.min_sum; }
};

// every pair walked as two maps; the rule reads shared alone
static Csr model(const Collection &t, bool tc, const Collection &q, bool qc, const bsk_search_params &sp) {
    Csr m;
    m.offsets.push_back(0);
    for (size_t i = 0; i < q.n(); ++i) {
        const auto qs = q.set(i, qc);
        for (size_t j = 0; j < t.n(); ++j) {
            const auto ts = t.set(j, tc);
            uint32_t s = 0;
            uint64_t dot = 0, ms = 0;
            for (auto &kv : qs) {
                auto it = ts.find(kv.first);
                if (it == ts.end()) continue;
                const uint64_t p = kv.second * it->second;
                ++s;
                dot = dot + p < p ? ~0ull : dot + p;
                ms += std::min(kv.second, it->second);
            }
            if (s >= std::max<uint32_t>(sp.min_shared, 1) && (double)s >= sp.min_query_cov * (double)q.size(i) && (double)s >= sp.min_target_cov * (double)t.size(j)) {
                m.target.push_back((uint32_t)j);
                m.shared.push_back(s);
                m.dot.push_back(dot);
                m.min_sum.push_back(ms);
            }
        }
        m.offsets.push_back(m.target.size());
    }
    return m;
}

static Csr fetched(Engine &e, const SearchHits &h) {
    Csr g;
    CHECK(h.fetch(e, g.offsets, g.target, g.shared) == BSK_OK);
    CHECK(h.fetch_weights(e, g.dot, g.min_sum) == BSK_OK);
    return g;
}

static bool weighted(const SearchHits &h) { return h.weights_device().first != nullptr && h.weights_device().second != nullptr; }
static bool unweighted(const SearchHits &h) { return h.weights_device().first == nullptr && h.weights_device().second == nullptr; }
static std::string plan_of(const SearchHits &h) {
    const char *p = "";
    bsk_hits_plan(h.get(), &p, nullptr);
    return p;
}

int main() {
    Engine e(0);
    const uint32_t M = 0xFFFFFFFFu;
    // the hand case: targets {3 4 5} {7} {} {1 3 5 7}, queries {1 3 5 7} {} {2 3}
    Collection t, q;
    t.add({3, 4, 5}, {2, 7, 6});
    t.add({7}, {3});
    t.add({}, {});
    t.add({1, 3, 5, 7}, {M, M, M, 1});
    q.add({1, 3, 5, 7}, {2, 3, 1, 4});
    q.add({}, {});
    q.add({2, 3}, {5, M});
    DeviceSets dt, dq, dtu, dqu;
    CHECK(dt.from_host_counted(e, t.offsets, t.values, t.counts) == BSK_OK && dq.from_host_counted(e, q.offsets, q.values, q.counts) == BSK_OK);
    CHECK(dtu.from_host(e, t.offsets, t.values) == BSK_OK && dqu.from_host(e, q.offsets, q.values) == BSK_OK);
    SearchIndex ix, plain, from_uncounted;
    CHECK(ix.build_counted(e, dt) == BSK_OK && ix.counted());
    CHECK(plain.build(e, dt) == BSK_OK && !plain.counted());                              // bsk_index_build of counted sets: an index without counts
    CHECK(from_uncounted.build_counted(e, dtu) == BSK_OK && !from_uncounted.counted());  // ... and so for uncounted sets through the new entry
    std::vector<uint64_t> sq, tt;
    CHECK(ix.fetch_norms(e, sq, tt) == BSK_OK && (tt == std::vector<uint64_t>{15, 3, 0, 3ull * M + 1}) && sq[0] == 4 + 49 + 36 && sq[1] == 9 && sq[2] == 0 && sq[3] == ~0ull);
    CHECK(plain.fetch_norms(e, sq, tt) == BSK_OK && (tt == std::vector<uint64_t>{3, 1, 0, 4}) && sq == tt);  // an index without counts: the sizes
    uint64_t b0 = 0, b1 = 0, p0 = 0, p1 = 0;
    CHECK(bsk_index_info(ix.get(), nullptr, &p1, nullptr, nullptr, &b1) == BSK_OK && bsk_index_info(plain.get(), nullptr, &p0, nullptr, nullptr, &b0) == BSK_OK);
    CHECK(p0 == p1 && p1 == 8 && b1 == b0 + 8 * 4 + 2 * 4 * 8);

    bsk_search_params sp{1, 0, 0.0, 0.0};
    SearchHits h;
    CHECK(ix.search_counted(e, dq, sp, h) == BSK_OK && weighted(h) && h.totals_device() == nullptr && h.members_device() == nullptr && h.large_queries() == 0);
    Csr g = fetched(e, h);
    const uint64_t mm = M;
    CHECK((g.offsets == std::vector<uint64_t>{0, 3, 3, 5}) && (g.target == std::vector<uint32_t>{0, 1, 3, 0, 3}) && (g.shared == std::vector<uint32_t>{2, 1, 4, 1, 1}));
    CHECK((g.dot == std::vector<uint64_t>{3 * 2 + 1 * 6, 4 * 3, 2 * mm + 3 * mm + mm + 4, mm * 2, mm * mm}));  // (one product of two u32 always fits)
    CHECK((g.min_sum == std::vector<uint64_t>{2 + 1, 3, 2 + 3 + 1 + 1, 2, mm}));
    CHECK(plan_of(h).find("k_sr_lookup + k_sr_small") == 0 && plan_of(h).find("; weights: k_sw_row 2 queries (<= 512 hits), k_sw_chunk 0 chunks of 256 values") != std::string::npos);
    // the four combinations, with thresholds
    for (int combo = 0; combo < 4; ++combo) {
        const bool tc = combo & 1, qc = combo & 2;
        const SearchIndex &index = tc ? ix : plain;
        const DeviceSets &queries = qc ? dq : dqu;
        for (const bsk_search_params &p : {bsk_search_params{1, 0, 0.0, 0.0}, bsk_search_params{2, 0, 0.0, 0.0}, bsk_search_params{1, 0, 0.5, 0.0}, bsk_search_params{1, 0, 0.0, 0.6}}) {
            CHECK(index.search_counted(e, queries, p, h) == BSK_OK && weighted(h));
            g = fetched(e, h);
            CHECK(g == model(t, tc, q, qc, p));
            if (!tc && !qc)
                for (size_t i = 0; i < g.target.size(); ++i) CHECK(g.dot[i] == g.shared[i] && g.min_sum[i] == g.shared[i]);
        }
    }

    // 300 targets; target j holds the multiples of 1 + j % 7 below 400, and every target holds 1000 and 1001.  Query 0 holds both and the values
    // below 300 (posting sum far beyond 2048: the large path, two chunks), the others a few values each
    Collection ct, cq;
    for (uint64_t j = 0; j < 300; ++j) {
        std::vector<uint64_t> s;
        std::vector<uint32_t> k;
        for (uint64_t v = 1 + j % 7; v < 400; v += 1 + j % 7) s.push_back(v), k.push_back((uint32_t)(1 + (v * 5 + j) % 11));
        s.push_back(1000), k.push_back(j % 3 ? 2 : M);
        s.push_back(1001), k.push_back(j % 3 ? 1 : M);
        ct.add(s, k);
    }
    {
        std::vector<uint64_t> s;
        std::vector<uint32_t> k;
        for (uint64_t v = 1; v < 300; ++v) s.push_back(v), k.push_back((uint32_t)(1 + v % 4));
        s.push_back(1000), k.push_back(M);
        s.push_back(1001), k.push_back(M);
        cq.add(s, k);
    }
    for (uint64_t i = 0; i < 20; ++i) cq.add({7 * i + 1, 7 * i + 2, 7 * i + 3}, {(uint32_t)(i + 1), 2, M});
    cq.add({5000}, {9});  // no hit
    DeviceSets dct, dcq;
    CHECK(dct.from_host_counted(e, ct.offsets, ct.values, ct.counts) == BSK_OK && dcq.from_host_counted(e, cq.offsets, cq.values, cq.counts) == BSK_OK);
    SearchIndex cix;
    CHECK(cix.build_counted(e, dct) == BSK_OK && cix.counted());
    SearchHits s;
    for (const bsk_search_params &p : {bsk_search_params{1, 0, 0.0, 0.0}, bsk_search_params{3, 0, 0.0, 0.0}, bsk_search_params{1, 0, 0.9, 0.0}}) {
        CHECK(cix.search_counted(e, dcq, p, s) == BSK_OK && weighted(s) && s.large_queries() == 1);
        g = fetched(e, s);
        CHECK(g == model(ct, true, cq, true, p) && !g.target.empty());
        CHECK(plan_of(s).find("k_sw_chunk 2 chunks of 256 values") != std::string::npos);
    }
    const Csr whole = fetched(e, s);
    CHECK(std::count(whole.dot.begin(), whole.dot.end(), ~0ull) > 0);  // query 0 against the targets that hold 1000 and 1001 with M: 2 M * M wraps

    // one object through a chain: search_counted -> search -> search_counted on smaller operands -> top
    const uint64_t *o0 = nullptr;
    const uint32_t *t0 = nullptr, *s0 = nullptr;
    CHECK(bsk_hits_device(s.get(), &o0, &t0, &s0) == BSK_OK);
    const auto w0 = s.weights_device();
    bsk_search_params all{1, 0, 0.0, 0.0};
    CHECK(cix.search(e, dcq, all, s) == BSK_OK && unweighted(s));
    std::vector<uint64_t> nd, nm;
    CHECK(s.fetch_weights(e, nd, nm) == BSK_ERR_ARG);
    CHECK(ix.search_counted(e, dq, all, s) == BSK_OK && weighted(s));  // smaller operands: no array moves
    const uint64_t *o1 = nullptr;
    const uint32_t *t1 = nullptr, *s1 = nullptr;
    CHECK(bsk_hits_device(s.get(), &o1, &t1, &s1) == BSK_OK && o1 == o0 && t1 == t0 && s1 == s0 && s.weights_device() == w0);
    CHECK(fetched(e, s) == model(t, true, q, true, all));
    SearchHits top;
    CHECK(s.top(e, 2, top) == BSK_OK && unweighted(top));
    // an attached handle shares the counts
    Engine e2(0);
    SearchIndex handle;
    CHECK(cix.attach(e2, handle) == BSK_OK && handle.counted());
    DeviceSets dcq2;
    CHECK(dcq2.from_host_counted(e2, cq.offsets, cq.values, cq.counts) == BSK_OK);
    SearchHits s2;
    CHECK(handle.search_counted(e2, dcq2, bsk_search_params{1, 0, 0.9, 0.0}, s2) == BSK_OK && fetched(e2, s2) == whole);

    // the owners' rules: a refused call leaves the object as it was
    bsk_hits *before = s.get();
    bsk_search_params bad{1, 1, 0.0, 0.0};
    CHECK(ix.search_counted(e, dq, bad, s) == BSK_ERR_ARG && s.get() == before);
    bad = bsk_search_params{1, 0, 1.5, 0.0};
    CHECK(ix.search_counted(e, dq, bad, s) == BSK_ERR_ARG && s.get() == before);
    DeviceSets empty;
    CHECK(ix.search_counted(e, empty, all, s) == BSK_ERR_ARG && s.get() == before);

    std::printf(fails ? "FAILED %d checks\n" : "all C++ search_counted checks passed\n", fails);
    return fails ? 1 : 0;
}
