// C++ test of the hits selected by a measure through the RAII owners of bio_amd/csrc/sketches.hpp: SearchHits::filter and ::top_by on
// uploaded hits with totals, on the weighted neighbours of counted sets and on folded hits, against a std::map model per row that
// evaluates every measure as a fraction of unsigned __int128 and compares by 256-bit cross products (wide_uint.hpp, compiled by the
// host compiler here); re-use and the refusals.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <vector>

#include "sketches.hpp"
#include "wide_uint.hpp"

using namespace sketches;
typedef unsigned __int128 u128;
typedef std::pair<uint64_t, uint64_t> Bound;  // a threshold: numerator, denominator

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                               \
        }                                                          \
    } while (0)

struct Rec {  // hits on the host; a payload the hits do not carry is empty
    std::vector<uint64_t> o{0};
    std::vector<uint32_t> t, s, total, members;
    std::vector<uint64_t> dot, msum;
    bool operator==(const Rec &r) const { return o == r.o && t == r.t && s == r.s && total == r.total && members == r.members && dot == r.dot && msum == r.msum; }
};

static Rec fetch_all(Engine &e, const SearchHits &h) {
    Rec r;
    CHECK(h.fetch(e, r.o, r.t, r.s) == BSK_OK);
    if (h.totals_device()) CHECK(h.fetch_totals(e, r.total) == BSK_OK);
    if (h.weights_device().first) CHECK(h.fetch_weights(e, r.dot, r.msum) == BSK_OK);
    if (h.members_device()) CHECK(h.fetch_members(e, r.members) == BSK_OK);
    return r;
}

struct Frac {
    u128 n, d;
};

// the header's table
static Frac measure_of(const Rec &r, const bsk_measure &m, size_t q, size_t i) {
    const u128 Q = m.qnorm ? m.qnorm[q] : 0, T = m.tnorm ? m.tnorm[r.t[i]] : 0;
    switch (m.kind) {
        case BSK_MEASURE_SHARED: return {r.s[i], 1};
        case BSK_MEASURE_MEMBERS: return {r.members[i], 1};
        case BSK_MEASURE_DOT: return {r.dot[i], 1};
        case BSK_MEASURE_MIN_SUM: return {r.msum[i], 1};
        case BSK_MEASURE_QUERY_COV: return {r.s[i], Q};
        case BSK_MEASURE_TARGET_COV: return {r.s[i], T};
        case BSK_MEASURE_JACCARD: return {r.s[i], r.total.empty() ? Q + T - r.s[i] : (u128)r.total[i]};
        case BSK_MEASURE_COSINE: return {(u128)r.dot[i] * r.dot[i], Q * T};
        case BSK_MEASURE_WEIGHTED_JACCARD: return {r.msum[i], Q + T - r.msum[i]};
        case BSK_MEASURE_BC_SIMILARITY: return {(u128)2 * r.msum[i], Q + T};
        default: return {r.dot[i], Q};
    }
}

static void push(const Rec &r, size_t i, Rec &out) {
    out.t.push_back(r.t[i]);
    out.s.push_back(r.s[i]);
    if (!r.total.empty()) out.total.push_back(r.total[i]);
    if (!r.members.empty()) out.members.push_back(r.members[i]);
    if (!r.dot.empty()) out.dot.push_back(r.dot[i]), out.msum.push_back(r.msum[i]);
}

static Rec filter_model(const Rec &r, const bsk_measure &m, uint64_t num, uint64_t den) {
    const bool sq = m.kind == BSK_MEASURE_COSINE;
    const u128 a = sq ? (u128)den * den : (u128)den, b = sq ? (u128)num * num : (u128)num;
    Rec out;
    for (size_t q = 0; q + 1 < r.o.size(); ++q) {
        for (size_t i = r.o[q]; i < r.o[q + 1]; ++i) {
            const Frac f = measure_of(r, m, q, i);
            if (wide_cmp(wide_mul(f.n, a), wide_mul(b, f.d)) >= 0) push(r, i, out);
        }
        out.o.push_back(out.t.size());
    }
    return out;
}

static Rec top_by_model(const Rec &r, const bsk_measure &m, uint32_t n) {
    Rec out;
    for (size_t q = 0; q + 1 < r.o.size(); ++q) {
        // a row's hits in a std::map ordered by the comparator: the larger measure first, ties by ascending target
        auto better = [&](size_t x, size_t y) {
            const Frac fx = measure_of(r, m, q, x), fy = measure_of(r, m, q, y);
            const int c = wide_cmp(wide_mul(fx.n, fy.d), wide_mul(fy.n, fx.d));
            return c > 0 || (c == 0 && r.t[x] < r.t[y]);
        };
        std::map<size_t, bool, decltype(better)> row(better);
        for (size_t i = r.o[q]; i < r.o[q + 1]; ++i) row[i] = true;
        uint32_t k = 0;
        for (auto it = row.begin(); it != row.end() && k < n; ++it, ++k) push(r, it->first, out);
        out.o.push_back(out.t.size());
    }
    return out;
}

static bsk_measure measure(uint32_t kind, const std::vector<uint64_t> *qn = nullptr, const std::vector<uint64_t> *tn = nullptr) {
    return bsk_measure{kind, 0, qn ? qn->data() : nullptr, qn ? qn->size() : 0, tn ? tn->data() : nullptr, tn ? tn->size() : 0};
}

int main() {
    Engine e(0);
    std::mt19937_64 rng(20271);
    // the wide helper against the compiler's own arithmetic where that suffices
    for (int it = 0; it < 1000; ++it) {
        const uint64_t a = rng(), b = rng(), c = rng() >> (rng() % 64), d = rng() >> (rng() % 64);
        const bsk_u256 p = wide_mul(a, b);
        CHECK(p.w[2] == 0 && p.w[3] == 0 && (((u128)p.w[1] << 64) | p.w[0]) == (u128)a * b);
        const bsk_u256 big = wide_mul(((u128)a << 64) | c, ((u128)b << 64) | d);  // (a 2^64 + c)(b 2^64 + d): the top limbs are those of a b plus carries
        const u128 lowmid = (u128)c * d, cross = (u128)a * d, cross2 = (u128)b * c;
        CHECK(big.w[0] == (uint64_t)lowmid);
        const u128 w1 = (lowmid >> 64) + (uint64_t)cross + (uint64_t)cross2;
        CHECK(big.w[1] == (uint64_t)w1);
        CHECK(wide_frac_cmp(a, 1, a, 1) == 0 && wide_frac_cmp(3, 6, 2, 4) == 0 && wide_frac_cmp(2, 4, 3, 7) > 0);
    }
    // hits with totals, rows of 0 .. 1 100 hits: every path of top_by
    Rec host;
    const size_t lens[] = {0, 1, 15, 16, 17, 64, 65, 300, 1024, 1025, 1100, 7};
    for (size_t c : lens) {
        std::vector<uint32_t> pool(3000);
        for (uint32_t i = 0; i < 3000; ++i) pool[i] = i;
        std::shuffle(pool.begin(), pool.end(), rng);
        std::sort(pool.begin(), pool.begin() + c);
        for (size_t i = 0; i < c; ++i) {
            const uint32_t s = 1 + rng() % 5;
            host.t.push_back(pool[i]);
            host.s.push_back(s);
            host.total.push_back(s * (2 + rng() % 3));  // 2/4 = 3/6
        }
        host.o.push_back(host.t.size());
    }
    SearchHits h, out, out2;
    CHECK(h.from_host(e, host.o, host.t, host.s, host.total) == BSK_OK);
    std::vector<uint64_t> qn(lens[0] + sizeof lens / sizeof *lens), tn(3000);
    for (auto &x : qn) x = 6 + rng() % 5;
    for (auto &x : tn) x = 6 + rng() % 5;
    qn[1] = ~0ULL, tn[host.t[0]] = ~0ULL - 1;  // Q + T passes 64 bits
    Rec plain = host;
    plain.total.clear();
    SearchHits hp;
    CHECK(hp.from_host(e, plain.o, plain.t, plain.s) == BSK_OK);
    for (uint32_t kind : {(uint32_t)BSK_MEASURE_SHARED, (uint32_t)BSK_MEASURE_QUERY_COV, (uint32_t)BSK_MEASURE_TARGET_COV, (uint32_t)BSK_MEASURE_JACCARD}) {
        const bsk_measure m = measure(kind, &qn, &tn);
        const std::pair<const SearchHits *, const Rec *> both[] = {{&h, &host}, {&hp, &plain}};
        for (const auto &[hits, rec] : both) {
            for (uint32_t n : {1u, 3u, 16u, 17u, 2000u}) {
                CHECK(hits->top_by(e, m, n, out) == BSK_OK);
                CHECK(fetch_all(e, out) == top_by_model(*rec, m, n));
            }
            const Bound bounds[] = {{0, 1}, {1, 2}, {1, 3}, {2, 5}, {~0ULL, 1}, {~0ULL, ~0ULL}, {~0ULL - 1, ~0ULL}};
            for (auto [num, den] : bounds) {
                CHECK(hits->filter(e, m, num, den, out) == BSK_OK);
                CHECK(fetch_all(e, out) == filter_model(*rec, m, num, den));
                CHECK(out.filter(e, m, num, den, out2) == BSK_OK && fetch_all(e, out2) == fetch_all(e, out));  // what passed passes again
            }
        }
    }
    {  // top_by by shared is top, with the totals on top of it
        SearchHits top;
        CHECK(h.top(e, 5, top) == BSK_OK && h.top_by(e, measure(BSK_MEASURE_SHARED), 5, out) == BSK_OK);
        Rec a = fetch_all(e, top), b = fetch_all(e, out);
        CHECK(a.o == b.o && a.t == b.t && a.s == b.s && a.total.empty() && b.total.size() == b.t.size());
    }
    // weighted neighbours of counted sets: totals and weights, the norms from the owners
    std::vector<uint64_t> so{0}, sv;
    std::vector<uint32_t> sc;
    for (int i = 0; i < 60; ++i) {
        std::map<uint64_t, uint32_t> set;
        for (int j = 0; j < 14; ++j) set[100 * (i % 6) + rng() % 24] = 1 + rng() % 6;
        for (auto &[v, c] : set) sv.push_back(v), sc.push_back(c);
        so.push_back(sv.size());
    }
    DeviceSets a;
    CHECK(a.from_host_counted(e, so, sv, sc) == BSK_OK);
    SearchHits nb;
    CHECK(a.neighbors_counted(e, a, 0, nullptr, nb) == BSK_OK);
    const Rec nrec = fetch_all(e, nb);
    CHECK(!nrec.dot.empty() && !nrec.total.empty());
    std::vector<uint64_t> sq, tot;
    CHECK(a.sumsq(e, sq) == BSK_OK && a.totals(e, tot) == BSK_OK);
    for (uint32_t kind : {(uint32_t)BSK_MEASURE_DOT, (uint32_t)BSK_MEASURE_MIN_SUM, (uint32_t)BSK_MEASURE_COSINE, (uint32_t)BSK_MEASURE_WEIGHTED_JACCARD,
                          (uint32_t)BSK_MEASURE_BC_SIMILARITY, (uint32_t)BSK_MEASURE_QUERY_MASS, (uint32_t)BSK_MEASURE_JACCARD}) {
        const std::vector<uint64_t> &norm = kind == BSK_MEASURE_COSINE ? sq : tot;
        const bsk_measure m = measure(kind, &norm, &norm);
        for (uint32_t n : {1u, 4u, 100u}) CHECK(nb.top_by(e, m, n, out) == BSK_OK && fetch_all(e, out) == top_by_model(nrec, m, n));
        const Bound bounds[] = {{1, 2}, {9, 10}, {1, 1}, {3, 1}, {~0ULL, ~0ULL - 1}};
        for (auto [num, den] : bounds)
            CHECK(nb.filter(e, m, num, den, out) == BSK_OK && fetch_all(e, out) == filter_model(nrec, m, num, den));
    }
    // folded hits: the best group keeps its members
    std::vector<uint64_t> go;
    for (uint64_t g = 0; g <= 3000; g += 3) go.push_back(g);
    SearchHits folded;
    CHECK(hp.fold(e, go, nullptr, folded) == BSK_OK);
    const Rec frec = fetch_all(e, folded);
    CHECK(!frec.members.empty());
    for (uint32_t n : {1u, 20u}) CHECK(folded.top_by(e, measure(BSK_MEASURE_MEMBERS), n, out) == BSK_OK && fetch_all(e, out) == top_by_model(frec, measure(BSK_MEASURE_MEMBERS), n));
    CHECK(out.members_device() != nullptr);
    CHECK(folded.filter(e, measure(BSK_MEASURE_MEMBERS), 2, 1, out) == BSK_OK && fetch_all(e, out) == filter_model(frec, measure(BSK_MEASURE_MEMBERS), 2, 1));
    // the refusals keep the slot and what it holds
    bsk_hits *held = out.get();
    const Rec before = fetch_all(e, out);
    CHECK(h.filter(e, measure(BSK_MEASURE_MEMBERS), 1, 1, out) == BSK_ERR_ARG && out.get() == held);          // no members
    CHECK(h.filter(e, measure(BSK_MEASURE_COSINE, &qn, &tn), 1, 1, out) == BSK_ERR_ARG && out.get() == held);  // no weights
    CHECK(hp.top_by(e, measure(BSK_MEASURE_JACCARD), 3, out) == BSK_ERR_ARG && out.get() == held);            // no totals, no norms
    CHECK(h.filter(e, measure(BSK_MEASURE_SHARED), 1, 0, out) == BSK_ERR_ARG && out.get() == held);           // min_den == 0
    CHECK(h.top_by(e, measure(BSK_MEASURE_SHARED), 0, out) == BSK_ERR_ARG && out.get() == held);              // n == 0
    CHECK(out.filter(e, measure(BSK_MEASURE_SHARED), 1, 1, out) == BSK_ERR_ARG && out.get() == held);         // *out == h
    std::vector<uint64_t> few(10, 1), zeros(3000, 0);
    CHECK(h.filter(e, measure(BSK_MEASURE_TARGET_COV, nullptr, &few), 1, 1, out) == BSK_ERR_ARG && out.get() == held);    // a target >= n_tnorm
    CHECK(h.top_by(e, measure(BSK_MEASURE_TARGET_COV, nullptr, &zeros), 2, out) == BSK_ERR_ARG && out.get() == held);     // D == 0
    CHECK(h.filter(e, measure(BSK_MEASURE_QUERY_COV, &few, nullptr), 1, 1, out) == BSK_ERR_ARG && out.get() == held);     // n_qnorm != n_queries
    bsk_measure flagged = measure(BSK_MEASURE_SHARED);
    flagged.flags = 2;
    CHECK(h.filter(e, flagged, 1, 1, out) == BSK_ERR_ARG && h.top_by(e, measure(99), 1, out) == BSK_ERR_ARG && out.get() == held);
    CHECK(fetch_all(e, out) == before);  // kept means intact

    if (fails) {
        std::printf("%d C++ select checks FAILED\n", fails);
        return 1;
    }
    std::printf("all C++ select checks passed\n");
    return 0;
}
