// C++ test of the abundance-weighted entries through the RAII owners of bio_amd/csrc/sketches.hpp: SetsCompare::compare_counted and
// fetch_weights against a std::map walk -- random counted sets around the window size, a rectangular matrix of more than one tile, a == b,
// an uncounted operand, counts that saturate the sum of products -- DeviceSets::sumsq, and the object's rules: a plain compare into a
// weighted object leaves it unweighted, a refused call leaves it as it was.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
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

using Counted = std::map<uint64_t, uint32_t>;  // value -> count, ascending
struct Collection {
    std::vector<uint64_t> offsets{0}, values;
    std::vector<uint32_t> counts;
    std::vector<Counted> sets;
    void add(const Counted &s) {
        for (const auto &vc : s) {
            values.push_back(vc.first);
            counts.push_back(vc.second);
        }
        offsets.push_back(values.size());
        sets.push_back(s);
    }
    size_t n() const { return offsets.size() - 1; }
};

struct Cell {
    uint32_t shared = 0, total = 0;
    uint64_t dot = 0, min_sum = 0;
};

// the walk: the first `limit` values of the union (0: all); over those both hold, the products summed (saturating) and the minima
static Cell walk(const Counted &a, const Counted &b, uint64_t limit, bool a_counted, bool b_counted) {
    Counted u = a;
    for (const auto &vc : b) u.insert(vc);
    Cell c;
    for (const auto &vc : u) {
        if (limit && c.total >= limit) break;
        ++c.total;
        const auto ia = a.find(vc.first), ib = b.find(vc.first);
        if (ia == a.end() || ib == b.end()) continue;
        const uint64_t ca = a_counted ? ia->second : 1, cb = b_counted ? ib->second : 1, p = ca * cb;
        ++c.shared;
        c.dot = c.dot + p < p ? ~0ull : c.dot + p;
        c.min_sum += std::min(ca, cb);
    }
    return c;
}

static Counted random_set(std::mt19937_64 &rng, size_t n, uint64_t pool, uint32_t max_count) {
    Counted s;
    while (s.size() < n) s[rng() % pool * 0x9E3779B97F4A7C15ull] = (uint32_t)(1 + rng() % max_count);
    return s;
}

static void check_compare(Engine &e, SetsCompare &cmp, const DeviceSets &da, const Collection &a, const DeviceSets &db, const Collection &b, uint64_t limit) {
    CHECK(cmp.compare_counted(e, da, db, limit) == BSK_OK && cmp.weighted());
    uint64_t na = 0, nb = 0, lim = 99;
    CHECK(cmp.info(na, nb, lim) == BSK_OK && na == a.n() && nb == b.n() && lim == limit);
    std::vector<uint32_t> sh, tt;
    std::vector<uint64_t> dt, ms;
    CHECK(cmp.fetch(e, sh, tt) == BSK_OK && sh.size() == a.n() * b.n() && tt.size() == sh.size());
    CHECK(cmp.fetch_weights(e, dt, ms) == BSK_OK && dt.size() == sh.size() && ms.size() == sh.size());
    size_t bad = 0;
    for (size_t i = 0; i < a.n(); ++i)
        for (size_t j = 0; j < b.n(); ++j) {
            const Cell c = walk(a.sets[i], b.sets[j], limit, da.counted(), db.counted());
            const size_t k = i * b.n() + j;
            if (sh[k] != c.shared || tt[k] != c.total || dt[k] != c.dot || ms[k] != c.min_sum) ++bad;
        }
    CHECK(bad == 0);
    uint64_t fig[3] = {0, 0, 0};
    const std::string plan = cmp.plan(fig);
    CHECK(plan.find("k_cmp_tile_w") != std::string::npos && plan.find("bsk_sets_compare_counted") == 0);
    CHECK(fig[0] == ((a.n() + 15) / 16) * ((b.n() + 15) / 16) && fig[1] >= fig[0] && fig[2] >= 1 && fig[2] <= fig[1]);
}

int main() {
    Engine e(0);
    std::mt19937_64 rng(20254);
    Collection a, b;
    for (int i = 0; i < 37; ++i) a.add(random_set(rng, i == 5 ? 0 : 1 + rng() % 400, 1500, 9));
    for (int j = 0; j < 21; ++j) b.add(random_set(rng, j == 2 ? 0 : 1 + rng() % 400, 1500, 1000));
    DeviceSets da, db, plain_b;
    CHECK(da.from_host_counted(e, a.offsets, a.values, a.counts) == BSK_OK);
    CHECK(db.from_host_counted(e, b.offsets, b.values, b.counts) == BSK_OK);
    CHECK(plain_b.from_host(e, b.offsets, b.values) == BSK_OK);

    SetsCompare cmp;  // re-used through every call
    for (uint64_t limit : {0ull, 1ull, 2ull, 100ull, 128ull, 129ull, 500ull, 100000ull}) check_compare(e, cmp, da, a, db, b, limit);
    check_compare(e, cmp, da, a, plain_b, b, 0);   // an uncounted operand counts 1
    check_compare(e, cmp, plain_b, b, da, a, 77);
    check_compare(e, cmp, da, a, da, a, 0);        // a == b
    check_compare(e, cmp, da, a, da, a, 64);

    // a == b at limit 0: the diagonal's dot is sumsq, its min_sum the totals
    CHECK(cmp.compare_counted(e, da, da, 0) == BSK_OK);
    std::vector<uint64_t> dt, ms, q, t;
    CHECK(cmp.fetch_weights(e, dt, ms) == BSK_OK && da.sumsq(e, q) == BSK_OK && da.totals(e, t) == BSK_OK && q.size() == a.n() && t.size() == a.n());
    for (size_t i = 0; i < a.n(); ++i) {
        uint64_t want = 0;
        for (const auto &vc : a.sets[i]) want += (uint64_t)vc.second * vc.second;
        CHECK(q[i] == want && dt[i * a.n() + i] == q[i] && ms[i * a.n() + i] == t[i]);
    }
    std::vector<uint64_t> sizes;
    CHECK(plain_b.sumsq(e, sizes) == BSK_OK && sizes.size() == b.n());
    for (size_t j = 0; j < b.n(); ++j) CHECK(sizes[j] == b.sets[j].size());

    // saturation: two shared values of count 2^32 - 1 on both sides
    const uint32_t M = 0xFFFFFFFFu;
    Collection sa, sb;
    sa.add({{10, M}, {20, M}});
    sb.add({{10, M}});
    sb.add({{10, M}, {20, M}});
    sb.add({{10, M}, {20, 1}});
    DeviceSets dsa, dsb;
    CHECK(dsa.from_host_counted(e, sa.offsets, sa.values, sa.counts) == BSK_OK && dsb.from_host_counted(e, sb.offsets, sb.values, sb.counts) == BSK_OK);
    check_compare(e, cmp, dsa, sa, dsb, sb, 0);
    CHECK(cmp.fetch_weights(e, dt, ms) == BSK_OK && dt.size() == 3);
    CHECK(dt[0] == (uint64_t)M * M && dt[1] == ~0ull && dt[2] == (uint64_t)M * M + M && ms[0] == M && ms[1] == 2ull * M && ms[2] == (uint64_t)M + 1);
    CHECK(dsa.sumsq(e, q) == BSK_OK && q.size() == 1 && q[0] == ~0ull);

    // the object's rules: a plain compare leaves it unweighted (arrays kept), a refused call leaves it as it was
    std::vector<uint32_t> sh, tt, sh2, tt2;
    CHECK(cmp.compare_counted(e, da, db, 50) == BSK_OK && cmp.fetch(e, sh, tt) == BSK_OK);
    bsk_compare *before = cmp.get();
    CHECK(cmp.compare(e, da, db, 50) == BSK_OK && cmp.get() == before && !cmp.weighted());
    CHECK(cmp.fetch_weights(e, dt, ms) == BSK_ERR_ARG);
    CHECK(cmp.fetch(e, sh2, tt2) == BSK_OK && sh == sh2 && tt == tt2 && !sh.empty());
    const uint64_t *pd = &dt[0], *pm = &ms[0];
    CHECK(bsk_compare_weights_device(cmp.get(), &pd, &pm) == BSK_OK && pd == nullptr && pm == nullptr);
    CHECK(cmp.compare_counted(e, da, db, 50) == BSK_OK && cmp.get() == before && cmp.weighted());
    DeviceSets none;
    CHECK(cmp.compare_counted(e, da, none, 0) == BSK_ERR_ARG && cmp.get() == before && cmp.weighted());
    std::vector<uint64_t> cell(4);
    CHECK(bsk_compare_fetch_weights(e.ctx(), cmp.get(), 0, a.n() + 1, cell.data(), nullptr, 1u << 30) == BSK_ERR_ARG);
    CHECK(bsk_compare_fetch_weights(e.ctx(), cmp.get(), 1, 1, cell.data(), nullptr, b.n() - 1) == BSK_ERR_ARG);
    CHECK(bsk_compare_weights_device(cmp.get(), &pd, &pm) == BSK_OK && pd != nullptr && pm != nullptr && pd != pm);

    std::printf(fails ? "FAILED %d checks\n" : "all C++ weighted compare checks passed\n", fails);
    return fails ? 1 : 0;
}
