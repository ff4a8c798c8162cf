// C++ test of the MinHash entries through the RAII owners of bio_amd/csrc/sketches.hpp: DeviceSets::bottom against a prefix copy (counts
// included) and SetsCompare::compare against a std::set_union walk -- random sets around the window size, a rectangular matrix of more
// than one tile, a == b, every limit that matters -- and the owners' argument rules.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <iterator>
#include <random>
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
    std::vector<uint32_t> counts;
    void add(const Set &s) {
        for (uint64_t v : s) {
            values.push_back(v);
            counts.push_back((uint32_t)(1 + v % 9));
        }
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

static Set random_set(std::mt19937_64 &rng, size_t n, uint64_t pool) {
    Set s;
    while (s.size() < n) {
        s.push_back(rng() % pool * 0x9E3779B97F4A7C15ull);
        std::sort(s.begin(), s.end());
        s.erase(std::unique(s.begin(), s.end()), s.end());
    }
    return s;
}

static void check_compare(Engine &e, SetsCompare &cmp, const DeviceSets &da, const Collection &a, const DeviceSets &db, const Collection &b, uint64_t limit) {
    CHECK(cmp.compare(e, da, db, limit) == BSK_OK);
    uint64_t na = 0, nb = 0, lim = 99;
    CHECK(cmp.info(na, nb, lim) == BSK_OK && na == a.n() && nb == b.n() && lim == limit);
    std::vector<uint32_t> sh, tt;
    CHECK(cmp.fetch(e, sh, tt) == BSK_OK && sh.size() == a.n() * b.n() && tt.size() == sh.size());
    size_t bad = 0;
    for (size_t i = 0; i < a.n(); ++i)
        for (size_t j = 0; j < b.n(); ++j) {
            uint32_t s = 0, t = 0;
            walk(a.set(i), b.set(j), limit, s, t);
            if (sh[i * b.n() + j] != s || tt[i * b.n() + j] != t) ++bad;
        }
    CHECK(bad == 0);
    uint64_t fig[3] = {0, 0, 0};
    const char *plan = cmp.plan(fig);
    CHECK(std::string(plan).find("k_cmp_tile") != std::string::npos);
    CHECK(fig[0] == ((a.n() + 15) / 16) * ((b.n() + 15) / 16) && fig[1] >= fig[0] && fig[2] >= 1 && fig[2] <= fig[1]);
}

int main() {
    Engine e(0);
    std::mt19937_64 rng(20253);
    Collection a, b;
    for (int i = 0; i < 37; ++i) a.add(random_set(rng, i == 5 ? 0 : 1 + rng() % 400, 1500));
    for (int j = 0; j < 21; ++j) b.add(random_set(rng, j == 2 ? 0 : 1 + rng() % 400, 1500));
    DeviceSets da, db;
    CHECK(da.from_host_counted(e, a.offsets, a.values, a.counts) == BSK_OK);
    CHECK(db.from_host(e, b.offsets, b.values) == BSK_OK);

    SetsCompare cmp;  // re-used through every call
    for (uint64_t limit : {0ull, 1ull, 2ull, 100ull, 128ull, 129ull, 500ull, 100000ull}) check_compare(e, cmp, da, a, db, b, limit);
    check_compare(e, cmp, da, a, da, a, 0);
    check_compare(e, cmp, da, a, da, a, 64);

    // bottom: a prefix of every set, the counts with it; then the identity compare(a, b, n) == compare(bottom(a, n), bottom(b, n), n)
    DeviceSets ba, bb;
    for (uint64_t n : {1ull, 50ull, 1ull << 40}) {
        CHECK(ba.bottom(e, da, n) == BSK_OK && bb.bottom(e, db, n) == BSK_OK);
        CHECK(ba.counted() && !bb.counted());
        Collection want;
        for (size_t i = 0; i < a.n(); ++i) {
            Set s = a.set(i);
            if (s.size() > n) s.resize(n);
            want.add(s);
        }
        std::vector<uint64_t> o, v;
        std::vector<uint32_t> c;
        CHECK(ba.fetch(e, o, v) == BSK_OK && ba.fetch_counts(e, c) == BSK_OK);
        CHECK(o == want.offsets && v == want.values && c == want.counts);
    }
    CHECK(ba.bottom(e, da, 50) == BSK_OK && bb.bottom(e, db, 50) == BSK_OK);
    std::vector<uint32_t> s1, t1, s2, t2;
    SetsCompare cmp2;
    CHECK(cmp.compare(e, da, db, 50) == BSK_OK && cmp.fetch(e, s1, t1) == BSK_OK);
    CHECK(cmp2.compare(e, ba, bb, 50) == BSK_OK && cmp2.fetch(e, s2, t2) == BSK_OK);
    CHECK(s1 == s2 && t1 == t2 && !s1.empty());

    // the owners' rules: a refused call leaves the object as it was
    bsk_sets *before = ba.get();
    CHECK(ba.bottom(e, da, 0) == BSK_ERR_ARG && ba.get() == before);
    CHECK(ba.bottom(e, ba, 5) == BSK_ERR_ARG && ba.get() == before);
    bsk_compare *cbefore = cmp.get();
    DeviceSets none;
    CHECK(cmp.compare(e, da, none, 0) == BSK_ERR_ARG && cmp.get() == cbefore);
    std::vector<uint32_t> cell(4);
    CHECK(bsk_compare_fetch(e.ctx(), cmp.get(), 0, a.n() + 1, cell.data(), nullptr, 1u << 30) == BSK_ERR_ARG);
    CHECK(bsk_compare_fetch(e.ctx(), cmp.get(), 1, 1, cell.data(), nullptr, b.n() - 1) == BSK_ERR_ARG);
    const uint32_t *ds = nullptr, *dt = nullptr;
    cmp.device(ds, dt);
    CHECK(ds != nullptr && dt != nullptr && ds != dt);

    std::printf(fails ? "FAILED %d checks\n" : "all C++ compare checks passed\n", fails);
    return fails ? 1 : 0;
}
