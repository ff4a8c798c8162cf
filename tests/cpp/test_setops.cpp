// C++ test of the set algebra through the RAII owners of bio_amd/csrc/sketches.hpp: DeviceSets::op on a few hundred random pairs
// (the values 0 and 2^64-1 included) and one tiled pair against std::set_union / std::set_intersection / std::set_difference /
// std::set_symmetric_difference, DeviceSets::reduce against a std::map count, and the owners' re-use and argument rules.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <iterator>
#include <map>
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
    void add(Set s) {
        std::sort(s.begin(), s.end());
        s.erase(std::unique(s.begin(), s.end()), s.end());
        values.insert(values.end(), s.begin(), s.end());
        offsets.push_back(values.size());
    }
    size_t n() const { return offsets.size() - 1; }
    Set set(size_t i) const { return Set(values.begin() + offsets[i], values.begin() + offsets[i + 1]); }
};

static Set random_set(std::mt19937_64 &rng, const Set &pool, size_t size) {
    Set s(size);
    for (auto &v : s) v = pool[rng() % pool.size()];
    return s;
}

static Set expected(const Set &a, const Set &b, int op) {
    Set r;
    if (op == BSK_SETOP_UNION) std::set_union(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(r));
    else if (op == BSK_SETOP_INTERSECT) std::set_intersection(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(r));
    else if (op == BSK_SETOP_DIFF) std::set_difference(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(r));
    else std::set_symmetric_difference(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(r));
    return r;
}

// every op of a x b (b of one set: broadcast) into `out`, compared set by set; returns the pairs per path of the last op
static void check_ops(Engine &e, const Collection &a, const Collection &b, DeviceSets &out, uint64_t paths[3]) {
    DeviceSets da, db;
    CHECK(da.from_host(e, a.offsets, a.values) == BSK_OK);
    CHECK(db.from_host(e, b.offsets, b.values) == BSK_OK);
    for (int op = BSK_SETOP_UNION; op <= BSK_SETOP_SYMDIFF; ++op) {
        CHECK(out.op(e, da, db, op) == BSK_OK);
        std::vector<uint64_t> o, v;
        CHECK(out.fetch(e, o, v) == BSK_OK);
        Collection want;
        for (size_t i = 0; i < a.n(); ++i) want.add(expected(a.set(i), b.set(b.n() == a.n() ? i : 0), op));
        CHECK(o == want.offsets);
        CHECK(v == want.values);
    }
    out.paths(paths);
}

int main() {
    Engine e(0);
    std::mt19937_64 rng(20251);
    Set pool(4000);
    for (auto &v : pool) v = rng();
    pool[0] = 0;
    pool[1] = ~0ULL;
    DeviceSets out;  // one object for every result: its arrays only grow
    uint64_t paths[3];

    // a few hundred random pairs, sizes from nothing to beyond one wavefront's LDS
    Collection a, b;
    for (int i = 0; i < 400; ++i) {
        const size_t cap = i % 7 == 0 ? 1500 : i % 3 == 0 ? 300 : 24;
        a.add(random_set(rng, pool, rng() % (cap + 1)));
        b.add(random_set(rng, pool, rng() % (cap + 1)));
    }
    check_ops(e, a, b, out, paths);
    CHECK(paths[0] + paths[1] + paths[2] == 400 && paths[0] > 50 && paths[1] > 50 && paths[2] > 5);
    std::printf("400 random pairs: %llu on the group path, %llu on the wave path, %llu tiled\n", (unsigned long long)paths[0], (unsigned long long)paths[1],
                (unsigned long long)paths[2]);

    // one tiled pair, half of its values shared
    Set big(60000);
    for (auto &v : big) v = rng() >> 20;
    Collection ta, tb;
    ta.add(Set(big.begin(), big.begin() + 40000));
    tb.add(Set(big.begin() + 20000, big.end()));
    check_ops(e, ta, tb, out, paths);
    CHECK(paths[0] == 0 && paths[1] == 0 && paths[2] == 1);

    // broadcast: every set of a against b's first set
    Collection one;
    one.add(b.set(7));
    check_ops(e, a, one, out, paths);
    CHECK(paths[0] + paths[1] + paths[2] == 400);

    // reduce: runs of 0..5 consecutive sets, the values of at least m members
    std::vector<uint64_t> go{0};
    while (go.back() < a.n()) go.push_back(std::min<uint64_t>(a.n(), go.back() + rng() % 6));
    DeviceSets da, reduced;
    CHECK(da.from_host(e, a.offsets, a.values) == BSK_OK);
    for (uint32_t m : {1u, 2u, 3u, (uint32_t)BSK_MEMBERS_ALL}) {
        CHECK(reduced.reduce(e, da, go, m) == BSK_OK);
        Collection want;
        for (size_t g = 0; g + 1 < go.size(); ++g) {
            std::map<uint64_t, uint64_t> count;
            for (uint64_t s = go[g]; s < go[g + 1]; ++s)
                for (uint64_t v : a.set(s)) ++count[v];
            const uint64_t need = m == BSK_MEMBERS_ALL ? go[g + 1] - go[g] : m;
            Set keep;
            for (auto &kv : count)
                if (kv.second >= need) keep.push_back(kv.first);
            want.add(keep);
        }
        std::vector<uint64_t> o, v;
        CHECK(reduced.fetch(e, o, v) == BSK_OK);
        CHECK(o == want.offsets);
        CHECK(v == want.values);
        CHECK(reduced.n_sets() == go.size() - 1);
    }

    // the owners' rules: the result object is neither input; a refused call leaves it as it was
    bsk_sets *before = out.get();
    DeviceSets db;
    CHECK(db.from_host(e, b.offsets, b.values) == BSK_OK);
    CHECK(out.op(e, da, db, 7) == BSK_ERR_ARG && out.get() == before);
    CHECK(da.op(e, da, db, BSK_SETOP_UNION) == BSK_ERR_ARG);
    CHECK(out.op(e, da, reduced, BSK_SETOP_UNION) == BSK_ERR_ARG && out.get() == before);  // 400 sets against the groups
    CHECK(out.reduce(e, da, go, 0) == BSK_ERR_ARG && out.get() == before);
    CHECK(out.reduce(e, da, {0, 1}, 1) == BSK_ERR_ARG && out.get() == before);
    std::printf(fails ? "FAILED %d checks\n" : "all C++ set-operation checks passed\n", fails);
    return fails ? 1 : 0;
}
