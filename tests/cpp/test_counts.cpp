// C++ test of the counted sets through the RAII owners of bio_amd/csrc/sketches.hpp: DeviceSets::from_result_counted on a few hundred
// reads against a std::map count of the result's own tuples (per sequence and whole batch, with a scale), op_counted / filter_counts /
// totals against the same maps, one tiled pair, and the owners' argument rules.
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

using Counted = std::map<uint64_t, uint64_t>;
struct Collection {
    std::vector<uint64_t> offsets{0}, values;
    std::vector<uint32_t> counts;
    void add(const Counted &m) {
        for (auto &kv : m) {
            values.push_back(kv.first);
            counts.push_back((uint32_t)std::min<uint64_t>(kv.second, 0xffffffffull));
        }
        offsets.push_back(values.size());
    }
    size_t n() const { return offsets.size() - 1; }
    Counted set(size_t i) const {
        Counted m;
        for (uint64_t j = offsets[i]; j < offsets[i + 1]; ++j) m[values[j]] = counts[j];
        return m;
    }
};

static Counted expected(const Counted &a, const Counted &b, int op) {
    Counted r;
    if (op == BSK_COUNTOP_ADD) {
        r = a;
        for (auto &kv : b) r[kv.first] += kv.second;
    } else {
        for (auto &kv : a)
            if ((b.count(kv.first) != 0) == (op == BSK_COUNTOP_KEEP)) r[kv.first] = kv.second;
    }
    return r;
}

static bool equals(Engine &e, const DeviceSets &s, const Collection &want) {
    std::vector<uint64_t> o, v, t;
    std::vector<uint32_t> c;
    if (s.fetch(e, o, v) != BSK_OK || s.fetch_counts(e, c) != BSK_OK || s.totals(e, t) != BSK_OK || !s.counted()) return false;
    if (o != want.offsets || v != want.values || c != want.counts || t.size() != want.n()) return false;
    for (size_t i = 0; i < want.n(); ++i) {
        uint64_t sum = 0;
        for (uint64_t j = want.offsets[i]; j < want.offsets[i + 1]; ++j) sum += want.counts[j];
        if (t[i] != sum) return false;
    }
    return true;
}

// every op of a x b (either of one set: broadcast) into `out`
static void check_ops(Engine &e, const Collection &a, const Collection &b, DeviceSets &out, uint64_t paths[3]) {
    DeviceSets da, db;
    CHECK(da.from_host_counted(e, a.offsets, a.values, a.counts) == BSK_OK);
    CHECK(db.from_host_counted(e, b.offsets, b.values, b.counts) == BSK_OK);
    const size_t n = std::max(a.n(), b.n());
    for (int op = BSK_COUNTOP_ADD; op <= BSK_COUNTOP_DROP; ++op) {
        CHECK(out.op_counted(e, da, db, op) == BSK_OK);
        Collection want;
        for (size_t i = 0; i < n; ++i) want.add(expected(a.set(a.n() == n ? i : 0), b.set(b.n() == n ? i : 0), op));
        CHECK(equals(e, out, want));
    }
    out.paths(paths);
}

int main() {
    Engine e(0);
    std::mt19937_64 rng(20252);
    // 300 reads of 30 .. 400 bases over a small alphabet of motifs, so that k-mers repeat inside and across reads
    std::vector<std::string> motifs(24);
    for (auto &m : motifs)
        for (int i = 0; i < 12; ++i) m += "ACGT"[rng() % 4];
    std::string bytes;
    std::vector<uint64_t> offs{0};
    for (int r = 0; r < 300; ++r) {
        const size_t len = 30 + rng() % 371;
        std::string s;
        while (s.size() < len) s += motifs[rng() % motifs.size()];
        bytes += s.substr(0, len);
        offs.push_back(bytes.size());
    }
    bsk_batch *batch = nullptr;
    bsk_result *res = nullptr;
    CHECK(bsk_batch_from_ascii(e.ctx(), (const uint8_t *)bytes.data(), offs.data(), 300, BSK_ALPHA_DNA, &batch) == BSK_OK);
    bsk_params p{};
    p.kind = BSK_KMER;
    p.k = 11;
    p.canonical = 1;
    CHECK(bsk_sketch(e.ctx(), batch, &p, &res) == BSK_OK);
    uint64_t n = 0, nt = 0;
    int hp = 0;
    CHECK(bsk_result_info(res, &n, &nt, &hp) == BSK_OK && n == 300 && nt > 20000);
    std::vector<uint64_t> ro(n + 1), hash(nt + 1);
    std::vector<uint8_t> status(n + 1);
    CHECK(bsk_result_fetch(e.ctx(), res, 0, n, ro.data(), status.data(), hash.data(), nullptr, nt + 1) == BSK_OK);

    DeviceSets per, whole;  // re-used through every scale
    Collection per1, whole1;
    for (int scale : {1, 3}) {
        const uint64_t maxhash = scale > 1 ? ~0ULL / (uint64_t)scale : ~0ULL;
        Collection wp, ww;
        Counted all;
        for (uint64_t r = 0; r < n; ++r) {
            Counted m;
            for (uint64_t j = ro[r]; j < ro[r + 1]; ++j)
                if (hash[j] <= maxhash) {
                    ++m[hash[j]];
                    ++all[hash[j]];
                }
            wp.add(m);
        }
        ww.add(all);
        CHECK(per.from_result_counted(e, res, BSK_SETS_PER_SEQUENCE, scale) == BSK_OK);
        CHECK(whole.from_result_counted(e, res, BSK_SETS_WHOLE_BATCH, scale) == BSK_OK);
        CHECK(equals(e, per, wp));
        CHECK(equals(e, whole, ww));
        if (scale == 1) {
            per1 = wp;
            whole1 = ww;
        }
    }
    CHECK(*std::max_element(whole1.counts.begin(), whole1.counts.end()) > 100);
    std::printf("300 reads: %zu distinct 11-mers, the most frequent %u times\n", whole1.values.size(), *std::max_element(whole1.counts.begin(), whole1.counts.end()));

    DeviceSets out;
    uint64_t paths[3];
    // read i against read i + 1 (pairwise), every read against the batch (b broadcast), the batch against every read (a broadcast)
    Collection shifted;
    for (size_t i = 0; i < per1.n(); ++i) shifted.add(per1.set((i + 1) % per1.n()));
    check_ops(e, per1, shifted, out, paths);
    CHECK(paths[0] + paths[1] + paths[2] == 300 && paths[1] + paths[2] > 0);
    check_ops(e, per1, whole1, out, paths);
    CHECK(paths[0] + paths[1] + paths[2] == 300);
    check_ops(e, whole1, per1, out, paths);
    CHECK(paths[0] + paths[1] + paths[2] == 300);

    // one tiled pair, half of its values shared
    std::vector<uint64_t> big(60000);
    for (auto &v : big) v = rng() >> 20;
    Collection ta, tb;
    Counted ma, mb;
    for (size_t i = 0; i < 40000; ++i) ma[big[i]] += 1 + i % 7;
    for (size_t i = 20000; i < 60000; ++i) mb[big[i]] += 1000 * (1 + i % 5);
    ta.add(ma);
    tb.add(mb);
    check_ops(e, ta, tb, out, paths);
    CHECK(paths[0] == 0 && paths[1] == 0 && paths[2] == 1);

    // filter: the values seen at least twice, then those seen 2 .. 5 times
    const std::pair<uint32_t, uint32_t> bounds_list[] = {{2, 0xffffffffu}, {2, 5}};
    for (auto bounds : bounds_list) {
        CHECK(out.filter_counts(e, whole, bounds.first, bounds.second) == BSK_OK);
        std::vector<uint64_t> o, v;
        std::vector<uint32_t> c;
        CHECK(whole.fetch(e, o, v) == BSK_OK && whole.fetch_counts(e, c) == BSK_OK);
        Counted keep;
        for (size_t i = 0; i < v.size(); ++i)
            if (c[i] >= bounds.first && c[i] <= bounds.second) keep[v[i]] = c[i];
        Collection want;
        want.add(keep);
        CHECK(equals(e, out, want));
    }

    // the owners' rules: a refused call leaves the object as it was; plain sets are not counted
    bsk_sets *before = out.get();
    DeviceSets plain;
    CHECK(plain.from_host(e, per1.offsets, per1.values) == BSK_OK && !plain.counted());
    CHECK(out.op_counted(e, per, whole, 3) == BSK_ERR_ARG && out.get() == before);
    CHECK(out.filter_counts(e, whole, 0, 5) == BSK_ERR_ARG && out.get() == before);
    CHECK(out.filter_counts(e, plain, 1, 5) == BSK_ERR_ARG && out.get() == before);
    CHECK(per.op_counted(e, per, whole, BSK_COUNTOP_ADD) == BSK_ERR_ARG);
    std::vector<uint32_t> c;
    CHECK(plain.fetch_counts(e, c) == BSK_ERR_ARG);
    std::vector<uint64_t> t;
    CHECK(plain.totals(e, t) == BSK_OK && t.size() == 300 && t[0] == per1.offsets[1]);
    Collection zero = per1;
    zero.counts[3] = 0;
    CHECK(plain.from_host_counted(e, zero.offsets, zero.values, zero.counts) == BSK_ERR_ARG && plain.get() == nullptr);

    bsk_result_release(res);
    bsk_batch_destroy(batch);
    std::printf(fails ? "FAILED %d checks\n" : "all C++ counted-set checks passed\n", fails);
    return fails ? 1 : 0;
}
