// C++ test of the window sets and the folded hits through the RAII owners of bio_amd/csrc/sketches.hpp: DeviceSets::from_windows on
// minimizer and ntHash results against a std::map per window built from the fetched tuples by the definition of include/biosketch.h,
// the reduce of a sequence's windows against its own set, SearchHits::fold against a std::map per row, re-use and the refusals.
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

struct Tuples {
    uint64_t n = 0;
    std::vector<uint64_t> offsets, hash;
    std::vector<uint32_t> pos;  // empty: implicit positions
};

struct Model {
    std::vector<uint64_t> seq_offsets{0}, offsets{0}, values;
    std::vector<uint32_t> counts;
};

// the definition, tuple by tuple and window by window
static Model windows_model(const Tuples &t, const bsk_window_params &wp, int scale) {
    const uint64_t maxhash = scale > 1 ? ~0ULL / (uint64_t)scale : ~0ULL;
    Model m;
    for (uint64_t i = 0; i < t.n; ++i) {
        const uint64_t a = t.offsets[i], b = t.offsets[i + 1];
        auto p_of = [&](uint64_t j) -> uint64_t { return t.pos.empty() ? j - a : (uint64_t)(t.pos[j] & BSK_POS_MASK); };
        uint64_t nwin = 0, W = wp.window, S = wp.step ? wp.step : wp.window;
        if (b > a) {
            const uint64_t P = p_of(b - 1);
            if (wp.count) W = S = std::max<uint64_t>(1, (P + wp.count) / wp.count);
            nwin = (P < W ? 0 : (P - W) / S + 1) + 1;
        }
        std::vector<std::map<uint64_t, uint32_t>> wins(nwin);
        for (uint64_t j = a; j < b; ++j) {
            if (t.hash[j] > maxhash) continue;
            const uint64_t p = p_of(j);
            for (uint64_t w = (p < W ? 0 : (p - W) / S + 1); w < nwin && w * S <= p; ++w)  // from first(p) on
                if (p < w * S + W) ++wins[w][t.hash[j]];
        }
        for (auto &w : wins) {
            for (auto &[v, c] : w) {
                m.values.push_back(v);
                m.counts.push_back(c);
            }
            m.offsets.push_back(m.values.size());
        }
        m.seq_offsets.push_back(m.seq_offsets.back() + nwin);
    }
    return m;
}

static bool equals(Engine &e, const DeviceSets &s, const Model &m, bool counted) {
    std::vector<uint64_t> o, v;
    std::vector<uint32_t> c;
    if (s.fetch(e, o, v) != BSK_OK || o != m.offsets || v != m.values || s.counted() != counted) return false;
    return !counted || (s.fetch_counts(e, c) == BSK_OK && c == m.counts);
}

static Tuples sketch(Engine &e, const std::vector<std::string> &reads, const bsk_params &p, bsk_batch *&batch, bsk_result *&res) {
    std::string bytes;
    std::vector<uint64_t> offs{0};
    for (auto &r : reads) {
        bytes += r;
        offs.push_back(bytes.size());
    }
    CHECK(bsk_batch_from_ascii(e.ctx(), (const uint8_t *)bytes.data(), offs.data(), reads.size(), BSK_ALPHA_DNA, &batch) == BSK_OK);
    CHECK(bsk_sketch(e.ctx(), batch, &p, &res) == BSK_OK);
    Tuples t;
    uint64_t nt = 0;
    int hp = 0;
    CHECK(bsk_result_info(res, &t.n, &nt, &hp) == BSK_OK);
    t.offsets.assign(t.n + 1, 0);
    t.hash.assign(nt + 1, 0);
    t.pos.assign(hp ? nt + 1 : 0, 0);
    std::vector<uint8_t> status(t.n + 1);
    CHECK(bsk_result_fetch(e.ctx(), res, 0, t.n, t.offsets.data(), status.data(), t.hash.data(), hp ? t.pos.data() : nullptr, nt + 1) == BSK_OK);
    t.hash.resize(nt);
    if (hp) t.pos.resize(nt);
    return t;
}

struct Folded {
    std::vector<uint64_t> offsets{0};
    std::vector<uint32_t> target, shared, members;
};

static Folded fold_model(const std::vector<uint64_t> &o, const std::vector<uint32_t> &t, const std::vector<uint32_t> &s, const std::vector<uint64_t> &go, const bsk_fold_params &fp) {
    Folded f;
    for (size_t q = 0; q + 1 < o.size(); ++q) {
        std::map<uint32_t, std::pair<uint64_t, uint64_t>> acc;  // group -> (sum, members)
        for (uint64_t i = o[q]; i < o[q + 1]; ++i) {
            const uint32_t g = (uint32_t)(std::upper_bound(go.begin(), go.end(), (uint64_t)t[i]) - go.begin() - 1);
            acc[g].first += s[i];
            acc[g].second += 1;
        }
        for (auto &[g, sm] : acc) {
            const uint64_t size = go[g + 1] - go[g];
            if (sm.second < std::max<uint32_t>(fp.min_members, 1)) continue;
            if (fp.frac_den && sm.second * fp.frac_den < (uint64_t)fp.frac_num * size) continue;
            f.target.push_back(g);
            f.shared.push_back((uint32_t)std::min<uint64_t>(sm.first, 0xFFFFFFFFull));
            f.members.push_back((uint32_t)sm.second);
        }
        f.offsets.push_back(f.target.size());
    }
    return f;
}

static bool equals(Engine &e, const SearchHits &h, const Folded &f) {
    std::vector<uint64_t> o;
    std::vector<uint32_t> t, s, m;
    return h.fetch(e, o, t, s) == BSK_OK && h.fetch_members(e, m) == BSK_OK && o == f.offsets && t == f.target && s == f.shared && m == f.members &&
           h.members_device() != nullptr && h.totals_device() == nullptr;
}

int main() {
    Engine e(0);
    std::mt19937_64 rng(20261);
    auto read = [&](size_t len) {
        std::string s;
        for (size_t i = 0; i < len; ++i) s += "ACGT"[rng() % 4];
        return s;
    };
    std::vector<std::string> reads;
    const size_t lens[6] = {0, 20, 150, 250, 400, 1000};
    for (int i = 0; i < 260; ++i) reads.push_back(read(lens[i % 6]));
    reads.push_back(read(6000));  // with it the minimizer batch is tiled: a wide result

    const bsk_window_params rules[] = {{1, 0, 0, 0}, {7, 1, 0, 0}, {64, 0, 0, 0}, {64, 32, 0, 0}, {64, 63, 0, BSK_WINDOWS_COUNTED}, {1000, 500, 0, 0}, {0x7fffffffu, 0, 0, BSK_WINDOWS_COUNTED},
                                       {0, 0, 1, 0}, {0, 0, 3, BSK_WINDOWS_COUNTED}, {0, 0, 10, 0}, {0, 0, 100000, 0}};
    for (int kind : {BSK_MINIMIZER, BSK_NTHASH}) {
        for (int wide = 0; wide < 2; ++wide) {
            bsk_params p{};
            p.kind = kind;
            p.k = 21;
            p.w = kind == BSK_MINIMIZER ? 11 : 0;
            p.canonical = 1;
            bsk_batch *batch = nullptr;
            bsk_result *res = nullptr;
            std::vector<std::string> rs(reads.begin(), reads.end() - (wide ? 0 : 1));
            const Tuples t = sketch(e, rs, p, batch, res);
            const uint64_t *wf = nullptr, *wc = nullptr;
            const uint64_t *refs = nullptr;
            bsk_result_device(res, &refs, nullptr, nullptr, nullptr);
            bsk_result_device_wide(res, &wf, &wc);
            // (the every-position kinds tile from 512 bases on: their result is wide with or without the long read)
            CHECK(wide || kind == BSK_NTHASH ? (refs == nullptr && wf != nullptr) : refs != nullptr);
            DeviceSets ws, own, back;  // re-used through every rule
            int k = 0;
            for (const auto &wp : rules) {
                const int scale = (k++ % 2) ? 100 : 1;
                const bool counted = (wp.flags & BSK_WINDOWS_COUNTED) != 0;
                const Model m = windows_model(t, wp, scale);
                std::vector<uint64_t> so;
                CHECK(ws.from_windows(e, res, wp, scale, &so) == BSK_OK);
                CHECK(so == m.seq_offsets);
                CHECK(equals(e, ws, m, counted));
                // the union of a sequence's windows is the sequence's own set
                CHECK(bsk_result_sets_reuse(e.ctx(), res, BSK_SETS_PER_SEQUENCE, scale, &own.handle()) == BSK_OK);
                CHECK(back.reduce(e, ws, so, 1) == BSK_OK);
                std::vector<uint64_t> o1, v1, o2, v2;
                CHECK(own.fetch(e, o1, v1) == BSK_OK && back.fetch(e, o2, v2) == BSK_OK && o1 == o2 && v1 == v2);
            }
            // refusals keep the object
            std::vector<uint64_t> o0, v0, o1, v1;
            CHECK(ws.fetch(e, o0, v0) == BSK_OK);
            bsk_sets *held = ws.get();
            for (const bsk_window_params bad : {bsk_window_params{0, 0, 0, 0}, {7, 0, 3, 0}, {7, 8, 0, 0}, {0, 1, 3, 0}, {0x80000000u, 0, 0, 0}, {7, 0, 0, 2}})
                CHECK(ws.from_windows(e, res, bad, 1) == BSK_ERR_ARG && ws.get() == held);
            CHECK(ws.from_windows(e, res, {7, 0, 0, 0}, -1) == BSK_ERR_ARG && ws.get() == held);
            CHECK(ws.fetch(e, o1, v1) == BSK_OK && o0 == o1 && v0 == v1);
            bsk_result_release(res);
            bsk_batch_destroy(batch);
        }
    }

    // folded hits: random rows over 40 targets in groups with empty ones; a long run; saturation; the rules
    const std::vector<uint64_t> go{0, 0, 3, 3, 10, 11, 20, 40, 40};
    std::vector<uint64_t> ho{0};
    std::vector<uint32_t> ht, hs;
    for (int q = 0; q < 300; ++q) {
        for (uint32_t t = 0; t < 40; ++t)
            if (rng() % 3 == 0) {
                ht.push_back(t);
                hs.push_back(1 + (uint32_t)(rng() % 1000));
            }
        ho.push_back(ht.size());
    }
    SearchHits h, f, f2;
    CHECK(h.from_host(e, ho, ht, hs) == BSK_OK);
    for (const bsk_fold_params fp : {bsk_fold_params{0, 0, 0, 0}, {1, 0, 0, 0}, {2, 0, 0, 0}, {1, 0, 1, 1}, {1, 0, 8, 10}, {1, 0, 1, 3}, {3, 0, 1, 3}}) {
        CHECK(h.fold(e, go, &fp, f) == BSK_OK);
        CHECK(equals(e, f, fold_model(ho, ht, hs, go, fp)));
    }
    CHECK(h.fold(e, go, nullptr, f) == BSK_OK && equals(e, f, fold_model(ho, ht, hs, go, bsk_fold_params{1, 0, 0, 0})));
    {  // one row of 5 000 hits into one group and into 5 000 groups; 0xFFFFFFFF + 1 saturates
        std::vector<uint64_t> o{0, 5000}, one{0, 5000}, each(5001);
        std::vector<uint32_t> t(5000), s(5000);
        for (uint32_t i = 0; i < 5000; ++i) t[i] = i, s[i] = 1 + i % 977, each[i + 1] = i + 1;
        SearchHits big;
        CHECK(big.from_host(e, o, t, s) == BSK_OK);
        CHECK(big.fold(e, one, nullptr, f) == BSK_OK && equals(e, f, fold_model(o, t, s, one, bsk_fold_params{1, 0, 0, 0})));
        CHECK(big.fold(e, each, nullptr, f) == BSK_OK && equals(e, f, fold_model(o, t, s, each, bsk_fold_params{1, 0, 0, 0})));
        std::vector<uint32_t> m;
        CHECK(f.fetch_members(e, m) == BSK_OK && m == std::vector<uint32_t>(5000, 1));
        std::vector<uint64_t> o2{0, 2}, g2{0, 2};
        std::vector<uint32_t> t2{0, 1}, s2{0xFFFFFFFFu, 1};
        CHECK(big.from_host(e, o2, t2, s2) == BSK_OK && big.fold(e, g2, nullptr, f) == BSK_OK);
        std::vector<uint64_t> fo;
        std::vector<uint32_t> ft, fs;
        CHECK(f.fetch(e, fo, ft, fs) == BSK_OK && fs == std::vector<uint32_t>{0xFFFFFFFFu});
    }
    // the best group of every row; its output carries no members.  A top() result is refused as input, and so are the other misuses
    CHECK(h.fold(e, go, nullptr, f) == BSK_OK && f.top(e, 1, f2) == BSK_OK && f2.members_device() == nullptr);
    SearchHits top3;
    CHECK(h.top(e, 3, top3) == BSK_OK);
    bsk_hits *held = f.get();
    CHECK(top3.fold(e, go, nullptr, f) == BSK_ERR_ARG && f.get() == held);
    CHECK(h.fold(e, {0, 5, 3, 40}, nullptr, f) == BSK_ERR_ARG && f.get() == held);   // offsets that decrease
    CHECK(h.fold(e, {0, 5, 39}, nullptr, f) == BSK_ERR_ARG && f.get() == held);      // a target beyond the last offset
    CHECK(f.fold(e, go, nullptr, f) == BSK_ERR_ARG && f.get() == held);              // *out == h
    const bsk_fold_params flag{1, 1, 0, 0}, frac{1, 0, 3, 2};
    CHECK(h.fold(e, go, &flag, f) == BSK_ERR_ARG && h.fold(e, go, &frac, f) == BSK_ERR_ARG && f.get() == held);
    CHECK(equals(e, f, fold_model(ho, ht, hs, go, bsk_fold_params{1, 0, 0, 0})));    // kept means intact

    if (fails) {
        std::printf("%d C++ window checks FAILED\n", fails);
        return 1;
    }
    std::printf("all C++ window checks passed\n");
    return 0;
}
