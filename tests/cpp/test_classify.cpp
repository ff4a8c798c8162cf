// C++ test of the read classification route through bio_amd/csrc/sketches.hpp: an index searched through an attached handle of a second
// engine (the owner released first), the n best hits of every query, and the pipeline's hits sink -- all against a host-side count over
// sets made on the host from the tuples Engine::run fetched, so nothing of the device-side reduction is taken on trust.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
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
    size_t n() const { return offsets.size() - 1; }
};

// per-sequence sets of a batch: the distinct hash values of every sequence's tuples, ascending
static Collection host_sets(Engine &e, const std::vector<std::string> &seqs, const bsk_params &p) {
    std::vector<std::string_view> v(seqs.begin(), seqs.end());
    Result r;
    CHECK(e.run(v, false, p, r) == BSK_OK);
    Collection c;
    for (size_t i = 0; i < seqs.size(); ++i) {
        std::vector<uint64_t> s(r.hash.begin() + r.offsets[i], r.hash.begin() + r.offsets[i + 1]);
        std::sort(s.begin(), s.end());
        s.erase(std::unique(s.begin(), s.end()), s.end());
        c.values.insert(c.values.end(), s.begin(), s.end());
        c.offsets.push_back(c.values.size());
    }
    return c;
}

// every query's hits by the contract; top_n != 0: largest shared count first, ties by ascending target, cut at top_n
static void expected(const Collection &tg, const Collection &q, uint32_t min_shared, uint32_t top_n, std::vector<uint64_t> &offs, std::vector<uint32_t> &tgt,
                     std::vector<uint32_t> &sh) {
    std::unordered_map<uint64_t, std::vector<uint32_t>> post;
    for (size_t t = 0; t < tg.n(); ++t)
        for (uint64_t i = tg.offsets[t]; i < tg.offsets[t + 1]; ++i) post[tg.values[i]].push_back((uint32_t)t);
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
        std::vector<std::pair<uint32_t, uint32_t>> hits;
        for (auto &h : count)
            if (h.second >= min_shared) hits.push_back(h);
        std::sort(hits.begin(), hits.end(), [&](const auto &a, const auto &b) {
            if (top_n && a.second != b.second) return a.second > b.second;
            return a.first < b.first;
        });
        if (top_n && hits.size() > top_n) hits.resize(top_n);
        for (auto &h : hits) {
            tgt.push_back(h.first);
            sh.push_back(h.second);
        }
        offs.push_back(tgt.size());
    }
}

int main() {
    std::mt19937_64 rng(0xC1A551F);
    const char acgt[] = "ACGT";
    // 20 targets of 3 000 bases; targets 2k and 2k + 1 share their first half, so reads from there hit both
    std::vector<std::string> genomes(20);
    for (size_t g = 0; g < genomes.size(); ++g) {
        std::string s(3000, 'A');
        for (auto &ch : s) ch = acgt[rng() & 3];
        if (g & 1) s.replace(0, 1500, genomes[g - 1], 0, 1500);
        genomes[g] = s;
    }
    // 700 reads of 150 bases from the targets, a few bases changed; some shorter than k, some with an N, some random
    std::vector<std::string> reads;
    for (int i = 0; i < 700; ++i) {
        const std::string &g = genomes[rng() % genomes.size()];
        std::string r = g.substr(rng() % (g.size() - 150), 150);
        for (int m = 0; m < 3; ++m) r[rng() % r.size()] = acgt[rng() & 3];
        if (i % 50 == 7) r.resize(10);
        if (i % 50 == 9) r[70] = 'N';
        if (i % 50 == 11)
            for (auto &ch : r) ch = acgt[rng() & 3];
        reads.push_back(r);
    }
    bsk_params p{};
    p.kind = BSK_MINIMIZER;
    p.k = 15;
    p.w = 5;
    p.canonical = 1;
    p.codon_table = 1;
    p.frame = 1;

    Engine owner(0), other(0);
    const Collection tg = host_sets(owner, genomes, p), qs = host_sets(owner, reads, p);
    DeviceSets dt, dq;
    CHECK(dt.from_host(owner, tg.offsets, tg.values) == BSK_OK);
    SearchIndex ix, handle;
    CHECK(ix.build(owner, dt) == BSK_OK);
    CHECK(ix.attach(other, handle) == BSK_OK);
    uint64_t a[5], b[5];
    CHECK(bsk_index_info(ix.get(), a, a + 1, a + 2, a + 3, a + 4) == BSK_OK && bsk_index_info(handle.get(), b, b + 1, b + 2, b + 3, b + 4) == BSK_OK);
    CHECK(std::equal(a, a + 5, b));
    // a handle belongs to the context it was attached to
    CHECK(dq.from_host(other, qs.offsets, qs.values) == BSK_OK);
    SearchHits hits, top;
    const bsk_search_params sp{2, 0, 0.0, 0.0};
    CHECK(ix.search(other, dq, sp, hits) == BSK_ERR_ARG);

    std::vector<uint64_t> o, eo;
    std::vector<uint32_t> t, s, et, es;
    for (const uint32_t top_n : {0u, 1u, 3u}) {
        expected(tg, qs, sp.min_shared, top_n, eo, et, es);
        // the attached handle, searched on the second engine
        CHECK(handle.search(other, dq, sp, hits) == BSK_OK);
        if (top_n) CHECK(hits.top(other, top_n, top) == BSK_OK);
        CHECK((top_n ? top : hits).fetch(other, o, t, s) == BSK_OK);
        CHECK(o == eo && t == et && s == es);
        // the pipeline: two workers on device 0, chunks of 128 reads
        std::string bytes;
        std::vector<uint64_t> roff{0};
        for (auto &r : reads) {
            bytes += r;
            roff.push_back(bytes.size());
        }
        std::vector<uint64_t> po{0};
        std::vector<uint32_t> pt, ps;
        uint64_t next_record = 0, link = 0;
        bsk_pipeline_stats st{};
        const int rc = classify_memory({0, 0}, 1, 128, 1, (const uint8_t *)bytes.data(), roff.data(), reads.size(), p, ix, sp, top_n,
                                       [&](const HitsChunk &hc) {
                                           CHECK(hc.c->first_record == next_record && hc.c->hash == nullptr);
                                           next_record += hc.c->n_records;
                                           for (uint64_t i = 0; i < hc.c->n_records; ++i) po.push_back(pt.size() + hc.offset(i + 1));
                                           pt.insert(pt.end(), hc.target, hc.target + hc.c->n_values);
                                           ps.insert(ps.end(), hc.shared, hc.shared + hc.c->n_values);
                                           CHECK(hc.c->link_bytes == hc.c->n_records * 5 + hc.c->n_values * 8);
                                           link += hc.c->link_bytes;
                                       },
                                       &st);
        CHECK(rc == BSK_OK);
        CHECK(st.records == reads.size() && st.chunks == (reads.size() + 127) / 128);
        CHECK(po == eo && pt == et && ps == es);
        std::printf("top_n %u: %zu hits (expected %zu), pipeline %zu hits in %llu chunks, %llu bytes down\n", top_n, t.size(), et.size(), pt.size(),
                    (unsigned long long)st.chunks, (unsigned long long)link);
        if (top_n == 0) {  // the owner goes first; the handle keeps the device arrays
            ix = SearchIndex();
            CHECK(handle.attach(owner, ix) == BSK_OK);  // and a handle attaches from a handle
        }
    }
    CHECK(et.size() > 300);  // (the case is not empty)
    CHECK(hits.top(other, 0, top) == BSK_ERR_ARG);
    const bsk_chunk none{};
    const uint32_t *x = nullptr;
    CHECK(bsk_chunk_hits(&none, &x, &x) == BSK_ERR_ARG);
    std::printf(fails ? "FAILED %d checks\n" : "all C++ classify checks passed\n", fails);
    return fails ? 1 : 0;
}
