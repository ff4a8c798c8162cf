// C++ test of the hits by target through the RAII owners of bio_amd/csrc/sketches.hpp: SearchHits::transpose and ::tally on uploaded
// hits with totals, on the weighted neighbours of counted sets and on folded hits, against a std::stable_sort model of the transpose
// and three counting loops for the table; both tally paths, BSK_TALLY_ADD, re-use and the refusals.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <numeric>
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

// the hits in CSR order, stably sorted by target; a hit's query becomes its target
static Rec transpose_model(const Rec &r, uint64_t nt) {
    const size_t H = r.t.size();
    std::vector<uint32_t> row(H);
    for (size_t q = 0; q + 1 < r.o.size(); ++q)
        for (size_t i = r.o[q]; i < r.o[q + 1]; ++i) row[i] = (uint32_t)q;
    std::vector<size_t> idx(H);
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return r.t[a] < r.t[b]; });
    Rec out;
    out.o.assign(nt + 1, 0);
    for (size_t i : idx) {
        out.o[r.t[i] + 1]++;
        out.t.push_back(row[i]);
        out.s.push_back(r.s[i]);
        if (!r.total.empty()) out.total.push_back(r.total[i]);
        if (!r.members.empty()) out.members.push_back(r.members[i]);
        if (!r.dot.empty()) out.dot.push_back(r.dot[i]), out.msum.push_back(r.msum[i]);
    }
    for (uint64_t t = 0; t < nt; ++t) out.o[t + 1] += out.o[t];
    return out;
}

struct Table {
    std::vector<uint64_t> rows, unique, shared;
    bool operator==(const Table &x) const { return rows == x.rows && unique == x.unique && shared == x.shared; }
};
static void tally_model(const Rec &r, Table &tb) {  // adds to tb
    for (size_t q = 0; q + 1 < r.o.size(); ++q)
        for (size_t i = r.o[q]; i < r.o[q + 1]; ++i) {
            tb.rows[r.t[i]]++;
            tb.shared[r.t[i]] += r.s[i];
            if (r.o[q + 1] - r.o[q] == 1) tb.unique[r.t[i]]++;
        }
}
static Table table(uint64_t nt) { return Table{std::vector<uint64_t>(nt, 0), std::vector<uint64_t>(nt, 0), std::vector<uint64_t>(nt, 0)}; }
static Table fetch_table(Engine &e, const Tally &t) {
    Table tb;
    CHECK(t.fetch(e, tb.rows, tb.unique, tb.shared) == BSK_OK);
    return tb;
}

int main() {
    Engine e(0);
    std::mt19937_64 rng(0x7A11E5);
    // hits with totals over 3 000 targets, rows of 0 .. 1 100 hits; target 7 is named by most rows
    Rec host;
    const size_t lens[] = {0, 1, 1, 2, 15, 16, 17, 64, 65, 300, 1024, 1100, 7, 1, 0};
    for (size_t c : lens) {
        std::vector<uint32_t> pool(3000);
        for (uint32_t i = 0; i < 3000; ++i) pool[i] = i;
        std::shuffle(pool.begin(), pool.end(), rng);
        if (c > 1) *std::find(pool.begin(), pool.end(), 7u) = pool[0], pool[0] = 7;
        std::sort(pool.begin(), pool.begin() + c);
        for (size_t i = 0; i < c; ++i) {
            const uint32_t s = 1 + rng() % 5;
            host.t.push_back(pool[i]);
            host.s.push_back(s);
            host.total.push_back(s * (2 + rng() % 3));
        }
        host.o.push_back(host.t.size());
    }
    const uint64_t nq = host.o.size() - 1;
    SearchHits h, out, back;
    CHECK(h.from_host(e, host.o, host.t, host.s, host.total) == BSK_OK);
    for (uint64_t nt : {3000ull, 3001ull, 4096ull, 70000ull}) {
        CHECK(h.transpose(e, nt, out) == BSK_OK);
        CHECK(fetch_all(e, out) == transpose_model(host, nt));
        CHECK(out.large_queries() == 0);
        CHECK(out.transpose(e, nq, back) == BSK_OK && fetch_all(e, back) == host);  // ascending rows: an involution
    }
    // the table on both paths: 3 000 targets go to global memory, the same hits folded into 1 000 and 2 048 groups stay in LDS
    Tally tl;
    {
        CHECK(h.tally(e, 3000, false, tl) == BSK_OK);
        Table want = table(3000);
        tally_model(host, want);
        CHECK(fetch_table(e, tl) == want && tl.plan().find("global") != std::string::npos);
        CHECK(tl.n_targets() == 3000 && tl.queries() == nq && tl.hits() == host.t.size() && tl.calls() == 1);
        CHECK(h.transpose(e, 3000, out) == BSK_OK);
        const Rec tr = fetch_all(e, out);
        for (uint64_t t = 0; t < 3000; ++t) CHECK(want.rows[t] == tr.o[t + 1] - tr.o[t]);  // the two entries agree with each other
    }
    Rec plain = host;
    plain.total.clear();
    SearchHits hp, folded;
    CHECK(hp.from_host(e, plain.o, plain.t, plain.s) == BSK_OK);
    std::vector<uint64_t> go;
    for (uint64_t g = 0; g <= 3000; g += 3) go.push_back(g);
    CHECK(hp.fold(e, go, nullptr, folded) == BSK_OK);
    const Rec frec = fetch_all(e, folded);
    CHECK(!frec.members.empty());
    for (uint64_t nt : {1000ull, 2048ull, 2049ull}) {
        CHECK(folded.tally(e, nt, false, tl) == BSK_OK);  // re-used: overwritten
        Table want = table(nt);
        tally_model(frec, want);
        CHECK(fetch_table(e, tl) == want && (tl.plan().find("lds") != std::string::npos) == (nt <= 2048) && tl.calls() == 1);
    }
    CHECK(folded.transpose(e, 1000, out) == BSK_OK && fetch_all(e, out) == transpose_model(frec, 1000) && out.members_device() != nullptr);
    CHECK(out.totals_device() == nullptr);  // the flags of the input, whatever the object held before
    // BSK_TALLY_ADD: three batches into one table
    {
        Tally sum;
        Table want = table(3000);
        CHECK(h.tally(e, 3000, true, sum) == BSK_OK && hp.tally(e, 3000, true, sum) == BSK_OK && folded.tally(e, 3000, true, sum) == BSK_OK);
        tally_model(host, want), tally_model(plain, want), tally_model(frec, want);
        CHECK(fetch_table(e, sum) == want && sum.calls() == 3 && sum.queries() == 3 * nq && sum.hits() == 2 * host.t.size() + frec.t.size());
        bsk_tally *held = sum.get();
        CHECK(h.tally(e, 3001, true, sum) == BSK_ERR_ARG && sum.get() == held);   // a table of another n_targets
        CHECK(h.tally(e, 3000, true, sum) == BSK_OK);
        CHECK(hp.tally(e, 7, false, sum) == BSK_ERR_ARG && sum.get() == held);     // a target >= n_targets (most rows name target 7)
        tally_model(host, want);
        CHECK(fetch_table(e, sum) == want && sum.calls() == 4);
        CHECK(bsk_hits_tally(e.ctx(), h.get(), 3000, 2, &sum.handle()) == BSK_ERR_ARG && sum.get() == held);  // a flag bit
        CHECK(fetch_table(e, sum) == want);  // kept means intact
        uint64_t one = 0;
        CHECK(bsk_tally_fetch(e.ctx(), sum.get(), 2999, 1, &one, nullptr, nullptr) == BSK_OK && one == want.rows[2999]);
        CHECK(bsk_tally_fetch(e.ctx(), sum.get(), 2999, 2, &one, nullptr, nullptr) == BSK_ERR_ARG);
    }
    // weighted neighbours of counted sets: totals and weights travel, and the transpose of a symmetric result is the result
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
    CHECK(nb.transpose(e, 60, out) == BSK_OK && fetch_all(e, out) == transpose_model(nrec, 60) && fetch_all(e, out) == nrec);
    // a top-n result has unordered rows: legal input
    SearchHits top;
    CHECK(nb.top_by(e, bsk_measure{BSK_MEASURE_DOT, 0, nullptr, 0, nullptr, 0}, 3, top) == BSK_OK);
    CHECK(top.transpose(e, 60, out) == BSK_OK && fetch_all(e, out) == transpose_model(fetch_all(e, top), 60));
    // empties
    SearchHits none, empty;
    CHECK(none.from_host(e, {0, 0, 0}, {}, {}) == BSK_OK);
    CHECK(none.transpose(e, 5, empty) == BSK_OK && fetch_all(e, empty).o == std::vector<uint64_t>(6, 0));
    CHECK(none.transpose(e, 0, empty) == BSK_OK && fetch_all(e, empty).o == std::vector<uint64_t>(1, 0));
    CHECK(none.tally(e, 5, false, tl) == BSK_OK && fetch_table(e, tl) == table(5) && tl.queries() == 2);
    // the refusals keep the slot and what it holds
    CHECK(h.transpose(e, 3000, out) == BSK_OK);
    bsk_hits *held = out.get();
    const Rec before = fetch_all(e, out);
    CHECK(h.transpose(e, 7, out) == BSK_ERR_ARG && out.get() == held);           // a target >= n_targets
    CHECK(out.transpose(e, 3000, out) == BSK_ERR_ARG && out.get() == held);      // *out == h
    CHECK(h.transpose(e, 1ull << 32, out) == BSK_ERR_UNSUPPORTED && out.get() == held);
    CHECK(bsk_hits_transpose(e.ctx(), nullptr, 3000, &out.handle()) == BSK_ERR_ARG && out.get() == held);
    CHECK(fetch_all(e, out) == before);  // kept means intact

    if (fails) {
        std::printf("%d C++ transpose checks FAILED\n", fails);
        return 1;
    }
    std::printf("all C++ transpose checks passed\n");
    return 0;
}
