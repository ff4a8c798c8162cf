// C++ test of the merged hits through the RAII owners of bio_amd/csrc/sketches.hpp: SearchHits::merge on uploaded hits with totals, on
// the weighted neighbours of counted sets and on folded hits, against a std::map model -- both paths, BSK_MERGE_ADD with saturation,
// the payloads all parts carry, re-use, a second engine and the refusals.
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

static std::string plan_of(const SearchHits &h) {
    const char *p = "";
    bsk_hits_plan(h.get(), &p, nullptr);
    return p ? p : "";
}

struct Cell {
    uint64_t s = 0, total = 0, members = 0, dot = 0, msum = 0, n = 0;
};
static uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }
static uint32_t sat32(uint64_t x) { return x > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)x; }

// per row a std::map from the shifted target to the sums; *dups: the pairs that occurred more than once
static Rec merge_model(const std::vector<Rec> &parts, const std::vector<uint64_t> &base, uint64_t *dups) {
    bool total = true, members = true, weights = true;
    for (const Rec &r : parts) total &= !r.total.empty() || r.t.empty(), members &= !r.members.empty() || r.t.empty(), weights &= !r.dot.empty() || r.t.empty();
    Rec out;
    *dups = 0;
    for (size_t q = 0; q + 1 < parts[0].o.size(); ++q) {
        std::map<uint64_t, Cell> row;
        for (size_t p = 0; p < parts.size(); ++p) {
            const Rec &r = parts[p];
            for (size_t i = r.o[q]; i < r.o[q + 1]; ++i) {
                Cell &c = row[r.t[i] + (base.empty() ? 0 : base[p])];
                c.s += r.s[i];
                if (total) c.total += r.total[i];
                if (members) c.members += r.members[i];
                if (weights) c.dot = sat_add(c.dot, r.dot[i]), c.msum = sat_add(c.msum, r.msum[i]);
                if (c.n++) ++*dups;
            }
        }
        for (auto &[t, c] : row) {
            out.t.push_back((uint32_t)t);
            out.s.push_back(sat32(c.s));
            if (total) out.total.push_back(sat32(c.total));
            if (members) out.members.push_back(sat32(c.members));
            if (weights) out.dot.push_back(c.dot), out.msum.push_back(c.msum);
        }
        out.o.push_back(out.t.size());
    }
    return out;
}

// rows of the given lengths over `span` targets, ascending, with totals
static Rec random_hits(std::mt19937_64 &rng, const std::vector<size_t> &lens, uint32_t span) {
    Rec r;
    std::vector<uint32_t> pool(span);
    for (uint32_t i = 0; i < span; ++i) pool[i] = i;
    for (size_t c : lens) {
        std::shuffle(pool.begin(), pool.end(), rng);
        std::sort(pool.begin(), pool.begin() + c);
        for (size_t i = 0; i < c; ++i) {
            const uint32_t s = 1 + rng() % 5;
            r.t.push_back(pool[i]);
            r.s.push_back(s);
            r.total.push_back(s * (2 + rng() % 3));
        }
        r.o.push_back(r.t.size());
    }
    return r;
}

int main() {
    Engine e(0);
    std::mt19937_64 rng(0x3E26E);
    // three parts with totals over 1 500 targets each; rows of 0 .. 1 100 hits, unevenly spread
    const std::vector<std::vector<size_t>> lens = {{0, 1, 0, 15, 64, 300, 1100, 0, 7, 0}, {0, 0, 1, 2, 1, 0, 1024, 0, 65, 0}, {0, 1, 1, 0, 17, 5, 900, 700, 16, 0}};
    std::vector<Rec> host;
    std::vector<SearchHits> dev(3);
    for (size_t p = 0; p < 3; ++p) {
        host.push_back(random_hits(rng, lens[p], 1500));
        CHECK(dev[p].from_host(e, host[p].o, host[p].t, host[p].s, host[p].total) == BSK_OK);
    }
    const std::vector<const SearchHits *> parts = {&dev[0], &dev[1], &dev[2]};
    uint64_t dups = 0;
    SearchHits out;
    // shards by target: disjoint bases -> concat
    const std::vector<uint64_t> base = {0, 1500, 3000};
    CHECK(SearchHits::merge(e, parts, base, false, out) == BSK_OK);
    CHECK(fetch_all(e, out) == merge_model(host, base, &dups) && dups == 0);
    CHECK(plan_of(out).find("path=concat parts=3") != std::string::npos && out.large_queries() == 0);
    {
        SearchHits fresh = SearchHits::merge(e, parts, base, false);  // the form that returns its result
        CHECK(fresh.get() != nullptr && fetch_all(e, fresh) == fetch_all(e, out));
    }
    // shards by value: equal bases, the pairs that several parts report add up -> sort
    CHECK(SearchHits::merge(e, parts, {}, false, out) == BSK_ERR_ARG);  // duplicates without ADD
    CHECK(SearchHits::merge(e, parts, {}, true, out) == BSK_OK);
    const Rec added = merge_model(host, {}, &dups);
    CHECK(fetch_all(e, out) == added && dups != 0);
    CHECK(plan_of(out).find("path=sort parts=3") != std::string::npos && plan_of(out).find("combined=" + std::to_string(dups)) != std::string::npos);
    // decreasing bases: disjoint, but not in the order of the parts -> sort, nothing combined
    const std::vector<uint64_t> down = {3000, 1500, 0};
    CHECK(SearchHits::merge(e, parts, down, false, out) == BSK_OK);
    CHECK(fetch_all(e, out) == merge_model(host, down, &dups) && dups == 0 && plan_of(out).find("path=sort") != std::string::npos &&
          plan_of(out).find("combined=0") != std::string::npos);
    // one part with a base: a relabelling
    CHECK(SearchHits::merge(e, {&dev[2]}, {77}, false, out) == BSK_OK && fetch_all(e, out) == merge_model({host[2]}, {77}, &dups));
    // a top-n result has unordered rows: legal input
    {
        SearchHits top0, top1;
        CHECK(dev[0].top(e, 3, top0) == BSK_OK && dev[1].top(e, 3, top1) == BSK_OK);
        const std::vector<uint64_t> b2 = {0, 1500};
        CHECK(SearchHits::merge(e, {&top0, &top1}, b2, false, out) == BSK_OK);
        CHECK(fetch_all(e, out) == merge_model({fetch_all(e, top0), fetch_all(e, top1)}, b2, &dups) && out.totals_device() == nullptr);
    }
    // saturation: shared and total of 2^32 - 1 plus 1
    {
        SearchHits a, b;
        CHECK(a.from_host(e, {0, 2}, {3, 9}, {0xFFFFFFFFu, 5}, {0xFFFFFFFFu, 6}) == BSK_OK && b.from_host(e, {0, 2}, {3, 9}, {1, 7}, {1, 8}) == BSK_OK);
        CHECK(SearchHits::merge(e, {&a, &b}, {}, true, out) == BSK_OK);
        const Rec r = fetch_all(e, out);
        CHECK(r.o == (std::vector<uint64_t>{0, 2}) && r.t == (std::vector<uint32_t>{3, 9}) && r.s == (std::vector<uint32_t>{0xFFFFFFFFu, 12}) &&
              r.total == (std::vector<uint32_t>{0xFFFFFFFFu, 14}));
    }
    // weighted neighbours of counted sets and folded hits: the payloads all parts carry
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
    CHECK(SearchHits::merge(e, {&nb, &nb}, {0, 60}, false, out) == BSK_OK && fetch_all(e, out) == merge_model({nrec, nrec}, {0, 60}, &dups));
    CHECK(out.weights_device().first != nullptr && out.totals_device() != nullptr && out.members_device() == nullptr);
    CHECK(SearchHits::merge(e, {&nb, &nb}, {}, true, out) == BSK_OK && fetch_all(e, out) == merge_model({nrec, nrec}, {}, &dups) && dups == nrec.t.size());
    {
        Rec plain = host[0];
        plain.total.clear();
        SearchHits hp, folded;
        CHECK(hp.from_host(e, plain.o, plain.t, plain.s) == BSK_OK);
        std::vector<uint64_t> go;
        for (uint64_t g = 0; g <= 1500; g += 3) go.push_back(g);
        CHECK(hp.fold(e, go, nullptr, folded) == BSK_OK);
        const Rec frec = fetch_all(e, folded);
        CHECK(!frec.members.empty());
        CHECK(SearchHits::merge(e, {&folded, &folded}, {}, true, out) == BSK_OK && fetch_all(e, out) == merge_model({frec, frec}, {}, &dups));
        CHECK(out.members_device() != nullptr && out.totals_device() == nullptr && out.weights_device().first == nullptr);
        // members and totals meet: neither is carried
        Rec p0 = host[0];
        CHECK(SearchHits::merge(e, {&folded, &dev[0]}, {0, 500}, false, out) == BSK_OK);
        p0.total.clear();
        Rec f0 = frec;
        f0.members.clear();
        CHECK(fetch_all(e, out) == merge_model({f0, p0}, {0, 500}, &dups) && out.members_device() == nullptr && out.totals_device() == nullptr);
    }
    // a part of a second engine on the same device
    {
        Engine e2(0);
        SearchHits other;
        CHECK(other.from_host(e2, host[1].o, host[1].t, host[1].s, host[1].total) == BSK_OK);
        CHECK(SearchHits::merge(e, {&dev[0], &other, &dev[2]}, base, false, out) == BSK_OK && fetch_all(e, out) == merge_model(host, base, &dups));
        bsk_hits *held = other.get();
        CHECK(SearchHits::merge(e, parts, base, false, other) == BSK_ERR_ARG && other.get() == held);  // *out of another context
    }
    // empties
    {
        SearchHits none, none2, empty;
        CHECK(none.from_host(e, {0, 0, 0}, {}, {}) == BSK_OK && none2.from_host(e, {0, 0, 0}, {}, {}) == BSK_OK);
        CHECK(SearchHits::merge(e, {&none, &none2}, {}, false, empty) == BSK_OK && fetch_all(e, empty).o == std::vector<uint64_t>(3, 0));
        CHECK(none.from_host(e, {0}, {}, {}) == BSK_OK && SearchHits::merge(e, {&none}, {}, true, empty) == BSK_OK && fetch_all(e, empty).o == std::vector<uint64_t>(1, 0));
    }
    // the refusals keep the slot and what it holds
    CHECK(SearchHits::merge(e, parts, base, false, out) == BSK_OK);
    bsk_hits *held = out.get();
    const Rec before = fetch_all(e, out);
    CHECK(SearchHits::merge(e, parts, {}, false, out) == BSK_ERR_ARG && out.get() == held);                       // a duplicate without ADD
    CHECK(SearchHits::merge(e, {&dev[0], &out}, {}, true, out) == BSK_ERR_ARG && out.get() == held);              // *out among the parts
    CHECK(SearchHits::merge(e, parts, {0, 1ull << 32, 0}, true, out) == BSK_ERR_ARG && out.get() == held);        // a base of 2^32
    CHECK(SearchHits::merge(e, parts, {0, 0xFFFFFFFFull, 0}, true, out) == BSK_ERR_UNSUPPORTED && out.get() == held);  // base + target beyond 32 bits
    CHECK(SearchHits::merge(e, parts, {0, 0}, true, out) == BSK_ERR_ARG && out.get() == held);                    // a base per part
    {
        const bsk_hits *hs[2] = {dev[0].get(), nullptr};
        CHECK(bsk_hits_merge(e.ctx(), hs, nullptr, 2, 0, &out.handle()) == BSK_ERR_ARG && out.get() == held);     // a NULL part
        CHECK(bsk_hits_merge(e.ctx(), hs, nullptr, 1, 2, &out.handle()) == BSK_ERR_ARG && out.get() == held);     // a flag bit
        CHECK(bsk_hits_merge(e.ctx(), hs, nullptr, 0, 0, &out.handle()) == BSK_ERR_ARG && out.get() == held);     // no parts
        SearchHits rows3;
        CHECK(rows3.from_host(e, {0, 0, 0, 0}, {}, {}) == BSK_OK);
        CHECK(SearchHits::merge(e, {&dev[0], &rows3}, {}, true, out) == BSK_ERR_ARG && out.get() == held);        // rows that differ
    }
    CHECK(fetch_all(e, out) == before);  // kept means intact

    if (fails) {
        std::printf("%d C++ merge checks FAILED\n", fails);
        return 1;
    }
    std::printf("all C++ merge checks passed\n");
    return 0;
}
