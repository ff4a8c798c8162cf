// sketches.hpp -- C++17 host-side mirror of the reference `sketches` package over the
// C ABI (include/biosketch.h).  Header only; links against libbiosketch.so.
//
// Same names, argument order and error behaviour as shenwei356/bio sketches/:
//   NewHashIterator / NextHash            iterator.go:615,658
//   NewKmerIterator / NextKmer            iterator.go:668,708
//   NewSimHashIterator / NextSimHash      iterator.go:113,191
//   NewMinimizerSketch / NextMinimizer    sketch.go:85,205
//   NewSyncmerSketch / NextSyncmer        sketch.go:142,312
//   NewProteinIterator / Next             iterator-protein.go:46,76
//   NewProteinMinimizerSketch / Next      sketch-protein.go:62,106
//   Index()                               iterator.go:776, sketch.go:488, ...
// Go returns (obj, err); here constructors return a std::unique_ptr and write the
// sentinel code to *err (bsk_err values 1..11 are the reference's sentinels).
// The device works on batches: Engine::batch() + Batch::run() is the fast path and
// Result::sketch(i) / iterator(i) hand out the same cursor types.
#pragma once
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "biosketch.h"

namespace sketches {

constexpr int ErrInvalidK = BSK_ERR_INVALID_K, ErrEmptySeq = BSK_ERR_EMPTY_SEQ, ErrShortSeq = BSK_ERR_SHORT_SEQ,
              ErrIllegalBase = BSK_ERR_ILLEGAL_BASE, ErrKTooLarge = BSK_ERR_K_TOO_LARGE, ErrInvalidM = BSK_ERR_INVALID_M,
              ErrInvalidScale = BSK_ERR_INVALID_SCALE, ErrInvalidS = BSK_ERR_INVALID_S, ErrInvalidW = BSK_ERR_INVALID_W;

struct Seq {  // seq.Seq (seq/seq.go:29-34): only the alphabet identity and the bytes cross the boundary
    bool protein = false;
    std::string Seq_;
};

class Cursor {  // common part of Iterator / Sketch / ProteinIterator / ProteinMinimizerSketch
   public:
    bool next(uint64_t &code) {
        if (i_ >= codes_.size()) return false;
        code = codes_[i_];
        idx_ = pos_.empty() ? (long)i_ : (long)(pos_[i_] & BSK_POS_MASK);
        if (per_strand_) idx_ %= (long)per_strand_;
        strand_ = pos_.empty() ? 0 : (int)(pos_[i_] >> 31);
        ++i_;
        return true;
    }
    long Index() const { return idx_; }
    int Strand() const { return strand_; }    // extension: 1 iff the reverse-strand hash was canonical
    uint8_t Status() const { return status_; }  // extension: BSK_ST_* flags of the read
    std::vector<uint64_t> codes_;
    std::vector<uint32_t> pos_;
    uint8_t status_ = 0;
    size_t i_ = 0, per_strand_ = 0;
    long idx_ = -1;
    int strand_ = 0;
};

struct Iterator : Cursor {
    bool NextHash(uint64_t &c) { return next(c); }
    bool NextSimHash(uint64_t &c) { return next(c); }
    bool NextKmer(uint64_t &c, int *err) {  // iterator.go:708: (code, ok, err)
        if (err) *err = 0;
        if (next(c)) return true;
        if (err && (status_ & BSK_ST_CODE_MASK) == BSK_ST_ILLEGAL) *err = ErrIllegalBase;
        return false;
    }
};
struct Sketch : Cursor {
    bool NextMinimizer(uint64_t &c) { return next(c); }
    bool NextSyncmer(uint64_t &c) { return next(c); }
    bool Next(uint64_t &c) { return next(c); }
};
struct ProteinIterator : Cursor {
    bool Next(uint64_t &c) { return next(c); }
};
struct ProteinMinimizerSketch : Cursor {
    bool Next(uint64_t &c) { return next(c); }
};

class Engine;

class Result {
   public:
    std::vector<uint64_t> offsets, hash;
    std::vector<uint32_t> pos;
    std::vector<uint8_t> status;
    template <class C>
    std::unique_ptr<C> cursor(size_t i, int *err) const {
        if ((status[i] & BSK_ST_CODE_MASK) == BSK_ST_SHORT) {
            if (err) *err = ErrShortSeq;
            return nullptr;
        }
        if (err) *err = 0;
        auto c = std::make_unique<C>();
        c->codes_.assign(hash.begin() + offsets[i], hash.begin() + offsets[i + 1]);
        if (!pos.empty()) c->pos_.assign(pos.begin() + offsets[i], pos.begin() + offsets[i + 1]);
        c->status_ = status[i];
        return c;
    }
};

class Engine {
   public:
    explicit Engine(int device = 0) {
        int rc = bsk_ctx_create(device, &ctx_);
        if (rc != BSK_OK) throw std::runtime_error(std::string("bsk_ctx_create: ") + bsk_err_name(rc));
    }
    ~Engine() { bsk_ctx_destroy(ctx_); }
    Engine(const Engine &) = delete;
    // one launch over a batch of sequences; returns the sentinel / engine error code (0 = ok)
    int run(const std::vector<std::string_view> &seqs, bool protein, const bsk_params &p, Result &out) {
        std::vector<uint64_t> offs(seqs.size() + 1, 0);
        std::string bytes;
        for (size_t i = 0; i < seqs.size(); ++i) {
            bytes.append(seqs[i]);
            offs[i + 1] = bytes.size();
        }
        bsk_batch *b = nullptr;
        int rc = bsk_batch_from_ascii(ctx_, (const uint8_t *)bytes.data(), offs.data(), seqs.size(),
                                      protein ? BSK_ALPHA_PROTEIN : BSK_ALPHA_DNA, &b);
        if (rc != BSK_OK) return rc;
        bsk_result *r = nullptr;
        rc = bsk_sketch(ctx_, b, &p, &r);
        if (rc == BSK_OK) {
            uint64_t n = 0, t = 0;
            int hp = 0;
            bsk_result_info(r, &n, &t, &hp);
            out.offsets.assign(n + 1, 0);
            out.status.assign(n + 1, 0);
            out.hash.assign(t + 1, 0);
            out.pos.assign(hp ? t + 1 : 0, 0);
            rc = bsk_result_fetch(ctx_, r, 0, n, out.offsets.data(), out.status.data(), out.hash.data(),
                                  hp ? out.pos.data() : nullptr, t + 1);
            out.hash.resize(t);
            if (hp) out.pos.resize(t);
        }
        if (r) bsk_result_release(r);
        bsk_batch_destroy(b);
        return rc;
    }
    const char *last_error() const { return bsk_last_error(ctx_); }
    bsk_ctx *ctx() const { return ctx_; }  // for the C entries without a mirror here

   private:
    bsk_ctx *ctx_ = nullptr;
};

// ---- containment search (include/biosketch.h): RAII owners of the device objects ----
template <class T, void (*Release)(T *)>
class Owned {
   public:
    Owned() = default;
    ~Owned() { Release(p_); }
    Owned(Owned &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) {
            Release(p_);
            p_ = o.p_;
            o.p_ = nullptr;
        }
        return *this;
    }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    T *get() const { return p_; }
    T *&handle() { return p_; }  // in-out slot for the C entries (release before overwriting, or pass for re-use)

   protected:
    T *p_ = nullptr;
};

// sorted distinct value sets on the device (bsk_sets)
class DeviceSets : public Owned<bsk_sets, bsk_sets_release> {
   public:
    // offsets[n+1] (offsets[0] = 0, offsets[n] = values.size()), values strictly ascending inside a set
    int from_host(Engine &e, const std::vector<uint64_t> &offsets, const std::vector<uint64_t> &values) {
        if (offsets.empty() || offsets.back() != values.size()) return BSK_ERR_ARG;
        bsk_sets_release(p_);
        p_ = nullptr;
        return bsk_sets_from_host(e.ctx(), offsets.data(), offsets.size() - 1, values.empty() ? nullptr : values.data(), &p_);
    }
    uint64_t n_sets() const {
        uint64_t n = 0;
        bsk_sets_info(p_, &n, nullptr);
        return n;
    }
    int fetch(Engine &e, std::vector<uint64_t> &offsets, std::vector<uint64_t> &values) const {
        uint64_t n = 0, nv = 0;
        int rc = bsk_sets_info(p_, &n, &nv);
        if (rc != BSK_OK) return rc;
        offsets.assign(n + 1, 0);
        values.assign(nv + 1, 0);
        rc = bsk_sets_fetch(e.ctx(), p_, 0, n, offsets.data(), values.data(), nv + 1);
        values.resize(nv);
        return rc;
    }
    // set algebra (bsk_sets_op / bsk_sets_reduce) INTO this object: empty, or the result of an earlier op / reduce on this engine (its
    // device arrays are kept and only grow); it must be neither a nor b.  which: BSK_SETOP_*; a b of one set is combined with every set of a
    int op(Engine &e, const DeviceSets &a, const DeviceSets &b, int which) { return bsk_sets_op(e.ctx(), a.get(), b.get(), which, &p_); }
    // group g: sets group_offsets[g] .. group_offsets[g + 1] - 1 of s; the values at least min_members of them hold (1: union,
    // BSK_MEMBERS_ALL: intersection)
    int reduce(Engine &e, const DeviceSets &s, const std::vector<uint64_t> &group_offsets, uint32_t min_members = 1) {
        if (group_offsets.empty()) return BSK_ERR_ARG;
        return bsk_sets_reduce(e.ctx(), s.get(), group_offsets.data(), group_offsets.size() - 1, min_members, &p_);
    }
    // pairs of the last op into this object that took the group, wave and tiled path
    void paths(uint64_t n_by_path[3]) const { bsk_sets_plan(p_, nullptr, n_by_path); }

    // ---- counted sets: values with their abundance (counts[i] belongs to values[i]) ----
    // the counted sets of a result INTO this object (empty, or any sets of this engine: arrays kept, grow only)
    int from_result_counted(Engine &e, const bsk_result *r, int scope, int scale = 1) { return bsk_result_sets_counted(e.ctx(), r, scope, scale, &p_); }
    // one set per window of every sequence's positions (bsk_result_sets_windows) INTO this object: wp.window / wp.step, or wp.count windows
    // per sequence; seq_offsets[n_reads + 1] receives where every sequence's windows start (the group offsets of reduce and SearchHits::fold)
    int from_windows(Engine &e, const bsk_result *r, const bsk_window_params &wp, int scale, std::vector<uint64_t> *seq_offsets = nullptr) {
        uint64_t n = 0;
        if (seq_offsets && bsk_result_info(r, &n, nullptr, nullptr) == BSK_OK) seq_offsets->assign(n + 1, 0);
        return bsk_result_sets_windows(e.ctx(), r, &wp, scale, &p_, seq_offsets ? seq_offsets->data() : nullptr);
    }
    int from_host_counted(Engine &e, const std::vector<uint64_t> &offsets, const std::vector<uint64_t> &values, const std::vector<uint32_t> &counts) {
        if (offsets.empty() || offsets.back() != values.size() || counts.size() != values.size()) return BSK_ERR_ARG;
        bsk_sets_release(p_);
        p_ = nullptr;
        return bsk_sets_from_host_counted(e.ctx(), offsets.data(), offsets.size() - 1, values.empty() ? nullptr : values.data(), counts.empty() ? nullptr : counts.data(), &p_);
    }
    bool counted() const {
        const uint32_t *c = nullptr;
        return bsk_sets_counts_device(p_, &c) == BSK_OK && c != nullptr;
    }
    int fetch_counts(Engine &e, std::vector<uint32_t> &counts) const {
        uint64_t n = 0, nv = 0;
        int rc = bsk_sets_info(p_, &n, &nv);
        if (rc != BSK_OK) return rc;
        counts.assign(nv + 1, 0);
        rc = bsk_sets_fetch_counts(e.ctx(), p_, 0, n, counts.data(), nv + 1);
        counts.resize(nv);
        return rc;
    }
    // which: BSK_COUNTOP_*; INTO this object as op(); an a of one set is combined with every set of b
    int op_counted(Engine &e, const DeviceSets &a, const DeviceSets &b, int which) { return bsk_sets_op_counted(e.ctx(), a.get(), b.get(), which, &p_); }
    int filter_counts(Engine &e, const DeviceSets &s, uint32_t min_count = 1, uint32_t max_count = 0xFFFFFFFFu) {
        return bsk_sets_filter_counts(e.ctx(), s.get(), min_count, max_count, &p_);
    }
    int totals(Engine &e, std::vector<uint64_t> &out) const {
        const uint64_t n = n_sets();
        out.assign(n + 1, 0);
        const int rc = bsk_sets_totals(e.ctx(), p_, 0, n, out.data());
        out.resize(n);
        return rc;
    }

    // per set the sum of its squared counts, saturating at 2^64 - 1 (the sets' sizes for sets without counts): the norms of cosine
    int sumsq(Engine &e, std::vector<uint64_t> &out) const {
        const uint64_t n = n_sets();
        out.assign(n + 1, 0);
        const int rc = bsk_sets_sumsq(e.ctx(), p_, 0, n, out.data());
        out.resize(n);
        return rc;
    }

    // ---- MinHash: every set of s cut to its min(n, size) smallest values (counts ride along) INTO this object, as op() ----
    int bottom(Engine &e, const DeviceSets &s, uint64_t n) { return bsk_sets_bottom(e.ctx(), s.get(), n, &p_); }
    // every set of this object against every set of b, the pairs that pass np only (defined below SearchHits)
    int neighbors(Engine &e, const DeviceSets &b, uint64_t limit, const bsk_neighbor_params *np, class SearchHits &into) const;
    // ... and with the counts: the same pairs, and dot and min_sum of every kept pair (defined below SearchHits)
    int neighbors_counted(Engine &e, const DeviceSets &b, uint64_t limit, const bsk_neighbor_params *np, class SearchHits &into) const;
};

// dense all-pairs comparison (bsk_compare): shared[n_a * n_b] and total[n_a * n_b], row-major
class SetsCompare : public Owned<bsk_compare, bsk_compare_release> {
   public:
    // every set of a against every set of b INTO this object (empty, or the result of an earlier compare on this engine: arrays kept,
    // grow only); limit: the distinct values of a pair's union that are walked (0: all -- the exact Jaccard; n: the Mash estimator)
    int compare(Engine &e, const DeviceSets &a, const DeviceSets &b, uint64_t limit = 0) { return bsk_sets_compare(e.ctx(), a.get(), b.get(), limit, &p_); }
    // compare() with the counts: besides shared and total, dot = the sum of ca * cb (saturating at 2^64 - 1) and min_sum = the sum of min(ca, cb)
    // over the walked values both sets hold; sets without counts count 1 for every value.  A later compare() leaves the object unweighted
    int compare_counted(Engine &e, const DeviceSets &a, const DeviceSets &b, uint64_t limit = 0) { return bsk_sets_compare_counted(e.ctx(), a.get(), b.get(), limit, &p_); }
    bool weighted() const {
        const uint64_t *d = nullptr, *m = nullptr;
        return bsk_compare_weights_device(p_, &d, &m) == BSK_OK && d != nullptr && m != nullptr;
    }
    int fetch_weights(Engine &e, std::vector<uint64_t> &dot, std::vector<uint64_t> &min_sum) const {  // BSK_ERR_ARG for an unweighted result
        uint64_t n_a = 0, n_b = 0;
        int rc = bsk_compare_info(p_, &n_a, &n_b, nullptr);
        if (rc != BSK_OK) return rc;
        dot.assign(n_a * n_b + 1, 0);
        min_sum.assign(n_a * n_b + 1, 0);
        rc = bsk_compare_fetch_weights(e.ctx(), p_, 0, n_a, dot.data(), min_sum.data(), n_a * n_b);
        dot.resize(n_a * n_b);
        min_sum.resize(n_a * n_b);
        return rc;
    }
    int info(uint64_t &n_a, uint64_t &n_b, uint64_t &limit) const { return bsk_compare_info(p_, &n_a, &n_b, &limit); }
    // figures: tiles run, rounds summed over the tiles, most rounds of one tile
    const char *plan(uint64_t figures[3]) const {
        const char *d = "";
        bsk_compare_plan(p_, &d, figures);
        return d;
    }
    int fetch(Engine &e, std::vector<uint32_t> &shared, std::vector<uint32_t> &total) const {
        uint64_t n_a = 0, n_b = 0;
        int rc = bsk_compare_info(p_, &n_a, &n_b, nullptr);
        if (rc != BSK_OK) return rc;
        shared.assign(n_a * n_b + 1, 0);
        total.assign(n_a * n_b + 1, 0);
        rc = bsk_compare_fetch(e.ctx(), p_, 0, n_a, shared.data(), total.data(), n_a * n_b);
        shared.resize(n_a * n_b);
        total.resize(n_a * n_b);
        return rc;
    }
    void device(const uint32_t *&shared, const uint32_t *&total) const { bsk_compare_device(p_, &shared, &total); }
};

// clusters of a hits graph (bsk_clusters): label[n], rep[n_clusters] ascending, offsets[n_clusters + 1], members[n]
class Clusters : public Owned<bsk_clusters, bsk_clusters_release> {
   public:
    uint64_t n_items() const { return info(0); }
    uint64_t n_clusters() const { return info(1); }
    uint64_t largest() const { return info(2); }
    // the rounds the host drove and the hits off the diagonal (bsk_clusters_plan)
    uint64_t rounds() const { return figure(0); }
    uint64_t edges() const { return figure(1); }
    std::string plan() const {
        const char *p = "";
        bsk_clusters_plan(p_, &p, nullptr);
        return p ? p : "";
    }
    int fetch(Engine &e, std::vector<uint32_t> &label, std::vector<uint32_t> &rep, std::vector<uint64_t> &offsets, std::vector<uint32_t> &members) const {
        uint64_t n = 0, nc = 0;
        int rc = bsk_clusters_info(p_, &n, &nc, nullptr);
        if (rc != BSK_OK) return rc;
        label.assign(n + 1, 0);
        rep.assign(nc + 1, 0);
        offsets.assign(nc + 1, 0);
        members.assign(n + 1, 0);
        rc = bsk_clusters_fetch(e.ctx(), p_, label.data(), rep.data(), offsets.data(), members.data());
        label.resize(n);
        rep.resize(nc);
        members.resize(n);
        return rc;
    }
    void device(const uint32_t *&label, const uint32_t *&rep, const uint64_t *&offsets, const uint32_t *&members) const {
        bsk_clusters_device(p_, &label, &rep, &offsets, &members);
    }

   private:
    uint64_t info(int i) const {
        uint64_t v[3] = {0, 0, 0};
        bsk_clusters_info(p_, &v[0], &v[1], &v[2]);
        return v[i];
    }
    uint64_t figure(int i) const {
        uint64_t f[2] = {0, 0};
        bsk_clusters_plan(p_, nullptr, f);
        return f[i];
    }
};

// the per-target table of hits (bsk_tally): rows[n_targets], unique[n_targets], shared[n_targets], u64 each
class Tally : public Owned<bsk_tally, bsk_tally_release> {
   public:
    uint64_t n_targets() const { return info(0); }
    // what the table holds: the rows, hits and calls tallied into it (they add up under BSK_TALLY_ADD)
    uint64_t queries() const { return info(1); }
    uint64_t hits() const { return info(2); }
    uint64_t calls() const { return info(3); }
    std::string plan() const {
        const char *p = "";
        bsk_tally_plan(p_, &p);
        return p ? p : "";
    }
    int fetch(Engine &e, std::vector<uint64_t> &rows, std::vector<uint64_t> &unique, std::vector<uint64_t> &shared) const {
        const uint64_t n = n_targets();
        rows.assign(n + 1, 0);
        unique.assign(n + 1, 0);
        shared.assign(n + 1, 0);
        const int rc = bsk_tally_fetch(e.ctx(), p_, 0, n, rows.data(), unique.data(), shared.data());
        rows.resize(n);
        unique.resize(n);
        shared.resize(n);
        return rc;
    }
    void device(const uint64_t *&rows, const uint64_t *&unique, const uint64_t *&shared) const { bsk_tally_device(p_, &rows, &unique, &shared); }

   private:
    uint64_t info(int i) const {
        uint64_t v[4] = {0, 0, 0, 0};
        bsk_tally_info(p_, &v[0], &v[1], &v[2], &v[3]);
        return v[i];
    }
};

// hits of a search (bsk_hits): CSR by query, target ids ascending inside a query
class SearchHits : public Owned<bsk_hits, bsk_hits_release> {
   public:
    // hits made elsewhere (bsk_hits_from_host): offsets[n + 1] from 0, targets strictly ascending inside a row, shared[] and, if not
    // empty, total[]; INTO this object (its device arrays are kept and only grow)
    int from_host(Engine &e, const std::vector<uint64_t> &offsets, const std::vector<uint32_t> &target, const std::vector<uint32_t> &shared,
                  const std::vector<uint32_t> &total = {}) {
        return hits_from_host(e, offsets, target, shared, total, *this);
    }
    // the hits as an undirected graph over their queries, clustered on the device (bsk_hits_cluster): method BSK_CLUSTER_COMPONENTS or
    // BSK_CLUSTER_GREEDY; score: one u64 per query (higher is better, ties to the smaller index) or empty for index order; into: empty,
    // or the clusters of an earlier call on this engine
    int cluster(Engine &e, uint32_t method, const std::vector<uint64_t> &score, Clusters &into) const {
        uint64_t nq = 0;
        bsk_hits_info(p_, &nq, nullptr);
        if (!score.empty() && score.size() != nq) return BSK_ERR_ARG;
        const bsk_cluster_params cp{method, 0};
        return bsk_hits_cluster(e.ctx(), p_, &cp, score.empty() ? nullptr : score.data(), &into.handle());
    }
    static int hits_from_host(Engine &e, const std::vector<uint64_t> &offsets, const std::vector<uint32_t> &target, const std::vector<uint32_t> &shared,
                              const std::vector<uint32_t> &total, SearchHits &into) {
        if (offsets.empty() || offsets.back() != target.size() || shared.size() != target.size() || (!total.empty() && total.size() != target.size())) return BSK_ERR_ARG;
        return bsk_hits_from_host(e.ctx(), offsets.data(), offsets.size() - 1, target.empty() ? nullptr : target.data(), shared.empty() ? nullptr : shared.data(),
                                  total.empty() ? nullptr : total.data(), &into.handle());
    }
    int fetch(Engine &e, std::vector<uint64_t> &offsets, std::vector<uint32_t> &target, std::vector<uint32_t> &shared) const {
        uint64_t nq = 0, nh = 0;
        int rc = bsk_hits_info(p_, &nq, &nh);
        if (rc != BSK_OK) return rc;
        offsets.assign(nq + 1, 0);
        target.assign(nh + 1, 0);
        shared.assign(nh + 1, 0);
        rc = bsk_hits_fetch(e.ctx(), p_, 0, nq, offsets.data(), target.data(), shared.data(), nh + 1);
        target.resize(nh);
        shared.resize(nh);
        return rc;
    }
    uint64_t large_queries() const {
        uint64_t n = 0;
        bsk_hits_plan(p_, nullptr, &n);
        return n;
    }
    // every query's min(n, hits) best hits, largest shared count first, ties by ascending target (bsk_hits_top); into: empty, or the
    // result of an earlier top on this engine (its device arrays are kept and only grow)
    int top(Engine &e, uint32_t n, SearchHits &into) const { return bsk_hits_top(e.ctx(), p_, n, &into.handle()); }
    // the hits summed by target group (bsk_hits_fold): group g is targets group_offsets[g] .. group_offsets[g + 1] - 1; fp: nullptr keeps every
    // group with a hit; into: empty, or any hits of this engine but this object.  The result carries members (members_device, fetch_members)
    int fold(Engine &e, const std::vector<uint64_t> &group_offsets, const bsk_fold_params *fp, SearchHits &into) const {
        if (group_offsets.empty()) return BSK_ERR_ARG;
        return bsk_hits_fold(e.ctx(), p_, group_offsets.data(), group_offsets.size() - 1, fp, &into.handle());
    }
    // the hits whose measure m is at least min_num / min_den, compared exactly (bsk_hits_filter): rows in their order, every payload kept;
    // m.qnorm / m.tnorm are host arrays, read during the call only; into: empty, or any hits of this engine but this object
    int filter(Engine &e, const bsk_measure &m, uint64_t min_num, uint64_t min_den, SearchHits &into) const {
        const bsk_filter_params fp{min_num, min_den};
        return bsk_hits_filter(e.ctx(), p_, &m, &fp, &into.handle());
    }
    // every query's min(n, hits) hits of largest measure, best first, ties by ascending target, every payload kept (bsk_hits_top_by)
    int top_by(Engine &e, const bsk_measure &m, uint32_t n, SearchHits &into) const { return bsk_hits_top_by(e.ctx(), p_, &m, n, &into.handle()); }
    // the hits by target (bsk_hits_transpose): n_targets rows, row t the queries that hit t, ascending, every payload with its hit; into:
    // empty, or any hits of this engine but this object
    int transpose(Engine &e, uint64_t n_targets, SearchHits &into) const { return bsk_hits_transpose(e.ctx(), p_, n_targets, &into.handle()); }
    // the per-target table (bsk_hits_tally): into: empty, or an earlier table of this engine -- overwritten, or with add == true (and the
    // same n_targets) added to
    int tally(Engine &e, uint64_t n_targets, bool add, Tally &into) const {
        return bsk_hits_tally(e.ctx(), p_, n_targets, add ? (uint32_t)BSK_TALLY_ADD : 0u, &into.handle());
    }
    // one SearchHits out of the hits of several searches of the same queries (bsk_hits_merge): row q holds every hit of row q of every
    // part with base[p] added to its target (base empty: all 0), strictly ascending, with every payload all parts carry; a pair that
    // occurs twice is BSK_ERR_ARG unless add, which sums its fields, saturating.  Parts may belong to other engines.  into: empty, or
    // any hits of this engine that are not among the parts
    static int merge(Engine &e, const std::vector<const SearchHits *> &parts, const std::vector<uint64_t> &base, bool add, SearchHits &into) {
        if (parts.empty() || (!base.empty() && base.size() != parts.size())) return BSK_ERR_ARG;
        std::vector<const bsk_hits *> hs;
        for (const SearchHits *p : parts) hs.push_back(p ? p->get() : nullptr);
        return bsk_hits_merge(e.ctx(), hs.data(), base.empty() ? nullptr : base.data(), (uint32_t)hs.size(), add ? (uint32_t)BSK_MERGE_ADD : 0u, &into.handle());
    }
    // ... as a new object: empty (get() == nullptr) when the call failed, and the engine's error says why
    static SearchHits merge(Engine &e, const std::vector<const SearchHits *> &parts, const std::vector<uint64_t> &base, bool add) {
        SearchHits out;
        (void)merge(e, parts, base, add, out);
        return out;
    }
    const uint32_t *members_device() const {  // nullptr for hits without members
        const uint32_t *m = nullptr;
        bsk_hits_members_device(p_, &m);
        return m;
    }
    int fetch_members(Engine &e, std::vector<uint32_t> &members) const {  // BSK_ERR_ARG for hits without members
        uint64_t nq = 0, nh = 0;
        int rc = bsk_hits_info(p_, &nq, &nh);
        if (rc != BSK_OK) return rc;
        members.assign(nh + 1, 0);
        rc = bsk_hits_fetch_members(e.ctx(), p_, 0, nq, members.data(), nh + 1);
        members.resize(nh);
        return rc;
    }
    // hits with totals (DeviceSets::neighbors): the device array total[n_hits], nullptr for the hits of a search or of top()
    const uint32_t *totals_device() const {
        const uint32_t *t = nullptr;
        bsk_hits_totals_device(p_, &t);
        return t;
    }
    int fetch_totals(Engine &e, std::vector<uint32_t> &total) const {  // BSK_ERR_ARG for hits without totals
        uint64_t nq = 0, nh = 0;
        int rc = bsk_hits_info(p_, &nq, &nh);
        if (rc != BSK_OK) return rc;
        total.assign(nh + 1, 0);
        rc = bsk_hits_fetch_totals(e.ctx(), p_, 0, nq, total.data(), nh + 1);
        total.resize(nh);
        return rc;
    }
    // hits with weights (DeviceSets::neighbors_counted): the device arrays dot[n_hits] and min_sum[n_hits], both nullptr for any other hits
    std::pair<const uint64_t *, const uint64_t *> weights_device() const {
        const uint64_t *d = nullptr, *m = nullptr;
        bsk_hits_weights_device(p_, &d, &m);
        return {d, m};
    }
    int fetch_weights(Engine &e, std::vector<uint64_t> &dot, std::vector<uint64_t> &min_sum) const {  // BSK_ERR_ARG for hits without weights
        uint64_t nq = 0, nh = 0;
        int rc = bsk_hits_info(p_, &nq, &nh);
        if (rc != BSK_OK) return rc;
        dot.assign(nh + 1, 0);
        min_sum.assign(nh + 1, 0);
        rc = bsk_hits_fetch_weights(e.ctx(), p_, 0, nq, dot.data(), min_sum.data(), nh + 1);
        dot.resize(nh);
        min_sum.resize(nh);
        return rc;
    }
};

// sparse all-pairs comparison (bsk_sets_neighbors): per set of a the sets of b that pass np (nullptr: every pair that shares a value),
// walked as SetsCompare::compare walks them, INTO `into` -- empty, or any hits of this engine (arrays kept, grow only).  The hits carry
// totals; no matrix is stored and the number of cells is not limited.
inline int DeviceSets::neighbors(Engine &e, const DeviceSets &b, uint64_t limit, const bsk_neighbor_params *np, SearchHits &into) const {
    return bsk_sets_neighbors(e.ctx(), p_, b.get(), limit, np, &into.handle());
}
// bsk_sets_neighbors_counted: neighbors() with the counts of SetsCompare::compare_counted -- the same hits, which also carry weights
// (SearchHits::weights_device, fetch_weights); np reads shared and total only
inline int DeviceSets::neighbors_counted(Engine &e, const DeviceSets &b, uint64_t limit, const bsk_neighbor_params *np, SearchHits &into) const {
    return bsk_sets_neighbors_counted(e.ctx(), p_, b.get(), limit, np, &into.handle());
}

// inverted index of target sets (bsk_index)
class SearchIndex : public Owned<bsk_index, bsk_index_release> {
   public:
    int build(Engine &e, const DeviceSets &targets) {
        bsk_index_release(p_);
        p_ = nullptr;
        return bsk_index_build(e.ctx(), targets.get(), &p_);
    }
    // into: empty, or the hits of an earlier search on this engine (its device arrays are kept and only grow)
    int search(Engine &e, const DeviceSets &queries, const bsk_search_params &sp, SearchHits &into) const {
        return bsk_index_search(e.ctx(), p_, queries.get(), &sp, &into.handle());
    }
    // build() with the targets' counts (bsk_index_build_counted): per posting the target's count, per target the norms; sets without
    // counts give an index without counts
    int build_counted(Engine &e, const DeviceSets &targets) {
        bsk_index_release(p_);
        p_ = nullptr;
        return bsk_index_build_counted(e.ctx(), targets.get(), &p_);
    }
    bool counted() const {
        int k = 0;
        bsk_index_counted(p_, &k);
        return k != 0;
    }
    // sumsq[t] and totals[t] of every target (bsk_index_fetch_norms); an index without counts reports the sizes for both
    int fetch_norms(Engine &e, std::vector<uint64_t> &sumsq, std::vector<uint64_t> &totals) const {
        uint64_t n = 0;
        bsk_index_info(p_, &n, nullptr, nullptr, nullptr, nullptr);
        sumsq.assign(n, 0);
        totals.assign(n, 0);
        return bsk_index_fetch_norms(e.ctx(), p_, 0, n, sumsq.data(), totals.data());
    }
    // search() with the counts (bsk_index_search_counted): the same hits, and per hit dot and min_sum (SearchHits::fetch_weights)
    int search_counted(Engine &e, const DeviceSets &queries, const bsk_search_params &sp, SearchHits &into) const {
        return bsk_index_search_counted(e.ctx(), p_, queries.get(), &sp, &into.handle());
    }
    uint64_t max_bucket() const {
        uint64_t m = 0;
        bsk_index_info(p_, nullptr, nullptr, nullptr, &m, nullptr);
        return m;
    }
    // a handle on this index for another engine (bsk_index_attach): shared arrays on the same device, one copy on another; the handles
    // of an index may go in any order
    int attach(Engine &e, SearchIndex &handle) const {
        bsk_index_release(handle.p_);
        handle.p_ = nullptr;
        return bsk_index_attach(e.ctx(), p_, &handle.p_);
    }
};

// One chunk of a BSK_SINK_HITS pipeline: record i owns target / shared[offset(i) .. offset(i + 1)); valid inside the callback.
struct HitsChunk {
    const bsk_chunk *c = nullptr;
    const uint32_t *target = nullptr, *shared = nullptr;
    uint64_t offset(uint64_t i) const { return c->offsets32 ? c->offsets32[i] : c->offsets64[i]; }
};
// Reads in host memory in, every read's best targets out (bsk_pipeline_open_memory_search): on_chunk(const HitsChunk &) sees every
// chunk in input order.  ix may belong to any engine; it must have been built from sets of the same params and scale.
template <class F>
int classify_memory(const std::vector<int> &devices, int n_streams, uint64_t chunk_records, int sets_scale, const uint8_t *bytes, const uint64_t *offsets, uint64_t n,
                    const bsk_params &p, const SearchIndex &ix, const bsk_search_params &sp, uint32_t top_n, F &&on_chunk, bsk_pipeline_stats *stats = nullptr) {
    bsk_pipeline_config cfg{};
    cfg.devices = devices.data();
    cfg.n_devices = (int32_t)devices.size();
    cfg.n_streams = n_streams;
    cfg.chunk_records = chunk_records;
    cfg.sink = BSK_SINK_HITS;
    cfg.sets_scale = sets_scale;
    cfg.alphabet = BSK_ALPHA_DNA;
    const bsk_pipeline_search s{ix.get(), sp, top_n, 0};
    bsk_pipeline *pl = nullptr;
    int rc = bsk_pipeline_open_memory_search(&cfg, bytes, offsets, n, 1, &p, &s, &pl);
    if (rc != BSK_OK) return rc;
    for (;;) {
        const bsk_chunk *c = nullptr;
        rc = bsk_pipeline_next(pl, &c);
        if (rc != BSK_OK || !c) break;
        HitsChunk hc;
        hc.c = c;
        rc = bsk_chunk_hits(c, &hc.target, &hc.shared);
        if (rc == BSK_OK) on_chunk(hc);
        bsk_pipeline_release(pl, c);
        if (rc != BSK_OK) break;
    }
    const int crc = bsk_pipeline_close(pl, stats);
    return rc != BSK_OK ? rc : crc;
}

inline Engine &default_engine() {
    static Engine e(0);
    return e;
}

namespace detail {
template <class C>
std::unique_ptr<C> single(const Seq &s, const bsk_params &p, int *err, Engine *eng) {
    Result r;
    int rc = (eng ? *eng : default_engine()).run({std::string_view(s.Seq_)}, s.protein, p, r);
    if (rc != BSK_OK) {
        if (err) *err = rc;
        return nullptr;
    }
    return r.cursor<C>(0, err);
}
inline bsk_params params(int kind, int k) {
    bsk_params p{};
    p.kind = kind;
    p.k = k;
    p.canonical = 1;
    p.codon_table = 1;
    p.frame = 1;
    return p;
}
}  // namespace detail

inline std::unique_ptr<Iterator> NewHashIterator(const Seq &s, int k, bool canonical, bool circular, int *err, Engine *e = nullptr) {
    auto p = detail::params(BSK_NTHASH, k);
    p.canonical = canonical;
    p.circular = circular;
    return detail::single<Iterator>(s, p, err, e);
}
inline std::unique_ptr<Iterator> NewKmerIterator(const Seq &s, int k, bool canonical, bool circular, int *err, Engine *e = nullptr) {
    auto p = detail::params(BSK_KMER, k);
    p.canonical = canonical;
    p.circular = circular;
    auto it = detail::single<Iterator>(s, p, err, e);
    if (it && !canonical) it->per_strand_ = it->codes_.size() / 2;  // Index() restarts on the second strand (iterator.go:720)
    return it;
}
inline std::unique_ptr<Iterator> NewSimHashIterator(const Seq &s, int k, int m, int scale, bool canonical, bool circular, int *err,
                                                    Engine *e = nullptr) {
    auto p = detail::params(BSK_SIMHASH, k);
    p.m = m;
    p.scale = scale;
    p.canonical = canonical;
    p.circular = circular;
    return detail::single<Iterator>(s, p, err, e);
}
inline std::unique_ptr<Sketch> NewMinimizerSketch(const Seq &S, int k, int w, bool circular, int *err, Engine *e = nullptr) {
    auto p = detail::params(BSK_MINIMIZER, k);
    p.w = w;
    p.circular = circular;
    return detail::single<Sketch>(S, p, err, e);
}
inline std::unique_ptr<Sketch> NewSyncmerSketch(const Seq &S, int k, int s, bool circular, int *err, Engine *e = nullptr) {
    auto p = detail::params(BSK_SYNCMER, k);
    p.s = s;
    p.circular = circular;
    return detail::single<Sketch>(S, p, err, e);
}
inline std::unique_ptr<ProteinIterator> NewProteinIterator(const Seq &s, int k, int codonTable, int frame, int *err, Engine *e = nullptr) {
    auto p = detail::params(BSK_PROT_HASH, k);
    p.codon_table = codonTable;
    p.frame = frame;
    return detail::single<ProteinIterator>(s, p, err, e);
}
inline std::unique_ptr<ProteinMinimizerSketch> NewProteinMinimizerSketch(const Seq &S, int k, int codonTable, int frame, int w, int *err,
                                                                         Engine *e = nullptr) {
    if (k >= 1 && S.Seq_.size() < (size_t)k * 3) {  // upstream's order: k, then this length check (sketch-protein.go:66), only then w (:69)
        if (err) *err = BSK_ERR_SHORT_SEQ;
        return nullptr;
    }
    auto p = detail::params(BSK_PROT_MINIMIZER, k);
    p.w = w;
    p.codon_table = codonTable;
    p.frame = frame;
    return detail::single<ProteinMinimizerSketch>(S, p, err, e);
}

}  // namespace sketches
