// merge.hip -- one bsk_hits out of several (include/biosketch.h "merged hits"): bsk_hits_merge joins the hits of the searches against the
// shards of a database, shifted by a per-part target base, with every payload all parts carry; pairs that several shards report add up
// under BSK_MERGE_ADD.
//
//   k_mg_check     per part, a lane per hit: the part's smallest and largest target and whether a hit is not above its predecessor in
//                  its row (only such a hit pays for the search of its row).  One ballot per trip of a wavefront, one min / max per
//                  wavefront at the end.  The host reads one block of figures and picks the path.
//   k_mg_starts    a lane per row: the output offsets before any combining -- the sum of the parts' offsets -- and per part where its
//                  hits of the row begin (a bounded loop over at most 64 parts, whose pointers live in a pool array)
//   k_mg_place     per part, a lane per hit: the hit's row by a search of the part's offsets, then target + base, shared and every
//                  carried payload to their place.  On the concat path that place is the result: every array read once and written once.
// The sort path places into pool scratch with the key (target' << idx_bits) | place -- every key distinct -- and goes on:
//   sets_sort_segments_u64  over the rows
//   k_mg_rows, k_mg_heads   a hit is a HEAD where its row starts or its target' differs from its predecessor's; a hit that is none is a
//                  duplicate, which without BSK_MERGE_ADD refuses the call before the result slot is taken over
//   scan_counts    over the heads -> the place of every output hit
//   k_mg_runs      a lane per head: gathers its run by the keys' low bits, sums it with saturation (k_fold_runs' idea) and places it
//   k_mg_offsets   a lane per row: the heads before the row's first hit
// Every word of the output is written once, by a lane that is a function of the input, and saturating sums of non-negative integers do
// not depend on their order: bit-identical from call to call.  Integers only, bounded loops, pooled memory, no atomics but the check's
// figures, no kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <type_traits>
#include <vector>

#include "biosketch.h"
#include "host_types.hpp"
#include "search_internal.hpp"
#include "sets_internal.hpp"

#define MG_BLOCK 256

namespace {

enum { MG_MIN = 0, MG_MAX = 1, MG_UNSORTED = 2, MG_PART_WORDS = 3 };  // the figures of one part, one u64 word each
enum { MG_DUP = 0, MG_HEADS = 1, MG_SORT_WORDS = 2 };                 // the figures of the sort path

struct MgPart {  // one part as the kernels read it; a payload the RESULT does not carry is NULL
    const u64 *off;
    const u32 *tgt, *sh, *total;
    const u64 *dot, *msum;
    const u32 *members;
    u64 base, H;
};
struct MgOut {
    u32 *tgt, *sh, *total;
    u64 *dot, *msum;
    u32 *members;
};

inline unsigned bits_of(u64 x) { return x ? 64u - (unsigned)__builtin_clzll(x) : 0u; }

// one ballot per trip of a whole wavefront
__device__ __forceinline__ void mg_flag(bool bad, u64 *word) {
    const u64 m = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicOr(reinterpret_cast<u32 *>(word), 1u);
}

// the last q with off[q] <= i (off[0] = 0 <= i < off[nq]; rows without hits are passed over).  33 halvings cover nq < 2^32.
__device__ __forceinline__ u64 mg_row_of(const u64 *off, u64 nq, u64 i) {
    u64 lo = 0, hi = nq;
    for (int it = 0; it < 33 && hi - lo > 1; ++it) {
        const u64 mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(MG_BLOCK) void k_mg_check(const u64 *off, const u32 *tgt, u64 nq, u64 H, u64 *fig) {
    u32 lo = 0xFFFFFFFFu, hi = 0;
    for (u64 b = (u64)blockIdx.x * MG_BLOCK; b < H; b += (u64)gridDim.x * MG_BLOCK) {
        const u64 i = b + threadIdx.x;
        bool bad = false;
        if (i < H) {
            const u32 t = tgt[i];
            lo = t < lo ? t : lo;
            hi = t > hi ? t : hi;
            if (i && tgt[i - 1] >= t) bad = off[mg_row_of(off, nq, i)] != i;  // not above its predecessor: legal only where a row starts
        }
        mg_flag(bad, fig + MG_UNSORTED);
    }
    for (int d = 32; d; d >>= 1) {
        const u32 a = __shfl_xor(lo, d, 64), c = __shfl_xor(hi, d, 64);
        lo = a < lo ? a : lo;
        hi = c > hi ? c : hi;
    }
    if ((threadIdx.x & 63) == 0 && lo <= hi) {  // (a wavefront that saw no hit keeps lo > hi)
        atomicMin(reinterpret_cast<u32 *>(fig + MG_MIN), lo);
        atomicMax(reinterpret_cast<u32 *>(fig + MG_MAX), hi);
    }
}

// out[q] = the sum of the parts' offsets[q]; delta[p * nq + q] + i = the place of hit i of part p, a hit of row q
__global__ __launch_bounds__(MG_BLOCK) void k_mg_starts(const MgPart *parts, u32 P, u64 nq, u64 *out, u64 *delta) {
    for (u64 q = (u64)blockIdx.x * MG_BLOCK + threadIdx.x; q <= nq; q += (u64)gridDim.x * MG_BLOCK) {
        u64 run = 0;
        for (u32 p = 0; p < P && p < BSK_MERGE_MAX_PARTS; ++p) run += parts[p].off[q];
        out[q] = run;
        if (q == nq) continue;
        for (u32 p = 0; p < P && p < BSK_MERGE_MAX_PARTS; ++p) {
            const u64 a = parts[p].off[q];
            delta[(u64)p * nq + q] = run - a;  // (run holds a itself: no borrow)
            run += parts[p].off[q + 1] - a;
        }
    }
}

// key == NULL: the concat path, o is the result.  Else o is the scratch, the target goes into the key.
__global__ __launch_bounds__(MG_BLOCK) void k_mg_place(MgPart h, u64 nq, const u64 *delta, unsigned idx_bits, u64 *key, MgOut o) {
    for (u64 i = (u64)blockIdx.x * MG_BLOCK + threadIdx.x; i < h.H; i += (u64)gridDim.x * MG_BLOCK) {
        const u64 d = delta[mg_row_of(h.off, nq, i)] + i;  // (< the hits in total: the rows' places tile the output)
        const u64 t = (u64)h.tgt[i] + h.base;              // (< 2^32: the host has seen the part's largest target)
        if (key) key[d] = (t << idx_bits) | d;
        else o.tgt[d] = (u32)t;
        o.sh[d] = h.sh[i];
        if (h.total) o.total[d] = h.total[i];
        if (h.dot) {
            o.dot[d] = h.dot[i];
            o.msum[d] = h.msum[i];
        }
        if (h.members) o.members[d] = h.members[i];
    }
}

__global__ __launch_bounds__(MG_BLOCK) void k_mg_rows(const u64 *off, u64 nq, u32 *head) {
    for (u64 q = (u64)blockIdx.x * MG_BLOCK + threadIdx.x; q < nq; q += (u64)gridDim.x * MG_BLOCK)
        if (off[q + 1] > off[q]) head[off[q]] = 1u;
}

// head[j] comes in as "sorted hit j starts a row" (k_mg_rows) and leaves as "j starts a run"; lane j writes head[j] alone and reads no other
__global__ __launch_bounds__(MG_BLOCK) void k_mg_heads(const u64 *key, u64 H, unsigned idx_bits, u32 *head, u64 *fig) {
    for (u64 b = (u64)blockIdx.x * MG_BLOCK; b < H; b += (u64)gridDim.x * MG_BLOCK) {
        const u64 j = b + threadIdx.x;
        bool dup = false;
        if (j < H && !head[j]) {  // (j > 0: hit 0 starts a row)
            dup = (key[j] >> idx_bits) == (key[j - 1] >> idx_bits);
            head[j] = dup ? 0u : 1u;
        }
        mg_flag(dup, fig + MG_DUP);
    }
}

__device__ __forceinline__ u64 mg_sat_add(u64 a, u64 b) {
    const u64 s = a + b;
    return s < a ? ~0ULL : s;
}
__device__ __forceinline__ u32 mg_sat32(u64 x) { return x > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)x; }

// s: the placed, unsorted arrays (s.tgt unused); the key's low bits are a hit's place there
__global__ __launch_bounds__(MG_BLOCK) void k_mg_runs(const u64 *key, const u32 *head, const u64 *hpos, u64 H, unsigned idx_bits, MgOut s, MgOut o) {
    const u64 mask = (1ULL << idx_bits) - 1;  // (idx_bits <= 32)
    for (u64 j = (u64)blockIdx.x * MG_BLOCK + threadIdx.x; j < H; j += (u64)gridDim.x * MG_BLOCK) {
        if (!head[j]) continue;
        const u64 k0 = key[j], r = hpos[j];
        u64 src = k0 & mask;  // (< H: the keys are a permutation of those k_mg_place wrote)
        u64 sh = s.sh[src], total = s.total ? s.total[src] : 0, members = s.members ? s.members[src] : 0;  // (fewer than 2^32 terms below 2^32: no overflow of the u64)
        u64 dot = s.dot ? s.dot[src] : 0, msum = s.dot ? s.msum[src] : 0;
        for (u64 x = j + 1; x < H && !head[x]; ++x) {  // (at most H steps)
            src = key[x] & mask;
            sh += s.sh[src];
            if (s.total) total += s.total[src];
            if (s.members) members += s.members[src];
            if (s.dot) {
                dot = mg_sat_add(dot, s.dot[src]);
                msum = mg_sat_add(msum, s.msum[src]);
            }
        }
        o.tgt[r] = (u32)(k0 >> idx_bits);
        o.sh[r] = mg_sat32(sh);
        if (s.total) o.total[r] = mg_sat32(total);
        if (s.members) o.members[r] = mg_sat32(members);
        if (s.dot) {
            o.dot[r] = dot;
            o.msum[r] = msum;
        }
    }
}

// out[q] = the heads before row q's first hit (hpos[H] = their number)
__global__ __launch_bounds__(MG_BLOCK) void k_mg_offsets(const u64 *off, u64 nq, const u64 *hpos, u64 *out) {
    for (u64 q = (u64)blockIdx.x * MG_BLOCK + threadIdx.x; q <= nq; q += (u64)gridDim.x * MG_BLOCK) out[q] = hpos[off[q]];
}

inline unsigned mg_grid(const bsk_ctx *ctx, u64 items) { return grid_for(ctx, items, MG_BLOCK, 16); }

// the checks that need no device, in the header's order; *out is not looked into before the arguments are there
int mg_check_args(bsk_ctx *ctx, const bsk_hits *const *parts, const uint64_t *base, u32 n_parts, u32 flags, bsk_hits *const *out, u64 *hits) {
    static thread_local char msg[160];
    const char *why = nullptr;
    int rc = BSK_ERR_ARG;
    if (!ctx || !parts || !out) why = "null argument";
    else if (n_parts == 0 || n_parts > BSK_MERGE_MAX_PARTS) why = "n_parts is 0 or beyond BSK_MERGE_MAX_PARTS";
    else if (flags & ~(u32)BSK_MERGE_ADD) why = "unknown flag";
    if (!why) {
        u64 H = 0;
        for (u32 p = 0; p < n_parts && !why; ++p)
            if (!parts[p]) why = "null part";
        for (u32 p = 0; p < n_parts && !why; ++p)
            if (parts[p]->n_queries != parts[0]->n_queries) why = "the parts differ in their rows";
        for (u32 p = 0; p < n_parts && !why; ++p)
            if (*out == parts[p]) why = "the result slot holds one of the parts";
        if (!why && *out && (*out)->ctx != ctx) why = "the result belongs to another context";
        for (u32 p = 0; p < n_parts && !why; ++p)
            if (base && base[p] >= (1ULL << 32)) why = "a target_base of 2^32 or more";
        for (u32 p = 0; p < n_parts && !why; ++p) {
            if (parts[p]->n_hits >= (1ULL << 32)) H = 1ULL << 32;
            else if (H < (1ULL << 32)) H += parts[p]->n_hits;
        }
        if (!why && (parts[0]->n_queries >= (1ULL << 32) || H >= (1ULL << 32))) why = "2^32 rows or hits in total or more (merge fewer parts)", rc = BSK_ERR_UNSUPPORTED;
        *hits = H;
    }
    if (!why) return BSK_OK;
    snprintf(msg, sizeof msg, "bsk_hits_merge: %s", why);
    if (ctx) ctx->err = msg;
    return rc;
}

// what the device passes before the take-over leave for the ones behind it
struct MgWork {
    u32 P = 0;
    u64 nq = 0, H = 0, K = 0;  // rows, hits in total, hits of the result
    bool sort = false, has_total = false, has_weights = false, has_members = false;
    std::vector<MgPart> parts;
    MgPart *table = nullptr;
    u64 *fig = nullptr, *ooff = nullptr, *delta = nullptr;
    // the sort path
    unsigned idx_bits = 1;
    u64 *sfig = nullptr, *kin = nullptr, *kout = nullptr, *hpos = nullptr, *part = nullptr;
    u32 *head = nullptr;
    MgOut s{};
};

// a part of another device: its arrays once into the pool, by the peer copy bsk_index_attach uses
int mg_fetch_peers(bsk_ctx *ctx, const bsk_hits *const *parts, MgWork &w) {
    Carve c;
    std::vector<size_t> at_off(w.P, 0);
    bool any = false;
    for (u32 p = 0; p < w.P; ++p) {
        const bsk_hits *h = parts[p];
        if (!h->ctx || h->ctx->device == ctx->device) continue;
        any = true;
        at_off[p] = c.add<u64>(w.nq + 1);
        c.add<u32>(h->n_hits), c.add<u32>(h->n_hits);
        if (w.has_total) c.add<u32>(h->n_hits);
        if (w.has_weights) c.add<u64>(h->n_hits), c.add<u64>(h->n_hits);
        if (w.has_members) c.add<u32>(h->n_hits);
    }
    if (!any) return BSK_OK;
    char *b = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_MERGE_PEER, c.bytes, &b));
    for (u32 p = 0; p < w.P; ++p) {
        const bsk_hits *h = parts[p];
        if (!h->ctx || h->ctx->device == ctx->device) continue;
        const int src = h->ctx->device;
        MgPart &m = w.parts[p];
        Carve k;
        k.bytes = at_off[p];
        auto pull = [&](auto *&field, size_t n) -> hipError_t {  // (the carve above and this one add the same arrays in the same order)
            typedef std::remove_const_t<std::remove_pointer_t<std::remove_reference_t<decltype(field)>>> T;
            T *dst = at<T>(b, k.add<T>(n));
            const hipError_t e = n ? hipMemcpyPeer(dst, ctx->device, field, src, n * sizeof(T)) : hipSuccess;
            field = dst;
            return e;
        };
        HIPCHK(ctx, pull(m.off, w.nq + 1));
        HIPCHK(ctx, pull(m.tgt, h->n_hits));
        HIPCHK(ctx, pull(m.sh, h->n_hits));
        if (w.has_total) HIPCHK(ctx, pull(m.total, h->n_hits));
        if (w.has_weights) {
            HIPCHK(ctx, pull(m.dot, h->n_hits));
            HIPCHK(ctx, pull(m.msum, h->n_hits));
        }
        if (w.has_members) HIPCHK(ctx, pull(m.members, h->n_hits));
    }
    HIPCHK(ctx, hipDeviceSynchronize());
    return BSK_OK;
}

void mg_place_all(bsk_ctx *ctx, const MgWork &w, u64 *key, const MgOut &o) {
    for (u32 p = 0; p < w.P; ++p)
        if (w.parts[p].H)
            hipLaunchKernelGGL(k_mg_place, dim3(mg_grid(ctx, w.parts[p].H)), dim3(MG_BLOCK), 0, ctx->stream, w.parts[p], w.nq, (const u64 *)(w.delta + (u64)p * w.nq),
                               w.idx_bits, key, o);
}

// the sort path up to the number of output hits: in pool scratch, before the slot is taken over
int mg_sort_pass(bsk_ctx *ctx, MgWork &w, bool add) {
    hipStream_t st = ctx->stream;
    const u64 H = w.H, nq = w.nq;
    w.idx_bits = std::max(1u, bits_of(H - 1));
    size_t tb = 0;
    HIPCHK(ctx, sets_sort_segments_u64(nullptr, tb, nullptr, nullptr, H, nq, w.ooff, st));
    Carve c;
    const size_t o_fig = c.add<u64>(MG_SORT_WORDS), o_kin = c.add<u64>(H), o_kout = c.add<u64>(H), o_hpos = c.add<u64>(H + 1), o_part = c.add<u64>(scan_parts(H)),
                 o_head = c.add<u32>(H), o_sh = c.add<u32>(H), o_total = c.add<u32>(w.has_total ? H : 1), o_dot = c.add<u64>(w.has_weights ? H : 1),
                 o_msum = c.add<u64>(w.has_weights ? H : 1), o_members = c.add<u32>(w.has_members ? H : 1), o_tmp = c.add<char>(tb ? tb : 8);
    void *b = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_MERGE_SORT, c.bytes, &b));
    w.sfig = at<u64>(b, o_fig), w.kin = at<u64>(b, o_kin), w.kout = at<u64>(b, o_kout), w.hpos = at<u64>(b, o_hpos), w.part = at<u64>(b, o_part), w.head = at<u32>(b, o_head);
    w.s = MgOut{nullptr, at<u32>(b, o_sh), w.has_total ? at<u32>(b, o_total) : nullptr, w.has_weights ? at<u64>(b, o_dot) : nullptr,
                w.has_weights ? at<u64>(b, o_msum) : nullptr, w.has_members ? at<u32>(b, o_members) : nullptr};
    HIPCHK(ctx, hipMemsetAsync(w.sfig, 0, MG_SORT_WORDS * 8, st));
    HIPCHK(ctx, hipMemsetAsync(w.head, 0, H * 4, st));
    hipLaunchKernelGGL(k_mg_starts, dim3(mg_grid(ctx, nq + 1)), dim3(MG_BLOCK), 0, st, (const MgPart *)w.table, w.P, nq, w.ooff, w.delta);
    mg_place_all(ctx, w, w.kin, w.s);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, sets_sort_segments_u64(at<char>(b, o_tmp), tb, w.kin, w.kout, H, nq, w.ooff, st));
    hipLaunchKernelGGL(k_mg_rows, dim3(mg_grid(ctx, nq)), dim3(MG_BLOCK), 0, st, (const u64 *)w.ooff, nq, w.head);
    hipLaunchKernelGGL(k_mg_heads, dim3(mg_grid(ctx, H)), dim3(MG_BLOCK), 0, st, (const u64 *)w.kout, H, w.idx_bits, w.head, w.sfig);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, scan_counts(st, KeepOf{w.head}, H, w.part, w.hpos, w.sfig + MG_HEADS, (u64 *)nullptr));
    HIPCHK(ctx, read_back(ctx, w.sfig, MG_SORT_WORDS));
    if (ctx->h_pinned[MG_DUP] && !add) return fail_arg(ctx, "bsk_hits_merge: a row names a target twice (BSK_MERGE_ADD adds such hits up)");
    w.K = ctx->h_pinned[MG_HEADS];
    return BSK_OK;
}

// what runs on the object take_over hands over
int mg_impl(bsk_ctx *ctx, const MgWork &w, bsk_hits *res) {
    hipStream_t st = ctx->stream;
    const u64 nq = w.nq, k = w.K ? w.K : 1;
    res->n_queries = nq;
    res->n_hits = 0;
    res->n_large = 0;
    res->has_total = res->has_weights = res->has_members = false;
    HIPCHK(ctx, grow_array(&res->offsets, &res->c_offsets, (nq + 1) * 8));
    HIPCHK(ctx, grow_array(&res->target, &res->c_target, k * 4));
    HIPCHK(ctx, grow_array(&res->shared, &res->c_shared, k * 4));
    if (w.has_total) HIPCHK(ctx, grow_array(&res->total, &res->c_total, k * 4));
    if (w.has_weights) {
        HIPCHK(ctx, grow_array(&res->dot, &res->c_dot, k * 8));
        HIPCHK(ctx, grow_array(&res->msum, &res->c_msum, k * 8));
    }
    if (w.has_members) HIPCHK(ctx, grow_array(&res->members, &res->c_members, k * 4));
    const MgOut o{res->target, res->shared, w.has_total ? res->total : nullptr, w.has_weights ? res->dot : nullptr, w.has_weights ? res->msum : nullptr,
                  w.has_members ? res->members : nullptr};
    if (!w.H) {
        HIPCHK(ctx, hipMemsetAsync(res->offsets, 0, (nq + 1) * 8, st));
    } else if (!w.sort) {
        hipLaunchKernelGGL(k_mg_starts, dim3(mg_grid(ctx, nq + 1)), dim3(MG_BLOCK), 0, st, (const MgPart *)w.table, w.P, nq, res->offsets, w.delta);
        mg_place_all(ctx, w, nullptr, o);
        HIPCHK(ctx, hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_mg_runs, dim3(mg_grid(ctx, w.H)), dim3(MG_BLOCK), 0, st, (const u64 *)w.kout, (const u32 *)w.head, (const u64 *)w.hpos, w.H, w.idx_bits, w.s, o);
        hipLaunchKernelGGL(k_mg_offsets, dim3(mg_grid(ctx, nq + 1)), dim3(MG_BLOCK), 0, st, (const u64 *)w.ooff, nq, (const u64 *)w.hpos, res->offsets);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    res->n_hits = w.K;
    res->has_total = w.has_total;
    res->has_weights = w.has_weights;
    res->has_members = w.has_members;
    snprintf(res->plan, sizeof res->plan, "bsk_hits_merge: %s, path=%s parts=%u hits=%llu combined=%llu",
             w.sort ? "k_mg_check + k_mg_starts + k_mg_place + segmented sort + k_mg_heads + k_mg_runs + k_mg_offsets" : "k_mg_check + k_mg_starts + k_mg_place",
             w.sort ? "sort" : "concat", w.P, (unsigned long long)w.H, (unsigned long long)(w.H - w.K));
    return BSK_OK;
}

}  // namespace

extern "C" int bsk_hits_merge(bsk_ctx *ctx, const bsk_hits *const *parts, const uint64_t *target_base, uint32_t n_parts, uint32_t flags, bsk_hits **out) {
    MgWork w;
    int rc = mg_check_args(ctx, parts, target_base, n_parts, flags, out, &w.H);
    if (rc != BSK_OK) return rc;
    const bool add = (flags & BSK_MERGE_ADD) != 0;
    w.P = n_parts;
    w.nq = parts[0]->n_queries;
    w.has_total = w.has_weights = w.has_members = true;
    for (u32 p = 0; p < n_parts; ++p) {
        w.has_total &= parts[p]->has_total;
        w.has_weights &= parts[p]->has_weights;
        w.has_members &= parts[p]->has_members;
    }
    // a part of another context: its stream is synchronised on the host before anything of this context reads the part
    for (u32 p = 0; p < n_parts; ++p) {
        const bsk_ctx *pc = parts[p]->ctx;
        if (!pc || pc == ctx) continue;
        HIPCHK(ctx, hipSetDevice(pc->device));
        HIPCHK(ctx, hipStreamSynchronize(pc->stream));
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u64 nq = w.nq, H = w.H;
    w.K = H;
    if (H) {
        w.parts.resize(n_parts);
        for (u32 p = 0; p < n_parts; ++p) {
            const bsk_hits *h = parts[p];
            w.parts[p] = MgPart{h->offsets, h->target, h->shared, w.has_total ? h->total : nullptr, w.has_weights ? h->dot : nullptr, w.has_weights ? h->msum : nullptr,
                                w.has_members ? h->members : nullptr, target_base ? target_base[p] : 0, h->n_hits};
        }
        rc = mg_fetch_peers(ctx, parts, w);
        if (rc != BSK_OK) return rc;
        // the scratch every path needs, the table of the parts and the one pass over the hits that says which path it is
        std::vector<u64> fig((size_t)n_parts * MG_PART_WORDS, 0);
        for (u32 p = 0; p < n_parts; ++p) fig[(size_t)p * MG_PART_WORDS + MG_MIN] = 0xFFFFFFFFull;
        Carve c;
        const size_t o_fig = c.add<u64>(fig.size()), o_table = c.add<MgPart>(n_parts), o_ooff = c.add<u64>(nq + 1), o_delta = c.add<u64>((u64)n_parts * nq);
        void *b = nullptr;
        HIPCHK(ctx, ctx_pool(ctx, SLOT_MERGE_WORK, c.bytes, &b));
        w.fig = at<u64>(b, o_fig), w.table = at<MgPart>(b, o_table), w.ooff = at<u64>(b, o_ooff), w.delta = at<u64>(b, o_delta);
        HIPCHK(ctx, hipMemcpyAsync(w.fig, fig.data(), fig.size() * 8, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(w.table, w.parts.data(), n_parts * sizeof(MgPart), hipMemcpyHostToDevice, st));
        for (u32 p = 0; p < n_parts; ++p)
            if (w.parts[p].H)
                hipLaunchKernelGGL(k_mg_check, dim3(mg_grid(ctx, w.parts[p].H)), dim3(MG_BLOCK), 0, st, w.parts[p].off, w.parts[p].tgt, nq, w.parts[p].H,
                                   w.fig + (size_t)p * MG_PART_WORDS);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(fig.data(), w.fig, fig.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        // concat: every part's rows ascend and the shifted ranges of the non-empty parts are disjoint and increase with p
        u64 top = 0;
        bool first = true;
        for (u32 p = 0; p < n_parts; ++p) {
            if (!w.parts[p].H) continue;
            const u64 *f = &fig[(size_t)p * MG_PART_WORDS];
            const u64 lo = (u32)f[MG_MIN] + w.parts[p].base, hi = (u32)f[MG_MAX] + w.parts[p].base;
            if (hi >= (1ULL << 32)) {
                ctx->err = "bsk_hits_merge: a target_base + target of 2^32 or more";
                return BSK_ERR_UNSUPPORTED;
            }
            if ((u32)f[MG_UNSORTED] || (!first && lo <= top)) w.sort = true;
            top = first || hi > top ? hi : top;
            first = false;
        }
        if (w.sort) {
            rc = mg_sort_pass(ctx, w, add);
            if (rc != BSK_OK) return rc;
        }
    }
    return take_over(ctx, out, bsk_hits_release, [&](bsk_hits *res, bool) { return mg_impl(ctx, w, res); });
}
