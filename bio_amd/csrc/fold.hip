// fold.hip -- hits folded by target group (include/biosketch.h "window sets and folded hits"): the hits against an index of genome
// chunks list chunks; bsk_hits_fold sums them per genome and counts how many chunks of a genome a row hit (kmcp's
// --min-chunks-fraction), where the hits already are.
//
// Groups are runs of consecutive targets and the targets of a row are strictly ascending, so the hits of one group are a contiguous
// run of their row.
//   k_fold_map    a lane per target: its group by a search in the group offsets -> a u32 map (one load per hit afterwards instead of a
//                 search of ~log2(groups) dependent loads per hit)
//   k_fold_rows   a lane per row: marks the row's first hit
//   k_fold_check  a lane per hit: refuses a target beyond the last group and a target not above its predecessor in the row; a hit is
//                 a HEAD where its row starts or its group differs from its predecessor's.  Runs before the result slot is taken over.
//   scan_counts   over the heads -> the run number of every head, and the number of runs
//   k_fold_runs   a lane per head: the owner walks its run (a genome of thousands of contigs hit by one query is a run longer than a
//                 workgroup: the walk is sequential, but nothing is added into shared words), sums shared with saturation, counts the
//                 members and decides whether the run is kept
//   scan_counts   over the kept flags -> the place of every kept run
//   k_fold_place  a lane per run: the kept ones to their places; k_fold_offsets, a lane per row: the kept runs before the row's first hit
// Every word of the output is written once, by a lane that is a function of the input: bit-identical from call to call.  Integers
// only, bounded loops, no atomics but the one "bad input" flag, no kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "biosketch.h"
#include "host_types.hpp"
#include "search_internal.hpp"
#include "sets_internal.hpp"

#define FOLD_BLOCK 256

namespace {

enum { FOLD_BAD = 0, FOLD_RUNS = 1, FOLD_KEPT = 2, FOLD_WORDS = 4 };  // the figures, one u64 word each
enum : u32 { FOLD_BAD_TARGET = 1, FOLD_BAD_ORDER = 2 };

struct FoldRule {
    u32 min_members, frac_num, frac_den;
};

__global__ __launch_bounds__(FOLD_BLOCK) void k_fold_map(const u64 *goff, u64 ng, u64 nt, u32 *map) {
    for (u64 t = (u64)blockIdx.x * FOLD_BLOCK + threadIdx.x; t < nt; t += (u64)gridDim.x * FOLD_BLOCK) {
        // the last g with goff[g] <= t (goff[0] = 0 <= t < goff[ng]; empty groups are passed over).  33 halvings cover ng < 2^32.
        u64 lo = 0, hi = ng;
        for (int it = 0; it < 33 && hi - lo > 1; ++it) {
            const u64 mid = (lo + hi) >> 1;
            if (goff[mid] <= t) lo = mid;
            else hi = mid;
        }
        map[t] = (u32)lo;
    }
}

__global__ __launch_bounds__(FOLD_BLOCK) void k_fold_rows(const u64 *off, u64 nq, u32 *head) {
    for (u64 q = (u64)blockIdx.x * FOLD_BLOCK + threadIdx.x; q < nq; q += (u64)gridDim.x * FOLD_BLOCK)
        if (off[q + 1] > off[q]) head[off[q]] = 1u;
}

// head[i] comes in as "hit i starts a row" (k_fold_rows) and leaves as "hit i starts a run"; lane i writes head[i] alone and reads no other
__global__ __launch_bounds__(FOLD_BLOCK) void k_fold_check(const u32 *tgt, u64 H, const u32 *map, u64 nt, u32 *head, u64 *fig) {
    const int lane = threadIdx.x & 63;
    for (u64 b = (u64)blockIdx.x * FOLD_BLOCK; b < H; b += (u64)gridDim.x * FOLD_BLOCK) {
        const u64 i = b + threadIdx.x;
        u32 bad = 0;
        if (i < H) {
            const u32 t = tgt[i];
            const bool row_start = head[i] != 0;
            if ((u64)t >= nt) {
                bad = FOLD_BAD_TARGET;
            } else if (!row_start) {
                const u32 p = tgt[i - 1];  // (i > 0: hit 0 starts a row)
                if (p >= t) bad = FOLD_BAD_ORDER;  // (p < t < nt from here: both map reads are inside the map)
                else head[i] = map[p] != map[t] ? 1u : 0u;
            }
        }
        const u64 mt = __ballot(bad == FOLD_BAD_TARGET), mo = __ballot(bad == FOLD_BAD_ORDER);
        if (lane == 0 && (mt | mo)) atomicOr(reinterpret_cast<u32 *>(fig + FOLD_BAD), (mt ? (u32)FOLD_BAD_TARGET : 0u) | (mo ? (u32)FOLD_BAD_ORDER : 0u));
    }
}

__global__ __launch_bounds__(FOLD_BLOCK) void k_fold_runs(const u32 *tgt, const u32 *shared, const u32 *head, const u64 *hpos, u64 H, const u32 *map, const u64 *goff,
                                                          FoldRule rule, u32 *rgroup, u32 *rshared, u32 *rmembers, u32 *keep) {
    for (u64 i = (u64)blockIdx.x * FOLD_BLOCK + threadIdx.x; i < H; i += (u64)gridDim.x * FOLD_BLOCK) {
        if (!head[i]) continue;
        u64 sum = shared[i], m = 1;
        for (u64 j = i + 1; j < H && !head[j]; ++j) {  // (at most H steps)
            sum += shared[j];  // (fewer than 2^32 terms below 2^32: no overflow of the u64)
            ++m;
        }
        const u32 g = map[tgt[i]];
        const u64 size = goff[g + 1] - goff[g], r = hpos[i];
        rgroup[r] = g;
        rshared[r] = sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)sum;
        rmembers[r] = (u32)m;  // (distinct targets of one group: at most its size, at most 2^32 - 1 hits anyway)
        keep[r] = (m >= rule.min_members && (rule.frac_den == 0 || m * rule.frac_den >= (u64)rule.frac_num * size)) ? 1u : 0u;
    }
}

__global__ __launch_bounds__(FOLD_BLOCK) void k_fold_place(const u32 *rgroup, const u32 *rshared, const u32 *rmembers, const u32 *keep, const u64 *kpos, u64 R, u32 *otgt,
                                                           u32 *oshared, u32 *omembers) {
    for (u64 r = (u64)blockIdx.x * FOLD_BLOCK + threadIdx.x; r < R; r += (u64)gridDim.x * FOLD_BLOCK) {
        if (!keep[r]) continue;
        const u64 k = kpos[r];
        otgt[k] = rgroup[r];
        oshared[k] = rshared[r];
        omembers[k] = rmembers[r];
    }
}

// out[q] = the kept runs before row q's first hit: a row's first hit is a head, hpos of it is the row's first run (hpos[H] = R, kpos[R] = K)
__global__ __launch_bounds__(FOLD_BLOCK) void k_fold_offsets(const u64 *off, u64 nq, const u64 *hpos, const u64 *kpos, u64 *out) {
    for (u64 q = (u64)blockIdx.x * FOLD_BLOCK + threadIdx.x; q <= nq; q += (u64)gridDim.x * FOLD_BLOCK) out[q] = kpos[hpos[off[q]]];
}

inline unsigned fold_grid(const bsk_ctx *ctx, u64 items) { return grid_for(ctx, items, FOLD_BLOCK, 16); }

// the scratch of one call: taken from the pool ONCE, before the first launch (a pool buffer that grows moves); the runs are at most the hits
struct FoldScratch {
    u64 *fig = nullptr, *goff = nullptr, *hpos = nullptr, *kpos = nullptr, *part = nullptr;
    u32 *head = nullptr, *rgroup = nullptr, *rshared = nullptr, *rmembers = nullptr, *keep = nullptr, *map = nullptr;
};

int fold_scratch(bsk_ctx *ctx, u64 ng, u64 nt, u64 H, FoldScratch &s) {
    Carve c;
    const size_t o_fig = c.add<u64>(FOLD_WORDS), o_goff = c.add<u64>(ng + 1), o_hpos = c.add<u64>(H + 1), o_kpos = c.add<u64>(H + 1), o_part = c.add<u64>(scan_parts(H)),
                 o_head = c.add<u32>(H), o_rgroup = c.add<u32>(H), o_rshared = c.add<u32>(H), o_rmembers = c.add<u32>(H), o_keep = c.add<u32>(H);
    void *b = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_FOLD_WORK, c.bytes, &b));
    HIPCHK(ctx, ctx_pool(ctx, SLOT_FOLD_MAP, (nt ? nt : 1) * 4, &s.map));
    s.fig = at<u64>(b, o_fig), s.goff = at<u64>(b, o_goff), s.hpos = at<u64>(b, o_hpos), s.kpos = at<u64>(b, o_kpos), s.part = at<u64>(b, o_part);
    s.head = at<u32>(b, o_head), s.rgroup = at<u32>(b, o_rgroup), s.rshared = at<u32>(b, o_rshared), s.rmembers = at<u32>(b, o_rmembers), s.keep = at<u32>(b, o_keep);
    return BSK_OK;
}

// what runs on the object take_over hands over: the heads are marked and scanned, R runs
int fold_impl(bsk_ctx *ctx, const bsk_hits *h, const FoldScratch &s, u64 ng, u64 R, const FoldRule &rule, bsk_hits *res) {
    hipStream_t st = ctx->stream;
    const u64 nq = h->n_queries, H = h->n_hits;
    res->n_queries = nq;
    res->n_hits = 0;
    res->n_large = 0;
    res->has_total = false;
    res->has_weights = false;
    res->has_members = false;
    HIPCHK(ctx, grow_array(&res->offsets, &res->c_offsets, (nq + 1) * 8));
    u64 K = 0;
    if (R) {
        hipLaunchKernelGGL(k_fold_runs, dim3(fold_grid(ctx, H)), dim3(FOLD_BLOCK), 0, st, (const u32 *)h->target, (const u32 *)h->shared, (const u32 *)s.head,
                           (const u64 *)s.hpos, H, (const u32 *)s.map, (const u64 *)s.goff, rule, s.rgroup, s.rshared, s.rmembers, s.keep);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, scan_counts(st, KeepOf{s.keep}, R, s.part, s.kpos, s.fig + FOLD_KEPT, (u64 *)nullptr));
        HIPCHK(ctx, read_back(ctx, s.fig + FOLD_KEPT, 1));
        K = ctx->h_pinned[0];
    }
    HIPCHK(ctx, grow_array(&res->target, &res->c_target, (K ? K : 1) * 4));
    HIPCHK(ctx, grow_array(&res->shared, &res->c_shared, (K ? K : 1) * 4));
    HIPCHK(ctx, grow_array(&res->members, &res->c_members, (K ? K : 1) * 4));
    if (R) {
        hipLaunchKernelGGL(k_fold_place, dim3(fold_grid(ctx, R)), dim3(FOLD_BLOCK), 0, st, (const u32 *)s.rgroup, (const u32 *)s.rshared, (const u32 *)s.rmembers,
                           (const u32 *)s.keep, (const u64 *)s.kpos, R, res->target, res->shared, res->members);
        hipLaunchKernelGGL(k_fold_offsets, dim3(fold_grid(ctx, nq + 1)), dim3(FOLD_BLOCK), 0, st, (const u64 *)h->offsets, nq, (const u64 *)s.hpos, (const u64 *)s.kpos,
                           res->offsets);
        HIPCHK(ctx, hipGetLastError());
    } else {
        HIPCHK(ctx, hipMemsetAsync(res->offsets, 0, (nq + 1) * 8, st));
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    res->n_hits = K;
    res->has_members = true;
    snprintf(res->plan, sizeof res->plan, "bsk_hits_fold: k_fold_map + k_fold_check + k_fold_runs + k_fold_place, groups=%llu runs=%llu kept=%llu", (unsigned long long)ng,
             (unsigned long long)R, (unsigned long long)K);
    return BSK_OK;
}

}  // namespace

extern "C" int bsk_hits_fold(bsk_ctx *ctx, const bsk_hits *h, const uint64_t *group_offsets, uint64_t n_groups, const bsk_fold_params *fp, bsk_hits **out) {
    if (!ctx || !h || !group_offsets || !out) return fail_arg(ctx, "bsk_hits_fold: null argument");
    if (fp && fp->flags != 0) return fail_arg(ctx, "bsk_hits_fold: unknown flag");
    if (fp && fp->frac_den != 0 && fp->frac_num > fp->frac_den) return fail_arg(ctx, "bsk_hits_fold: frac_num > frac_den");
    if (h->ctx != ctx || (*out && (*out)->ctx != ctx)) return fail_arg(ctx, "bsk_hits_fold: the hits belong to another context");
    if (*out == h) return fail_arg(ctx, "bsk_hits_fold: *out is h itself");
    if (n_groups >= (1ULL << 32)) return fail_arg(ctx, "bsk_hits_fold: 2^32 groups or more");
    if (group_offsets[0] != 0) return fail_arg(ctx, "bsk_hits_fold: group_offsets[0] != 0");
    for (u64 g = 0; g < n_groups; ++g)
        if (group_offsets[g + 1] < group_offsets[g]) return fail_arg(ctx, "bsk_hits_fold: group_offsets decrease");
    const u64 nt = group_offsets[n_groups];
    if (nt > (1ULL << 32)) return fail_arg(ctx, "bsk_hits_fold: more than 2^32 targets in the groups");
    const u64 nq = h->n_queries, H = h->n_hits;
    if (nq >= (1ULL << 32) || H >= (1ULL << 32)) {
        ctx->err = "bsk_hits_fold: 2^32 rows or hits or more (split the hits)";
        return BSK_ERR_UNSUPPORTED;
    }
    const FoldRule rule{fp && fp->min_members ? fp->min_members : 1u, fp ? fp->frac_num : 0u, fp ? fp->frac_den : 0u};
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the scratch, the map and the one pass over the hits that can refuse them: before the slot is taken over, *out stays as it was
    hipStream_t st = ctx->stream;
    FoldScratch s;
    u64 R = 0;
    if (H) {
        const int rc = fold_scratch(ctx, n_groups, nt, H, s);
        if (rc != BSK_OK) return rc;
        HIPCHK(ctx, hipMemsetAsync(s.fig, 0, FOLD_WORDS * 8, st));
        HIPCHK(ctx, hipMemsetAsync(s.head, 0, H * 4, st));
        HIPCHK(ctx, hipMemcpyAsync(s.goff, group_offsets, (n_groups + 1) * 8, hipMemcpyHostToDevice, st));
        if (nt) hipLaunchKernelGGL(k_fold_map, dim3(fold_grid(ctx, nt)), dim3(FOLD_BLOCK), 0, st, (const u64 *)s.goff, n_groups, nt, s.map);
        hipLaunchKernelGGL(k_fold_rows, dim3(fold_grid(ctx, nq)), dim3(FOLD_BLOCK), 0, st, (const u64 *)h->offsets, nq, s.head);
        hipLaunchKernelGGL(k_fold_check, dim3(fold_grid(ctx, H)), dim3(FOLD_BLOCK), 0, st, (const u32 *)h->target, H, (const u32 *)s.map, nt, s.head, s.fig);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, scan_counts(st, KeepOf{s.head}, H, s.part, s.hpos, s.fig + FOLD_RUNS, (u64 *)nullptr));
        HIPCHK(ctx, read_back(ctx, s.fig + FOLD_BAD, 2));  // (synchronises: group_offsets is not read after this)
        if (ctx->h_pinned[0] & FOLD_BAD_TARGET) return fail_arg(ctx, "bsk_hits_fold: a target >= group_offsets[n_groups]");
        if (ctx->h_pinned[0] & FOLD_BAD_ORDER) return fail_arg(ctx, "bsk_hits_fold: targets not strictly ascending inside a row (the output of bsk_hits_top is not)");
        R = ctx->h_pinned[1];
    }
    return take_over(ctx, out, bsk_hits_release, [&](bsk_hits *res, bool) { return fold_impl(ctx, h, s, n_groups, R, rule, res); });
}

extern "C" int bsk_hits_members_device(const bsk_hits *h, const uint32_t **members) {
    if (!h) return BSK_ERR_ARG;
    if (members) *members = h->has_members ? (const uint32_t *)h->members : nullptr;
    return BSK_OK;
}

extern "C" int bsk_hits_fetch_members(bsk_ctx *ctx, const bsk_hits *h, uint64_t first, uint64_t count, uint32_t *members, uint64_t hit_cap) {
    if (!ctx || !h || !members) return fail_arg(ctx, "bsk_hits_fetch_members: null argument");
    if (h->ctx != ctx) return fail_arg(ctx, "bsk_hits_fetch_members: the hits belong to another context");
    if (!h->has_members) return fail_arg(ctx, "bsk_hits_fetch_members: the hits carry no members (bsk_hits_fold makes such)");
    if (first > h->n_queries || count > h->n_queries - first) return fail_arg(ctx, "bsk_hits_fetch_members: range outside the hits");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, h->offsets + first, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned + 1, h->offsets + first + count, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const u64 o0 = ctx->h_pinned[0], nh = ctx->h_pinned[1] - o0;
    if (nh > hit_cap) return fail_arg(ctx, "bsk_hits_fetch_members: hit_cap too small");
    if (nh) HIPCHK(ctx, hipMemcpyAsync(members, h->members + o0, nh * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BSK_OK;
}
