// select.hip -- hits selected by a measure (include/biosketch.h "hits selected by a measure"): bsk_hits_filter keeps the hits whose
// measure reaches a threshold, bsk_hits_top_by every row's n hits of largest measure.  Both carry every payload of their input.
//
// A measure is an exact fraction N/D of two 128-bit integers (sel_nd: the table of the header); two fractions are compared by their
// cross products in 256 bits (wide_uint.hpp).  Integers only.
//   k_sel_check    a lane per hit: refuses a target beyond the target norms and a denominator that is not positive; for the filter it
//                  also writes the hit's keep flag (the flag pass and the check are one pass).  Runs before the result slot is taken over.
//   scan_counts    over the keep flags -> the place of every kept hit
//   k_sel_place    a lane per hit: the kept ones to their places, every array; k_sel_offsets, a lane per row: the scan at the old offset
//   k_tb_classes   a lane per row: how many rows each of the three paths below takes
//   k_tb_group     rows of at most 16 hits, a group of 16 lanes each: a lane's hit goes to the place (number of better hits of the group)
//   k_tb_lds       rows of 17 .. 1 024 hits, a wavefront each: the hit indices sorted in LDS on the bitonic network, with the comparator
//   k_tb_global    longer rows, a workgroup each: the same network over a u32 index array in pooled global memory, __syncthreads()
//                  between the steps; indices beyond the row compare as worst
// The three gather every array by the sorted indices themselves.  Every word of the output is written once, by a lane that is a function
// of the input: bit-identical from call to call.  Bounded loops, no atomics but the "bad input" flag and the class counts, no kernel
// waits for another workgroup.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "biosketch.h"
#include "host_types.hpp"
#include "search_internal.hpp"
#include "sets_internal.hpp"
#include "wide_uint.hpp"

#define SEL_BLOCK 256
#define TB_GROUP 16    // hits a group of 16 lanes ranks in registers, one per lane (as k_top_group)
#define TB_LDS 1024    // hit indices one wavefront sorts in LDS: 4 KB
#define TB_WAVES 4     // wavefronts per workgroup of k_tb_lds
#define TB_PAD 0xFFFFFFFFu  // an index beyond the row: worse than every hit

namespace {

typedef bsk_u128 u128;

// the figures, one u64 word each: [0] bad input, [1] hits kept; bsk_hits_top_by: [2] hits kept, [3] u32 of the global path's index
// arrays, [4] [5] [6] rows of the group, LDS and global path
enum { SEL_BAD = 0, SEL_KEPT = 1, TB_KEPT = 2, TB_INDEX = 3, TB_CLASSES = 4, SEL_WORDS = 8 };
enum : u32 { SEL_BAD_TARGET = 1, SEL_BAD_DEN = 2 };
enum : u32 { NEED_Q = 1, NEED_T = 2, NEED_WEIGHTS = 4, NEED_MEMBERS = 8 };

struct SelHits {  // the input; a payload it does not carry is NULL
    const u64 *off;
    const u32 *tgt, *sh, *total;
    const u64 *dot, *msum;
    const u32 *members;
    u64 nq, H;
};
struct SelOut {
    u32 *tgt, *sh, *total;
    u64 *dot, *msum;
    u32 *members;
};
struct SelMeasure {
    u32 kind, need;
    const u64 *qn, *tn;  // device copies of the call's norms
    u64 n_tn;
};
struct SelRule {  // kept iff N * a >= b * D
    u128 a, b;
};

// the last q with off[q] <= i (off[0] = 0 <= i < off[nq]; rows without hits are passed over).  33 halvings cover nq < 2^32.
__device__ __forceinline__ u64 sel_row_of(const u64 *off, u64 nq, u64 i) {
    u64 lo = 0, hi = nq;
    for (int it = 0; it < 33 && hi - lo > 1; ++it) {
        const u64 mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// N and D of hit i of row q; != 0: why the hit has none (N / D is then 0 / 1, and nothing outside the arrays was read)
__device__ __forceinline__ u32 sel_nd(const SelHits &h, const SelMeasure &m, u64 q, u64 i, u128 &N, u128 &D) {
    N = 0;
    D = 1;
    u64 Q = 0, T = 0;
    if (m.need & NEED_Q) Q = m.qn[q];
    if (m.need & NEED_T) {
        const u32 t = h.tgt[i];
        if ((u64)t >= m.n_tn) return SEL_BAD_TARGET;
        T = m.tn[t];
    }
    const u128 sum = (u128)Q + T;  // (65 bits)
    u128 n = 0, d = 1;
    bool ok = true;
    switch (m.kind) {
        case BSK_MEASURE_SHARED: n = h.sh[i]; break;
        case BSK_MEASURE_MEMBERS: n = h.members[i]; break;
        case BSK_MEASURE_DOT: n = h.dot[i]; break;
        case BSK_MEASURE_MIN_SUM: n = h.msum[i]; break;
        case BSK_MEASURE_QUERY_COV: n = h.sh[i], d = Q; break;
        case BSK_MEASURE_TARGET_COV: n = h.sh[i], d = T; break;
        case BSK_MEASURE_JACCARD:
            n = h.sh[i];
            if (h.total) d = h.total[i];
            else ok = sum >= n, d = sum - n;
            break;
        case BSK_MEASURE_COSINE: n = (u128)h.dot[i] * h.dot[i], d = (u128)Q * T; break;
        case BSK_MEASURE_WEIGHTED_JACCARD: n = h.msum[i], ok = sum >= n, d = sum - n; break;
        case BSK_MEASURE_BC_SIMILARITY: n = (u128)h.msum[i] * 2, d = sum; break;
        default: n = h.dot[i], d = Q; break;  // BSK_MEASURE_QUERY_MASS (the host refuses every other kind)
    }
    if (!ok || d == 0) return SEL_BAD_DEN;
    N = n;
    D = d;
    return 0;
}

// hit a (Na / Da, target ta) before hit b: the larger measure, ties by ascending target
__device__ __forceinline__ bool tb_better(u128 na, u128 da, u32 ta, u128 nb, u128 db, u32 tb) {
    const int c = wide_frac_cmp(na, da, nb, db);
    return c > 0 || (c == 0 && ta < tb);
}

template <bool FILTER>
__global__ __launch_bounds__(SEL_BLOCK) void k_sel_check(SelHits h, SelMeasure m, SelRule r, u32 *keep, u64 *fig) {
    const int lane = threadIdx.x & 63;
    for (u64 b = (u64)blockIdx.x * SEL_BLOCK; b < h.H; b += (u64)gridDim.x * SEL_BLOCK) {
        const u64 i = b + threadIdx.x;
        u32 bad = 0;
        if (i < h.H) {
            const u64 q = (m.need & NEED_Q) ? sel_row_of(h.off, h.nq, i) : 0;
            u128 N, D;
            bad = sel_nd(h, m, q, i, N, D);
            if (FILTER) keep[i] = (!bad && wide_cmp(wide_mul(N, r.a), wide_mul(r.b, D)) >= 0) ? 1u : 0u;
        }
        const u64 mt = __ballot(bad == SEL_BAD_TARGET), md = __ballot(bad == SEL_BAD_DEN);
        if (lane == 0 && (mt | md)) atomicOr(reinterpret_cast<u32 *>(fig + SEL_BAD), (mt ? (u32)SEL_BAD_TARGET : 0u) | (md ? (u32)SEL_BAD_DEN : 0u));
    }
}

// hit src of the input to place dst of the output: every array the input carries
__device__ __forceinline__ void sel_copy(const SelHits &h, const SelOut &o, u64 src, u64 dst) {
    o.tgt[dst] = h.tgt[src];
    o.sh[dst] = h.sh[src];
    if (h.total) o.total[dst] = h.total[src];
    if (h.dot) {
        o.dot[dst] = h.dot[src];
        o.msum[dst] = h.msum[src];
    }
    if (h.members) o.members[dst] = h.members[src];
}

__global__ __launch_bounds__(SEL_BLOCK) void k_sel_place(SelHits h, const u32 *keep, const u64 *kpos, SelOut o) {
    for (u64 i = (u64)blockIdx.x * SEL_BLOCK + threadIdx.x; i < h.H; i += (u64)gridDim.x * SEL_BLOCK)
        if (keep[i]) sel_copy(h, o, i, kpos[i]);
}

// out[q] = the kept hits before row q's first hit (kpos[H] = the kept hits of all rows)
__global__ __launch_bounds__(SEL_BLOCK) void k_sel_offsets(const u64 *off, u64 nq, const u64 *kpos, u64 *out) {
    for (u64 q = (u64)blockIdx.x * SEL_BLOCK + threadIdx.x; q <= nq; q += (u64)gridDim.x * SEL_BLOCK) out[q] = kpos[off[q]];
}

// ---- the n best hits of every row by a measure ----
__device__ __forceinline__ u64 tb_pow2(u64 c) { return c <= 1 ? 1 : 1ULL << (64 - __builtin_clzll(c - 1)); }  // (c < 2^32)
struct TbCnt {  // what a row keeps: min(n, its hits)
    const u64 *off;
    u64 n;
    __device__ __forceinline__ u64 operator()(u64 q) const {
        const u64 c = off[q + 1] - off[q];
        return c < n ? c : n;
    }
};
struct TbPadOf {  // rows beyond one wavefront's LDS: the entries of their index array
    const u64 *off;
    __device__ __forceinline__ u64 operator()(u64 q) const {
        const u64 c = off[q + 1] - off[q];
        return c > TB_LDS ? tb_pow2(c) : 0;
    }
};
__global__ __launch_bounds__(SEL_BLOCK) void k_tb_classes(const u64 *off, u64 nq, u64 *cnt) {
    u32 g = 0, w = 0, l = 0;
    for (u64 q = (u64)blockIdx.x * SEL_BLOCK + threadIdx.x; q < nq; q += (u64)gridDim.x * SEL_BLOCK) {
        const u64 c = off[q + 1] - off[q];
        g += c >= 1 && c <= TB_GROUP;
        w += c > TB_GROUP && c <= TB_LDS;
        l += c > TB_LDS;
    }
    for (int d = 32; d; d >>= 1) {
        g += __shfl_xor(g, d, 64);
        w += __shfl_xor(w, d, 64);
        l += __shfl_xor(l, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (g) atomicAdd((unsigned long long *)cnt, (unsigned long long)g);
        if (w) atomicAdd((unsigned long long *)cnt + 1, (unsigned long long)w);
        if (l) atomicAdd((unsigned long long *)cnt + 2, (unsigned long long)l);
    }
}

__device__ __forceinline__ u128 tb_shfl16(u128 x, int j) {
    const u64 lo = __shfl((u64)x, j, 16), hi = __shfl((u64)(x >> 64), j, 16);
    return ((u128)hi << 64) | lo;
}
__global__ __launch_bounds__(SEL_BLOCK) void k_tb_group(SelHits h, SelMeasure m, u32 n, const u64 *toff, SelOut o) {
    const u64 wave = ((u64)blockIdx.x * SEL_BLOCK + threadIdx.x) >> 6, nw = ((u64)gridDim.x * SEL_BLOCK) >> 6;
    const u32 l = threadIdx.x & 15, g = (threadIdx.x & 63) >> 4;
    for (u64 q0 = wave * 4; q0 < h.nq; q0 += nw * 4) {  // (the whole wavefront stays in step: the shuffles read every lane)
        const u64 q = q0 + g;
        u64 a = 0, c = 0;
        if (q < h.nq) {
            a = h.off[q];
            c = h.off[q + 1] - a;
        }
        if (c > TB_GROUP) c = 0;  // another path's row
        const bool mine = l < c;
        u128 N = 0, D = 1;
        u32 t = 0;
        if (mine) {
            t = h.tgt[a + l];
            (void)sel_nd(h, m, q, a + l, N, D);
        }
        u32 rank = 0;
#pragma unroll
        for (int j = 0; j < TB_GROUP; ++j) {
            const u128 nj = tb_shfl16(N, j), dj = tb_shfl16(D, j);
            const u32 tj = __shfl(t, j, 16);
            rank += (u64)j < c && tb_better(nj, dj, tj, N, D, t);
        }
        if (mine && rank < n) sel_copy(h, o, a + l, toff[q] + rank);
    }
}

// index x of row q (first hit a) before index y
__device__ __forceinline__ bool tb_before(const SelHits &h, const SelMeasure &m, u64 q, u64 a, u32 x, u32 y) {
    if (x == TB_PAD) return false;
    if (y == TB_PAD) return true;
    u128 nx, dx, ny, dy;
    (void)sel_nd(h, m, q, a + x, nx, dx);
    (void)sel_nd(h, m, q, a + y, ny, dy);
    return tb_better(nx, dx, h.tgt[a + x], ny, dy, h.tgt[a + y]);
}
// idx[0 .. c2) <- the indices of the row's c hits, best first, the pads behind them; c2 a power of two >= c.  BLOCK: the lanes are a
// workgroup and idx is global memory, else a wavefront and idx is its LDS.  Every lane of the team runs every step.
template <bool BLOCK>
__device__ __forceinline__ void tb_sort(const SelHits &h, const SelMeasure &m, u64 q, u64 a, u32 *idx, u64 c, u64 c2, u32 tid, u32 team) {
    for (u64 i = tid; i < c2; i += team) idx[i] = i < c ? (u32)i : TB_PAD;
    if (BLOCK) __syncthreads();
    else wave_sync_lds();
    for (u64 k = 2; k <= c2; k <<= 1) {
        for (u64 j = k >> 1; j > 0; j >>= 1) {
            for (u64 e = tid; e < (c2 >> 1); e += team) {  // pair e of the step: i without bit j, its partner with it
                const u64 i = ((e & ~(j - 1)) << 1) | (e & (j - 1)), p = i | j;
                const u32 x = idx[i], y = idx[p];
                const bool up = (i & k) == 0;
                if (up ? tb_before(h, m, q, a, y, x) : tb_before(h, m, q, a, x, y)) {
                    idx[i] = y;
                    idx[p] = x;
                }
            }
            if (BLOCK) __syncthreads();
            else wave_sync_lds();
        }
    }
}

__global__ __launch_bounds__(64 * TB_WAVES) void k_tb_lds(SelHits h, SelMeasure m, u32 n, const u64 *toff, SelOut o) {
    __shared__ u32 lds[TB_WAVES][TB_LDS];
    u32 *idx = lds[threadIdx.x >> 6];
    const u32 lane = threadIdx.x & 63;
    const u64 wave = ((u64)blockIdx.x * (64 * TB_WAVES) + threadIdx.x) >> 6, nw = ((u64)gridDim.x * (64 * TB_WAVES)) >> 6;
    for (u64 q = wave; q < h.nq; q += nw) {
        const u64 a = h.off[q], c = h.off[q + 1] - a;  // (the same in every lane of the wavefront)
        if (c <= TB_GROUP || c > TB_LDS) continue;
        tb_sort<false>(h, m, q, a, idx, c, tb_pow2(c), lane, 64);
        const u64 keep = c < n ? c : n, d = toff[q];
        for (u64 r = lane; r < keep; r += 64) sel_copy(h, o, a + idx[r], d + r);
        wave_sync_lds();  // every lane is done with the buffer before the next row fills it
    }
}

__global__ __launch_bounds__(SEL_BLOCK) void k_tb_global(SelHits h, SelMeasure m, u32 n, const u64 *toff, const u64 *ioff, u32 *index, SelOut o) {
    for (u64 q = blockIdx.x; q < h.nq; q += gridDim.x) {
        const u64 a = h.off[q], c = h.off[q + 1] - a;  // (the same in every lane of the workgroup)
        if (c <= TB_LDS) continue;
        u32 *idx = index + ioff[q];
        tb_sort<true>(h, m, q, a, idx, c, tb_pow2(c), threadIdx.x, SEL_BLOCK);
        const u64 keep = c < n ? c : n, d = toff[q];
        for (u64 r = threadIdx.x; r < keep; r += SEL_BLOCK) sel_copy(h, o, a + idx[r], d + r);
    }
}

inline unsigned sel_grid(const bsk_ctx *ctx, u64 items) { return grid_for(ctx, items, SEL_BLOCK, 16); }

const char *const MEASURE_NAME[] = {"shared", "members", "dot", "min_sum", "query_cov", "target_cov", "jaccard", "cosine", "weighted_jaccard", "bc_similarity", "query_mass"};

// what the kind reads besides the hits' own shared and target
u32 measure_needs(u32 kind, const bsk_hits *h) {
    switch (kind) {
        case BSK_MEASURE_SHARED: return 0;
        case BSK_MEASURE_MEMBERS: return NEED_MEMBERS;
        case BSK_MEASURE_DOT:
        case BSK_MEASURE_MIN_SUM: return NEED_WEIGHTS;
        case BSK_MEASURE_QUERY_COV: return NEED_Q;
        case BSK_MEASURE_TARGET_COV: return NEED_T;
        case BSK_MEASURE_JACCARD: return h->has_total ? 0 : NEED_Q | NEED_T;
        case BSK_MEASURE_QUERY_MASS: return NEED_WEIGHTS | NEED_Q;
        default: return NEED_WEIGHTS | NEED_Q | NEED_T;  // cosine, weighted Jaccard, Bray-Curtis similarity
    }
}

// the checks both entries share, in the header's order; nothing touches the device
int sel_check_args(bsk_ctx *ctx, const char *entry, const bsk_hits *h, const bsk_measure *m, bsk_hits *const *out, u32 *need) {
    static thread_local char msg[160];
    const char *why = nullptr;
    int rc = BSK_ERR_ARG;
    if (!ctx || !h || !m || !out) why = "null argument";
    else if (m->kind > BSK_MEASURE_QUERY_MASS) why = "unknown measure";
    else if (m->flags != 0) why = "unknown flag";
    else if (h->ctx != ctx || (*out && (*out)->ctx != ctx)) why = "the hits belong to another context";
    else if (*out == h) why = "the result slot holds h itself";
    if (!why) {
        *need = measure_needs(m->kind, h);
        if ((*need & NEED_MEMBERS) && !h->has_members) why = "the measure needs hits with members (bsk_hits_fold makes such)";
        else if ((*need & NEED_WEIGHTS) && !h->has_weights) why = "the measure needs hits with weights";
        else if ((*need & NEED_Q) && !m->qnorm) why = "the measure needs qnorm";
        else if ((*need & NEED_T) && !m->tnorm) why = "the measure needs tnorm";
        else if ((*need & NEED_Q) && m->n_qnorm != h->n_queries) why = "n_qnorm != n_queries";
        else if (h->n_queries >= (1ULL << 32) || h->n_hits >= (1ULL << 32)) why = "2^32 rows or hits or more (split the hits)", rc = BSK_ERR_UNSUPPORTED;
    }
    if (!why) return BSK_OK;
    snprintf(msg, sizeof msg, "%s: %s", entry, why);
    if (ctx) ctx->err = msg;
    return rc;
}

// the scratch of one call: every pool buffer taken ONCE, before the first launch (a pool buffer that grows moves)
struct SelScratch {
    u64 *fig = nullptr, *part = nullptr, *pos = nullptr;  // pos: the filter's kept places [H + 1]; top_by's index offsets [nq + 1]
    u32 *keep = nullptr;
    SelHits in{};
    SelMeasure dm{};
};

int sel_prepare(bsk_ctx *ctx, const bsk_hits *h, const bsk_measure *m, u32 need, bool filter, SelScratch &s) {
    const u64 nq = h->n_queries, H = h->n_hits;
    hipStream_t st = ctx->stream;
    Carve c;
    const size_t o_fig = c.add<u64>(SEL_WORDS), o_part = c.add<u64>(scan_parts(H > nq ? H : nq)), o_pos = c.add<u64>((filter ? H : nq) + 1), o_keep = c.add<u32>(filter ? H : 1);
    void *b = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_SELECT_WORK, c.bytes, &b));
    s.fig = at<u64>(b, o_fig), s.part = at<u64>(b, o_part), s.pos = at<u64>(b, o_pos), s.keep = at<u32>(b, o_keep);
    HIPCHK(ctx, hipMemsetAsync(s.fig, 0, SEL_WORDS * 8, st));
    s.in = SelHits{h->offsets, h->target, h->shared, h->has_total ? h->total : nullptr, h->has_weights ? h->dot : nullptr, h->has_weights ? h->msum : nullptr,
                   h->has_members ? h->members : nullptr, nq, H};
    s.dm = SelMeasure{m->kind, need, nullptr, nullptr, (need & NEED_T) ? m->n_tnorm : 0};
    if (need & (NEED_Q | NEED_T)) {
        Carve cn;
        const size_t o_q = cn.add<u64>((need & NEED_Q) ? nq : 0), o_t = cn.add<u64>((need & NEED_T) ? m->n_tnorm : 0);
        void *bn = nullptr;
        HIPCHK(ctx, ctx_pool(ctx, SLOT_SELECT_NORMS, cn.bytes, &bn));
        u64 *qn = at<u64>(bn, o_q), *tn = at<u64>(bn, o_t);
        // (the caller's arrays are read until the call's first read-back, which every call with norms reaches before it returns BSK_OK)
        if ((need & NEED_Q) && nq) HIPCHK(ctx, hipMemcpyAsync(qn, m->qnorm, nq * 8, hipMemcpyHostToDevice, st));
        if ((need & NEED_T) && m->n_tnorm) HIPCHK(ctx, hipMemcpyAsync(tn, m->tnorm, m->n_tnorm * 8, hipMemcpyHostToDevice, st));
        s.dm.qn = qn, s.dm.tn = tn;
    }
    return BSK_OK;
}

int sel_refuse(bsk_ctx *ctx, const char *entry, u64 bad) {
    static thread_local char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", entry, (bad & SEL_BAD_TARGET) ? "a target >= n_tnorm" : "a hit whose denominator is not positive (norms inconsistent with the hits)");
    ctx->err = msg;
    return BSK_ERR_ARG;
}

// the output's arrays for K hits with the payloads of h, and its flags; n_hits stays 0 until the entry is done
int sel_shape(bsk_ctx *ctx, const bsk_hits *h, u64 K, bsk_hits *res, SelOut &o) {
    const u64 k = K ? K : 1;
    HIPCHK(ctx, grow_array(&res->target, &res->c_target, k * 4));
    HIPCHK(ctx, grow_array(&res->shared, &res->c_shared, k * 4));
    if (h->has_total) HIPCHK(ctx, grow_array(&res->total, &res->c_total, k * 4));
    if (h->has_weights) {
        HIPCHK(ctx, grow_array(&res->dot, &res->c_dot, k * 8));
        HIPCHK(ctx, grow_array(&res->msum, &res->c_msum, k * 8));
    }
    if (h->has_members) HIPCHK(ctx, grow_array(&res->members, &res->c_members, k * 4));
    o = SelOut{res->target, res->shared, res->total, res->dot, res->msum, res->members};
    return BSK_OK;
}

void sel_begin(const bsk_hits *h, bsk_hits *res) {
    res->n_queries = h->n_queries;
    res->n_hits = 0;
    res->n_large = 0;
    res->has_total = res->has_weights = res->has_members = false;
}
void sel_end(const bsk_hits *h, u64 K, bsk_hits *res) {
    res->n_hits = K;
    res->has_total = h->has_total;
    res->has_weights = h->has_weights;
    res->has_members = h->has_members;
}

// what runs on the object take_over hands over: the flags are written and scanned, K hits kept
int filter_impl(bsk_ctx *ctx, const bsk_hits *h, const bsk_measure *m, const SelScratch &s, u64 K, bsk_hits *res) {
    hipStream_t st = ctx->stream;
    const u64 nq = h->n_queries, H = h->n_hits;
    sel_begin(h, res);
    HIPCHK(ctx, grow_array(&res->offsets, &res->c_offsets, (nq + 1) * 8));
    SelOut o;
    const int rc = sel_shape(ctx, h, K, res, o);
    if (rc != BSK_OK) return rc;
    if (H) {
        hipLaunchKernelGGL(k_sel_place, dim3(sel_grid(ctx, H)), dim3(SEL_BLOCK), 0, st, s.in, (const u32 *)s.keep, (const u64 *)s.pos, o);
        hipLaunchKernelGGL(k_sel_offsets, dim3(sel_grid(ctx, nq + 1)), dim3(SEL_BLOCK), 0, st, (const u64 *)h->offsets, nq, (const u64 *)s.pos, res->offsets);
        HIPCHK(ctx, hipGetLastError());
    } else {
        HIPCHK(ctx, hipMemsetAsync(res->offsets, 0, (nq + 1) * 8, st));
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    sel_end(h, K, res);
    snprintf(res->plan, sizeof res->plan, "bsk_hits_filter %s: k_sel_check + k_sel_place + k_sel_offsets, hits=%llu kept=%llu", MEASURE_NAME[m->kind], (unsigned long long)H,
             (unsigned long long)K);
    return BSK_OK;
}

int top_by_impl(bsk_ctx *ctx, const bsk_hits *h, const bsk_measure *m, const SelScratch &s, u32 n, bsk_hits *res) {
    hipStream_t st = ctx->stream;
    const u64 nq = h->n_queries;
    sel_begin(h, res);
    HIPCHK(ctx, grow_array(&res->offsets, &res->c_offsets, (nq + 1) * 8));
    HIPCHK(ctx, scan_counts(st, TbCnt{h->offsets, n}, nq, s.part, res->offsets, s.fig + TB_KEPT, (u64 *)nullptr));
    HIPCHK(ctx, scan_counts(st, TbPadOf{h->offsets}, nq, s.part, s.pos, s.fig + TB_INDEX, (u64 *)nullptr));
    if (nq) {
        hipLaunchKernelGGL(k_tb_classes, dim3(sel_grid(ctx, nq)), dim3(SEL_BLOCK), 0, st, (const u64 *)h->offsets, nq, s.fig + TB_CLASSES);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, read_back(ctx, s.fig + TB_KEPT, 5));
    const u64 K = ctx->h_pinned[0], L = ctx->h_pinned[1], n_group = ctx->h_pinned[2], n_lds = ctx->h_pinned[3], n_global = ctx->h_pinned[4];
    SelOut o;
    const int rc = sel_shape(ctx, h, K, res, o);
    if (rc != BSK_OK) return rc;
    if (n_group) {
        hipLaunchKernelGGL(k_tb_group, dim3(grid_for(ctx, nq * 16, SEL_BLOCK, 32)), dim3(SEL_BLOCK), 0, st, s.in, s.dm, n, (const u64 *)res->offsets, o);
        HIPCHK(ctx, hipGetLastError());
    }
    if (n_lds) {
        hipLaunchKernelGGL(k_tb_lds, dim3(grid_for(ctx, nq, TB_WAVES, 8)), dim3(64 * TB_WAVES), 0, st, s.in, s.dm, n, (const u64 *)res->offsets, o);
        HIPCHK(ctx, hipGetLastError());
    }
    if (n_global) {
        u32 *index = nullptr;
        HIPCHK(ctx, ctx_pool(ctx, SLOT_SELECT_INDEX, L * 4, &index));
        hipLaunchKernelGGL(k_tb_global, dim3(grid_for(ctx, n_global, 1, 8)), dim3(SEL_BLOCK), 0, st, s.in, s.dm, n, (const u64 *)res->offsets, (const u64 *)s.pos, index, o);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    sel_end(h, K, res);
    res->n_large = n_global;
    snprintf(res->plan, sizeof res->plan, "bsk_hits_top_by n = %u %s: k_tb_group %llu queries (<= %d hits); k_tb_lds %llu queries (<= %d hits); k_tb_global %llu queries, %llu indices",
             n, MEASURE_NAME[m->kind], (unsigned long long)n_group, TB_GROUP, (unsigned long long)n_lds, TB_LDS, (unsigned long long)n_global, (unsigned long long)L);
    return BSK_OK;
}

}  // namespace

extern "C" int bsk_hits_filter(bsk_ctx *ctx, const bsk_hits *h, const bsk_measure *m, const bsk_filter_params *fp, bsk_hits **out) {
    if (!fp) return fail_arg(ctx, "bsk_hits_filter: null argument");
    u32 need = 0;
    int rc = sel_check_args(ctx, "bsk_hits_filter", h, m, out, &need);
    if (rc != BSK_OK) return rc;
    if (fp->min_den == 0) return fail_arg(ctx, "bsk_hits_filter: min_den == 0");
    const bool sq = m->kind == BSK_MEASURE_COSINE;  // the bound is on the cosine, N / D is its square
    const SelRule rule{sq ? (u128)fp->min_den * fp->min_den : (u128)fp->min_den, sq ? (u128)fp->min_num * fp->min_num : (u128)fp->min_num};
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the scratch and the one pass over the hits that can refuse them: before the slot is taken over, *out stays as it was
    hipStream_t st = ctx->stream;
    const u64 H = h->n_hits;
    SelScratch s;
    u64 K = 0;
    if (H) {
        rc = sel_prepare(ctx, h, m, need, true, s);
        if (rc != BSK_OK) return rc;
        hipLaunchKernelGGL(k_sel_check<true>, dim3(sel_grid(ctx, H)), dim3(SEL_BLOCK), 0, st, s.in, s.dm, rule, s.keep, s.fig);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, scan_counts(st, KeepOf{s.keep}, H, s.part, s.pos, s.fig + SEL_KEPT, (u64 *)nullptr));
        HIPCHK(ctx, read_back(ctx, s.fig + SEL_BAD, 2));  // (synchronises: the norms are not read after this)
        if (ctx->h_pinned[0]) return sel_refuse(ctx, "bsk_hits_filter", ctx->h_pinned[0]);
        K = ctx->h_pinned[1];
    }
    return take_over(ctx, out, bsk_hits_release, [&](bsk_hits *res, bool) { return filter_impl(ctx, h, m, s, K, res); });
}

extern "C" int bsk_hits_top_by(bsk_ctx *ctx, const bsk_hits *h, const bsk_measure *m, uint32_t n, bsk_hits **top) {
    u32 need = 0;
    int rc = sel_check_args(ctx, "bsk_hits_top_by", h, m, top, &need);
    if (rc != BSK_OK) return rc;
    if (n == 0) return fail_arg(ctx, "bsk_hits_top_by: n == 0");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SelScratch s;
    rc = sel_prepare(ctx, h, m, need, false, s);
    if (rc != BSK_OK) return rc;
    // the integer measures have no norms and D = 1: nothing to refuse.  The others: one pass before the slot is taken over.
    if (h->n_hits && m->kind >= BSK_MEASURE_QUERY_COV) {
        hipLaunchKernelGGL(k_sel_check<false>, dim3(sel_grid(ctx, h->n_hits)), dim3(SEL_BLOCK), 0, st, s.in, s.dm, SelRule{1, 0}, (u32 *)nullptr, s.fig);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, read_back(ctx, s.fig + SEL_BAD, 1));  // (synchronises: the norms are not read after this)
        if (ctx->h_pinned[0]) return sel_refuse(ctx, "bsk_hits_top_by", ctx->h_pinned[0]);
    } else if (need & (NEED_Q | NEED_T)) {
        HIPCHK(ctx, hipStreamSynchronize(st));  // (no hits: the norms' copies are done before the caller has them back)
    }
    return take_over(ctx, top, bsk_hits_release, [&](bsk_hits *res, bool) { return top_by_impl(ctx, h, m, s, n, res); });
}
