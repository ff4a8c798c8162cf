// counts.hip -- COUNTED sketch sets: a bsk_sets whose values carry how often they occurred (k-mer / minimizer abundance), what a
// k-mer counter, an error filter ("seen at least twice") and an abundance-weighted containment start from.
//
// Construction.  sets.hip's general path sorts a scope's values, flags the first of every run (k_flag_unique) and scans the flags.
// The run length it used to throw away is the count.  A run ends at the next BOUNDARY: the next kept head -- a set's first element is
// one, so runs stop at set borders -- or the first filtered element (they sort to the end of their set).  Three kernels, all coalesced:
//   k_cnt_first   the first boundary of every chunk of CNT_CHUNK elements
//   k_cnt_suffix  one workgroup: the first boundary at or behind every chunk (suffix minimum over the chunks)
//   k_cnt_runs    a thread owns CNT_PER_THREAD consecutive elements; a suffix minimum across the workgroup gives every thread the
//                 first boundary behind its own elements, inside the chunk or -- only for runs that leave it -- from k_cnt_suffix
// so a poly-A batch, one run of millions, costs what any other input costs: nobody walks a run.
//
// bsk_sets_filter_counts: flags -> the library's scan -> scatter of values and counts -> new offsets, as sets.hip compacts.
// bsk_sets_totals: one scan of the counts (u64: exact) and a difference at the sets' offsets; no thread walks a set.
// bsk_sets_sumsq: a group of lanes per set sums c * c with saturating adds and reduces by shuffles (a difference of prefix sums, as
// bsk_sets_totals takes, cannot saturate correctly: the prefix would have to).
// The counted set algebra (bsk_sets_op_counted) lives with the merge kernels in setops.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "biosketch.h"
#include "host_types.hpp"
#include "sets_internal.hpp"

#define CNT_PER_THREAD 8
#define CNT_BLOCK 256
#define CNT_CHUNK (CNT_PER_THREAD * CNT_BLOCK)
#define CNT_NONE (~0ULL)

namespace {

__device__ __forceinline__ u64 min_u64(u64 a, u64 b) { return a < b ? a : b; }

__global__ __launch_bounds__(CNT_BLOCK) void k_cnt_first(const u64 *v, const u32 *keep, u64 n, u64 maxhash, int filt, u64 *cfirst) {
    __shared__ u64 s_w[CNT_BLOCK / 64];
    const u64 b0 = (u64)blockIdx.x * CNT_CHUNK;
    u64 m = CNT_NONE;
#pragma unroll
    for (int i = 0; i < CNT_PER_THREAD; ++i) {
        const u64 r = b0 + (u64)i * CNT_BLOCK + threadIdx.x;
        if (r < n && (keep[r] || (filt && v[r] > maxhash))) m = min_u64(m, r);
    }
    for (int d = 32; d; d >>= 1) m = min_u64(m, __shfl_xor(m, d, 64));
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CNT_BLOCK / 64; ++w) m = min_u64(m, s_w[w]);
        cfirst[blockIdx.x] = m;
    }
}

// in place: cf[c] <- min(cf[c .. nb)); trips of 1 024 chunks from the end, the carry crosses the trips (k_scan_top's shape: a suffix
// minimum by shuffles inside a wavefront, sixteen LDS words across them, three barriers a trip)
__global__ __launch_bounds__(1024) void k_cnt_suffix(u64 *cf, u64 nb) {
    __shared__ u64 s_w[16];
    __shared__ u64 s_carry;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = CNT_NONE;
    __syncthreads();
    for (u64 trip = (nb + 1023) / 1024; trip-- > 0;) {
        const u64 i = trip * 1024 + threadIdx.x;
        u64 x = i < nb ? cf[i] : CNT_NONE;
        for (int d = 1; d < 64; d <<= 1) {
            const u64 t = __shfl_down(x, d, 64);
            if (lane + d < 64) x = min_u64(x, t);
        }
        if (lane == 0) s_w[w] = x;
        __syncthreads();
        x = min_u64(x, s_carry);
        for (int q = w + 1; q < 16; ++q) x = min_u64(x, s_w[q]);
        if (i < nb) cf[i] = x;
        __syncthreads();
        if (threadIdx.x == 0) s_carry = x;
        __syncthreads();
    }
}

__global__ __launch_bounds__(CNT_BLOCK) void k_cnt_runs(const u64 *v, const u32 *keep, const u64 *pos, u64 n, u64 maxhash, int filt, const u64 *cnext, u64 nb,
                                                       u32 *counts) {
    __shared__ u64 s_w[CNT_BLOCK / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const u64 r0 = (u64)blockIdx.x * CNT_CHUNK + (u64)threadIdx.x * CNT_PER_THREAD;
    bool kp[CNT_PER_THREAD], bd[CNT_PER_THREAD];
    u64 ps[CNT_PER_THREAD];
#pragma unroll
    for (int i = 0; i < CNT_PER_THREAD; ++i) {
        const u64 r = r0 + i;
        kp[i] = r < n && keep[r] != 0;
        bd[i] = kp[i] || (filt && r < n && v[r] > maxhash);
        ps[i] = kp[i] ? pos[r] : 0;
    }
    u64 tf = CNT_NONE;  // the thread's first boundary
#pragma unroll
    for (int i = CNT_PER_THREAD - 1; i >= 0; --i)
        if (bd[i]) tf = r0 + i;
    u64 inc = tf;  // ... and the first one of this lane and the lanes behind it
    for (int d = 1; d < 64; d <<= 1) {
        const u64 t = __shfl_down(inc, d, 64);
        if (lane + d < 64) inc = min_u64(inc, t);
    }
    if (lane == 0) s_w[w] = inc;
    __syncthreads();
    u64 cur = __shfl_down(inc, 1, 64);  // the first boundary behind the thread's own elements
    if (lane == 63) cur = CNT_NONE;
    for (int q = w + 1; q < CNT_BLOCK / 64; ++q) cur = min_u64(cur, s_w[q]);
    if (blockIdx.x + 1 < nb) cur = min_u64(cur, cnext[blockIdx.x + 1]);  // a run that leaves the chunk
    cur = min_u64(cur, n);
#pragma unroll
    for (int i = CNT_PER_THREAD - 1; i >= 0; --i) {
        if (kp[i]) counts[ps[i]] = (u32)(cur - (r0 + i));  // (a call holds fewer than 2^32 values)
        if (bd[i]) cur = r0 + i;
    }
}

// ---- bsk_sets_filter_counts ----
__global__ void k_fc_flags(const u32 *c, u64 n, u32 lo, u32 hi, u32 *keep) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) keep[i] = (c[i] >= lo && c[i] <= hi) ? 1u : 0u;
}
__global__ void k_fc_scatter(const u64 *v, const u32 *c, const u32 *keep, const u64 *pos, u64 n, u64 *ov, u32 *oc) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        if (keep[i]) {
            ov[pos[i]] = v[i];
            oc[pos[i]] = c[i];
        }
}
__global__ void k_fc_offsets(const u64 *offs, const u64 *pos, u64 n_sets, u64 n_in, u64 n_out, u64 *out) {
    for (u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x; s <= n_sets; s += (u64)gridDim.x * blockDim.x) out[s] = offs[s] < n_in ? pos[offs[s]] : n_out;
}
// ---- bsk_sets_totals: csum = exclusive scan of the counts, csum[n_values] the grand total (NULL: the sets' sizes) ----
__global__ void k_ct_totals(const u64 *offs, const u64 *csum, u64 count, u64 *out) {
    for (u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x; s < count; s += (u64)gridDim.x * blockDim.x) {
        const u64 a = offs[s], b = offs[s + 1];
        out[s] = csum ? csum[b] - csum[a] : b - a;
    }
}
// ---- bsk_sets_sumsq: LANES lanes a set; saturating addition of non-negative terms is associative, so any order gives min(sum, 2^64 - 1) ----
__device__ __forceinline__ u64 add_sat(u64 a, u64 b) {
    const u64 s = a + b;
    return s < a ? ~0ull : s;
}
template <int LANES>
__global__ __launch_bounds__(256) void k_ct_sumsq(const u64 *offs, const u32 *c, u64 count, u64 *out) {
    const u64 lane = threadIdx.x % LANES;
    for (u64 s = ((u64)blockIdx.x * 256 + threadIdx.x) / LANES; s < count; s += (u64)gridDim.x * (256 / LANES)) {  // (a group enters and leaves together)
        const u64 a = offs[s], b = offs[s + 1];
        u64 acc = 0;
        for (u64 i = a + lane; i < b; i += LANES) acc = add_sat(acc, (u64)c[i] * c[i]);
        for (int d = LANES / 2; d; d >>= 1) acc = add_sat(acc, __shfl_xor(acc, d, LANES));
        if (lane == 0) out[s] = acc;
    }
}

unsigned ct_grid(const bsk_ctx *ctx, u64 items) { return grid_for(ctx, items, 256, 16); }

int filter_impl(bsk_ctx *ctx, const bsk_sets *s, u32 lo, u32 hi, bsk_sets *res) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u64 N = s->n_values, G = s->n_sets;
    res->n_sets = G;
    res->n_values = 0;
    res->counted = false;
    res->by_path[0] = res->by_path[1] = res->by_path[2] = 0;
    snprintf(res->plan, sizeof res->plan, "bsk_sets_filter_counts: %u <= count <= %u", lo, hi);
    HIPCHK(ctx, grow_array(&res->offsets, &res->c_offsets, (G + 1) * 8));
    if (N == 0) {
        HIPCHK(ctx, grow_array(&res->values, &res->c_values, 8));
        HIPCHK(ctx, sets_grow_counts(res, 1, true));
        HIPCHK(ctx, hipMemsetAsync(res->offsets, 0, (G + 1) * 8, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        res->counted = true;
        return BSK_OK;
    }
    void *bk = nullptr, *bp = nullptr, *bq = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_COUNT_KEEP, N * 4, &bk));
    HIPCHK(ctx, ctx_pool(ctx, SLOT_COUNT_POS, (N + 1) * 8, &bp));
    HIPCHK(ctx, ctx_pool(ctx, SLOT_COUNT_SCAN, (scan_parts(N) + 8) * 8, &bq));
    u32 *keep = static_cast<u32 *>(bk);
    u64 *pos = static_cast<u64 *>(bp), *tot = static_cast<u64 *>(bq), *part = tot + 8;
    HIPCHK(ctx, hipMemsetAsync(tot, 0, 64, st));
    hipLaunchKernelGGL(k_fc_flags, dim3(ct_grid(ctx, N)), dim3(256), 0, st, s->counts, N, lo, hi, keep);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, scan_counts(st, KeepOf{keep}, N, part, pos, tot, (u64 *)nullptr));
    HIPCHK(ctx, read_back(ctx, tot, 1));
    const u64 M = ctx->h_pinned[0];
    HIPCHK(ctx, grow_array(&res->values, &res->c_values, (M ? M : 1) * 8));
    HIPCHK(ctx, sets_grow_counts(res, M ? M : 1, true));
    if (M) hipLaunchKernelGGL(k_fc_scatter, dim3(ct_grid(ctx, N)), dim3(256), 0, st, s->values, s->counts, keep, pos, N, res->values, res->counts);
    hipLaunchKernelGGL(k_fc_offsets, dim3(ct_grid(ctx, G + 1)), dim3(256), 0, st, s->offsets, pos, G, N, M, res->offsets);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));
    res->n_values = M;
    res->counted = true;
    return BSK_OK;
}

}  // namespace

u64 sets_run_counts_parts(u64 n) { return n / CNT_CHUNK + 2; }

hipError_t sets_run_counts(hipStream_t st, const u64 *v, const u32 *keep, const u64 *pos, u64 n, u64 maxhash, bool filt, u64 *part, u32 *counts) {
    if (n == 0) return hipSuccess;
    const u64 nb = (n + CNT_CHUNK - 1) / CNT_CHUNK;
    hipLaunchKernelGGL(k_cnt_first, dim3((unsigned)nb), dim3(CNT_BLOCK), 0, st, v, keep, n, maxhash, filt ? 1 : 0, part);
    if (nb > 1) hipLaunchKernelGGL(k_cnt_suffix, dim3(1), dim3(1024), 0, st, part, nb);
    hipLaunchKernelGGL(k_cnt_runs, dim3((unsigned)nb), dim3(CNT_BLOCK), 0, st, v, keep, pos, n, maxhash, filt ? 1 : 0, (const u64 *)part, nb, counts);
    return hipGetLastError();
}

// The norms of sets first .. first + count - 1 (count != 0, the range checked by the caller) into a device array, on the context's stream
// and without a synchronisation: what bsk_sets_totals and bsk_sets_sumsq copy to the host, and what a counted index keeps (search.hip).
int sets_totals_device(bsk_ctx *ctx, const bsk_sets *s, u64 first, u64 count, u64 *out) {
    hipStream_t st = ctx->stream;
    const u64 N = s->n_values;
    void *bp = nullptr, *bq = nullptr;
    u64 *csum = nullptr;
    if (s->counted) {
        HIPCHK(ctx, ctx_pool(ctx, SLOT_COUNT_POS, (N + 1) * 8, &bp));
        HIPCHK(ctx, ctx_pool(ctx, SLOT_COUNT_SCAN, (scan_parts(N) + 8) * 8, &bq));
        csum = static_cast<u64 *>(bp);
        u64 *tot = static_cast<u64 *>(bq);
        HIPCHK(ctx, scan_counts(st, KeepOf{s->counts}, N, tot + 8, csum, tot, (u64 *)nullptr));
    }
    hipLaunchKernelGGL(k_ct_totals, dim3(ct_grid(ctx, count)), dim3(256), 0, st, (const u64 *)(s->offsets + first), (const u64 *)csum, count, out);
    HIPCHK(ctx, hipGetLastError());
    return BSK_OK;
}

int sets_sumsq_device(bsk_ctx *ctx, const bsk_sets *s, u64 first, u64 count, u64 *out) {
    hipStream_t st = ctx->stream;
    const u64 *offs = s->offsets + first;
    if (!s->counted) {  // every count is 1: the sizes
        hipLaunchKernelGGL(k_ct_totals, dim3(ct_grid(ctx, count)), dim3(256), 0, st, offs, (const u64 *)nullptr, count, out);
    } else if (s->n_values <= s->n_sets * 16) {  // small sets (16 values on average): 8 lanes a set
        hipLaunchKernelGGL(k_ct_sumsq<8>, dim3(ct_grid(ctx, count * 8)), dim3(256), 0, st, offs, (const u32 *)s->counts, count, out);
    } else {  // a wavefront a set
        hipLaunchKernelGGL(k_ct_sumsq<64>, dim3(ct_grid(ctx, count * 64)), dim3(256), 0, st, offs, (const u32 *)s->counts, count, out);
    }
    HIPCHK(ctx, hipGetLastError());
    return BSK_OK;
}

extern "C" int bsk_sets_counts_device(const bsk_sets *s, const uint32_t **counts) {
    if (!s || !counts) return BSK_ERR_ARG;
    *counts = s->counted ? (const uint32_t *)s->counts : nullptr;
    return BSK_OK;
}

extern "C" int bsk_sets_fetch_counts(bsk_ctx *ctx, const bsk_sets *s, uint64_t first, uint64_t count, uint32_t *counts, uint64_t count_cap) {
    if (!ctx || !s || !counts) return fail_arg(ctx, "bsk_sets_fetch_counts: null argument");
    if (s->ctx != ctx) return fail_arg(ctx, "bsk_sets_fetch_counts: the sets belong to another context");
    if (!s->counted) return fail_arg(ctx, "bsk_sets_fetch_counts: the sets are not counted");
    if (first > s->n_sets || count > s->n_sets - first) return fail_arg(ctx, "bsk_sets_fetch_counts: range outside the sets");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    u64 o[2] = {0, 0};
    HIPCHK(ctx, hipMemcpy(&o[0], s->offsets + first, 8, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(&o[1], s->offsets + first + count, 8, hipMemcpyDeviceToHost));
    const u64 nv = o[1] - o[0];
    if (nv > count_cap) return fail_arg(ctx, "bsk_sets_fetch_counts: count_cap too small");
    if (nv) HIPCHK(ctx, hipMemcpy(counts, s->counts + o[0], nv * 4, hipMemcpyDeviceToHost));
    return BSK_OK;
}

extern "C" int bsk_sets_from_host_counted(bsk_ctx *ctx, const uint64_t *offsets, uint64_t n_sets, const uint64_t *values, const uint32_t *counts, bsk_sets **out) {
    bsk_sets *s = nullptr;
    if (out) *out = nullptr;
    if (ctx && offsets && out) {  // the counts first, before anything goes to the device: offsets that never decrease bound every index by N
        bool sane = offsets[0] == 0;
        for (u64 g = 0; sane && g < n_sets; ++g) sane = offsets[g + 1] >= offsets[g];
        if (sane) {
            const u64 N = offsets[n_sets];
            if (N && !counts) return fail_arg(ctx, "bsk_sets_from_host_counted: null counts");
            for (u64 i = 0; i < N; ++i)
                if (counts[i] == 0) return fail_arg(ctx, "bsk_sets_from_host_counted: a count of 0");
        }
    }
    const int rc = bsk_sets_from_host(ctx, offsets, n_sets, values, out ? &s : nullptr);  // (its checks; *out = NULL on every error)
    if (rc != BSK_OK) return rc;
    const u64 N = offsets[n_sets];
    hipError_t e = sets_grow_counts(s, N, false);
    if (e == hipSuccess && N) e = hipMemcpyAsync(s->counts, counts, N * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        bsk_sets_release(s);
        return fail_hip(ctx, e, "bsk_sets_from_host_counted");
    }
    s->counted = true;
    *out = s;
    return BSK_OK;
}

extern "C" int bsk_sets_filter_counts(bsk_ctx *ctx, const bsk_sets *s, uint32_t min_count, uint32_t max_count, bsk_sets **out) {
    if (!ctx || !s || !out) return fail_arg(ctx, "bsk_sets_filter_counts: null argument");
    if (s->ctx != ctx || (*out && (*out)->ctx != ctx)) return fail_arg(ctx, "bsk_sets_filter_counts: the sets belong to another context");
    if (*out == s) return fail_arg(ctx, "bsk_sets_filter_counts: *out is the input");
    if (!s->counted) return fail_arg(ctx, "bsk_sets_filter_counts: the sets are not counted");
    if (min_count == 0 || min_count > max_count) return fail_arg(ctx, "bsk_sets_filter_counts: min_count == 0 or min_count > max_count");
    return take_over(ctx, out, bsk_sets_release, [&](bsk_sets *res, bool) { return filter_impl(ctx, s, min_count, max_count, res); });
}

extern "C" int bsk_sets_totals(bsk_ctx *ctx, const bsk_sets *s, uint64_t first, uint64_t count, uint64_t *totals) {
    if (!ctx || !s || (count && !totals)) return fail_arg(ctx, "bsk_sets_totals: null argument");
    if (s->ctx != ctx) return fail_arg(ctx, "bsk_sets_totals: the sets belong to another context");
    if (first > s->n_sets || count > s->n_sets - first) return fail_arg(ctx, "bsk_sets_totals: range outside the sets");
    if (count == 0) return BSK_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    void *bo = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_COUNT_OUT, count * 8, &bo));
    const int rc = sets_totals_device(ctx, s, first, count, static_cast<u64 *>(bo));
    if (rc != BSK_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(totals, bo, count * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BSK_OK;
}

extern "C" int bsk_sets_sumsq(bsk_ctx *ctx, const bsk_sets *s, uint64_t first, uint64_t count, uint64_t *sumsq) {
    if (!ctx || !s || (count && !sumsq)) return fail_arg(ctx, "bsk_sets_sumsq: null argument");
    if (s->ctx != ctx) return fail_arg(ctx, "bsk_sets_sumsq: the sets belong to another context");
    if (first > s->n_sets || count > s->n_sets - first) return fail_arg(ctx, "bsk_sets_sumsq: range outside the sets");
    if (count == 0) return BSK_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    void *bo = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_COUNT_OUT, count * 8, &bo));
    const int rc = sets_sumsq_device(ctx, s, first, count, static_cast<u64 *>(bo));
    if (rc != BSK_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(sumsq, bo, count * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BSK_OK;
}
