// sets_internal.hpp -- what sets.hip shares with search.hip: the sets object behind bsk_sets, the library's own three-kernel exclusive
// scan (rocprim::exclusive_scan over a transform iterator was 1.1 MB of the shared object) and the one 64-bit key sort sets.hip
// instantiates -- and, for setops.hip, counts.hip and compare.hip too, the host helpers around them (scan_parts, the capped grid, Carve).
// Nothing here crosses the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "biosketch.h"
#include "host_types.hpp"

struct bsk_sets {
    bsk_ctx *ctx = nullptr;
    u64 n_sets = 0, n_values = 0;
    u64 *offsets = nullptr;  // [n_sets + 1]
    u64 *values = nullptr;   // [n_values] ascending inside a set
    size_t c_offsets = 0, c_values = 0;  // bytes allocated (grow-only when the object is re-used: bsk_result_sets_reuse)
    char plan[256] = "";     // setops.hip: what the last bsk_sets_op / bsk_sets_reduce into this object ran (bsk_sets_plan)
    u64 by_path[3] = {};     // ... and how many pairs of a bsk_sets_op took k_so_group, k_so_wave, k_so_tile
    // counted sets (counts.hip): counts[i] = how often values[i] occurred.  `counted` says whether the array is valid: every entry
    // that writes values into this object without counts clears it and keeps the array (grow-only, like the others).
    u32 *counts = nullptr;   // [n_values]
    size_t c_counts = 0;
    bool counted = false;
};

// What sets_build_spans (sets.hip) makes sets from: n spans of tuples of one hash array, one set per span (or one set of all of them).
// Span i is a packed reference word refs[i] -- (first_tuple << 24) | n_tuples, bit 63 = the tuples are 64 apart -- or, with refs == NULL,
// wfirst[i] / wcount[i] with stride 1: the two forms a bsk_result describes its sequences in.  Spans may overlap (windows.hip).
struct SpanSrc {
    const u64 *hash, *refs, *wfirst, *wcount;
    u64 n;
    const char *entry;  // the C entry's name, for the error text
};
// The sets of the spans into `res` (the object take_over handed to the entry; `reused`: its arrays grow with slack): the dense copy, the
// small-set path or the segmented sort, the FracMinHash filter and, with `counted`, the run lengths.  Every failure leaves `res` to be
// released by the caller's take_over.
int sets_build_spans(bsk_ctx *ctx, const SpanSrc &src, int scope, int scale, bool counted, bsk_sets *res, bool reused) __attribute__((visibility("hidden")));

// counts.hip: run lengths of the kept heads of a sorted, flagged array (what sets.hip's general path has after its scan).  keep[i] = 1
// marks a kept head, pos[i] its place in the output; a run ends at the next kept head, at the first value above maxhash (filt) or at n.
// part: sets_run_counts_parts(n) u64 of scratch.  All on `st`, nothing read back.
u64 sets_run_counts_parts(u64 n) __attribute__((visibility("hidden")));
hipError_t sets_run_counts(hipStream_t st, const u64 *v, const u32 *keep, const u64 *pos, u64 n, u64 maxhash, bool filt, u64 *part, u32 *counts)
    __attribute__((visibility("hidden")));
// the sets' counts array, grow-only (reuse: with slack)
static inline hipError_t sets_grow_counts(bsk_sets *s, u64 n, bool slack) { return grow_array(&s->counts, &s->c_counts, (n ? n : 1) * 4, slack); }

// counts.hip: per set of first .. first + count - 1 (count != 0, a range inside s) the sum of its counts / of its squared counts
// (saturating), as bsk_sets_totals / bsk_sets_sumsq define them, into a device array on the context's stream; nothing is read back.
int sets_totals_device(bsk_ctx *ctx, const bsk_sets *s, u64 first, u64 count, u64 *out) __attribute__((visibility("hidden")));
int sets_sumsq_device(bsk_ctx *ctx, const bsk_sets *s, u64 first, u64 count, u64 *out) __attribute__((visibility("hidden")));

// rocprim::radix_sort_keys<u64> over bits [begin_bit, end_bit) on `st` (sets.hip: the instantiation its whole-batch sets use).
// tmp == nullptr: *tmp_bytes receives the temporary storage it needs.
hipError_t sets_sort_u64(void *tmp, size_t &tmp_bytes, u64 *in, u64 *out, size_t n, unsigned begin_bit, unsigned end_bit, hipStream_t st)
    __attribute__((visibility("hidden")));

// rocprim::segmented_radix_sort_keys<u64> over all 64 bits, segment g = [offs[g], offs[g + 1]) (sets.hip: the instantiation its
// per-sequence sets use; `in` is only read).  tmp == nullptr: *tmp_bytes receives the temporary storage it needs.
hipError_t sets_sort_segments_u64(void *tmp, size_t &tmp_bytes, const u64 *in, u64 *out, u64 n, u64 n_segments, u64 *offs, hipStream_t st)
    __attribute__((visibility("hidden")));

namespace {
// ---- exclusive scan of n per-sequence numbers (counts taken from the result's reference words, or an array) into out[0 .. n]
// (out[n] = the total); three small kernels: block sums, one block over the block sums, local scan + block offset ----
struct ArrayOf {
    const u64 *a;
    __device__ __forceinline__ u64 operator()(u64 r) const { return a[r]; }
};
struct KeepOf {
    const u32 *a;
    __device__ __forceinline__ u64 operator()(u64 r) const { return (u64)a[r]; }
};
#define SCAN_PER_THREAD 8
#define SCAN_BLOCK 256
#define SCAN_CHUNK (SCAN_PER_THREAD * SCAN_BLOCK)
__device__ __forceinline__ u64 wave_incl(u64 x, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const u64 t = __shfl_up(x, d, 64);
        if (lane >= d) x += t;
    }
    return x;
}
template <class F>
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_sums(F f, u64 n, u64 *part, u64 *mx) {
    __shared__ u64 s_w[SCAN_BLOCK / 64];
    const u64 b0 = (u64)blockIdx.x * SCAN_CHUNK;
    u64 sum = 0, m = 0, x[SCAN_PER_THREAD];
#pragma unroll
    for (int i = 0; i < SCAN_PER_THREAD; ++i) {  // all loads in flight before the first use
        const u64 r = b0 + (u64)i * SCAN_BLOCK + threadIdx.x;
        x[i] = r < n ? f(r) : 0;
    }
#pragma unroll
    for (int i = 0; i < SCAN_PER_THREAD; ++i) {
        sum += x[i];
        m = x[i] > m ? x[i] : m;
    }
    for (int d = 32; d; d >>= 1) {
        sum += __shfl_xor(sum, d, 64);
        const u64 t = __shfl_xor(m, d, 64);
        m = t > m ? t : m;
    }
    __shared__ u64 s_m[SCAN_BLOCK / 64];
    if ((threadIdx.x & 63) == 0) {
        s_w[threadIdx.x >> 6] = sum;
        s_m[threadIdx.x >> 6] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t = 0, bm = 0;
        for (int w = 0; w < SCAN_BLOCK / 64; ++w) {
            t += s_w[w];
            bm = s_m[w] > bm ? s_m[w] : bm;
        }
        part[blockIdx.x] = t;
        // one atomic per block, and only when it can raise the maximum (thousands of blocks hitting one address serialise in the L2)
        if (mx && bm > __hip_atomic_load(mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax((unsigned long long *)mx, (unsigned long long)bm);
    }
}
__global__ __launch_bounds__(1024) void k_scan_top(u64 *part, u64 nb, u64 *total) {  // in place: part[b] <- sum of part[0 .. b)
    __shared__ u64 s_w[16];
    __shared__ u64 s_carry;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (u64 b0 = 0; b0 < nb; b0 += 1024) {
        const u64 i = b0 + threadIdx.x;
        const u64 x = i < nb ? part[i] : 0;
        const u64 inc = wave_incl(x, lane);
        if (lane == 63) s_w[w] = inc;
        __syncthreads();
        u64 before = s_carry;
        for (int q = 0; q < w; ++q) before += s_w[q];
        if (i < nb) part[i] = before + inc - x;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = before + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = s_carry;
}
template <class F>
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_apply(F f, u64 n, const u64 *part, const u64 *total, u64 *out) {
    __shared__ u64 s_w[SCAN_BLOCK / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // thread t owns SCAN_PER_THREAD consecutive numbers
    const u64 r0 = (u64)blockIdx.x * SCAN_CHUNK + (u64)threadIdx.x * SCAN_PER_THREAD;
    u64 x[SCAN_PER_THREAD], sum = 0;
#pragma unroll
    for (int i = 0; i < SCAN_PER_THREAD; ++i) x[i] = r0 + i < n ? f(r0 + i) : 0;
#pragma unroll
    for (int i = 0; i < SCAN_PER_THREAD; ++i) sum += x[i];
    const u64 inc = wave_incl(sum, lane);
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    u64 run = part[blockIdx.x] + inc - sum;
    for (int q = 0; q < w; ++q) run += s_w[q];
#pragma unroll
    for (int i = 0; i < SCAN_PER_THREAD; ++i) {
        if (r0 + i < n) out[r0 + i] = run;
        run += x[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = *total;
}
// out[0..n] = exclusive scan of f(0..n-1); *total_dev (device) receives the total, *mx_dev (may be NULL) the maximum
template <class F>
hipError_t scan_counts(hipStream_t st, F f, u64 n, u64 *part, u64 *out, u64 *total_dev, u64 *mx_dev) {
    const u64 nb = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
    if (nb) hipLaunchKernelGGL(k_scan_sums<F>, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, st, f, n, part, mx_dev);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, st, part, nb, total_dev);
    if (nb) hipLaunchKernelGGL(k_scan_apply<F>, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, st, f, n, part, total_dev, out);
    else hipLaunchKernelGGL(k_scan_apply<F>, dim3(1), dim3(SCAN_BLOCK), 0, st, f, n, part, total_dev, out);
    return hipGetLastError();
}
inline u64 scan_parts(u64 n) { return (n + SCAN_CHUNK - 1) / SCAN_CHUNK + 2; }  // u64 of scan_counts' `part` for n numbers

// ---- host-side helpers of the sets-side translation units ----
// workgroups of `per_block` items, at most `blocks_per_cu` per CU and at least one
inline unsigned grid_for(const bsk_ctx *ctx, u64 items, u64 per_block, u64 blocks_per_cu) {
    return capped_grid(ctx, (items + per_block - 1) / per_block, blocks_per_cu);
}
// one pooled buffer carved into aligned pieces: add() every array, take Carve::bytes from the pool, then at() every piece
struct Carve {
    size_t bytes = 0;
    template <class T>
    size_t add(u64 n) {  // offset of an array of n T, 256-byte aligned
        const size_t at = bytes;
        bytes += ((n ? n : 1) * sizeof(T) + 255) & ~(size_t)255;
        return at;
    }
};
template <class T>
T *at(void *base, size_t off) {
    return reinterpret_cast<T *>(static_cast<char *>(base) + off);
}

}  // namespace
