// transpose.hip -- hits by target (include/biosketch.h "hits by target"): bsk_hits_transpose writes the hits whose rows are the targets,
// every payload with its hit; bsk_hits_tally fills the per-target table (rows, unique, shared) everybody computes from it and can add
// batch after batch into one table.
//
// The transpose:
//   k_tp_keys      a lane per hit: refuses a target >= n_targets and writes the key (target << hit_bits) | hit index -- every key is
//                  distinct, so the sorted order is a function of the keys alone, whatever the sort does with equal keys.  Runs before
//                  the result slot is taken over.
//   sets_sort_u64  over the hit_bits + target_bits that matter
//   k_tp_offsets   a lane per target: its first key by a search of the sorted keys (k_win_spans' idea) -> the output offsets
//   k_tp_place     a lane per output hit: the key's low bits are the input hit; its query, by a search of the input's offsets, is the
//                  output's target[]; every array the input carries is gathered by that index
// Every word of the output is written once, by a lane that is a function of the input: bit-identical from call to call.  No row of
// either side is walked by one lane.  No atomics but the "bad input" flag.
//
// The tally:
//   k_tl_check     a lane per hit: refuses a target >= n_targets.  Its answer is read before anything is added.
//   k_tl_add<lds>  n_targets <= TL_LDS_TARGETS: a workgroup adds its share of the hits (rows, shared) and of the rows of one hit (unique)
//                  into three u64 counters per target in LDS, then adds its non-zero counters to the table: one global add per counter
//                  and workgroup.  3 x 8 B x 2 048 targets = 48 KB of the CU's 160 KB: three workgroups of 512 lanes, six wavefronts
//                  per SIMD.
//   k_tl_add<global>  more targets: the adds go straight to the table in global memory
// In both a wavefront whose 64 hits name one target -- the read set of one genome -- sums on its lanes first and adds once.  The sums
// are integer adds, their result does not depend on the order: bit-identical from call to call.
// Integers only, bounded loops, pooled memory, no kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "biosketch.h"
#include "host_types.hpp"
#include "search_internal.hpp"
#include "sets_internal.hpp"

#define TP_BLOCK 256
#define TL_BLOCK 512
#define TL_LDS_TARGETS 2048  // three u64 counters per target: 48 KB of LDS a workgroup
#define TL_HITS_PER_LANE 16  // k_tl_lds: hits a workgroup should at least take per lane before it pays for its flush

struct bsk_tally {
    bsk_ctx *ctx = nullptr;
    u64 n_targets = 0, queries = 0, hits = 0, calls = 0;
    u64 *table = nullptr;  // rows[n_targets], unique[n_targets], shared[n_targets]
    size_t c_table = 0;    // bytes allocated (grow-only when the object is re-used)
    char plan[160] = "";
};

namespace {

enum { TP_BAD = 0, TP_WORDS = 2 };  // the figures, one u64 word each

struct TpHits {  // the input; a payload it does not carry is NULL
    const u64 *off;
    const u32 *tgt, *sh, *total;
    const u64 *dot, *msum;
    const u32 *members;
    u64 nq, H;
};
struct TpOut {
    u32 *tgt, *sh, *total;
    u64 *dot, *msum;
    u32 *members;
};

inline unsigned bits_of(u64 x) { return x ? 64u - (unsigned)__builtin_clzll(x) : 0u; }

// one ballot per trip of a whole wavefront: a lane whose target is beyond the targets raises the flag
__device__ __forceinline__ void tp_flag_bad(bool bad, u64 *fig) {
    const u64 m = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicOr(reinterpret_cast<u32 *>(fig + TP_BAD), 1u);
}

__global__ __launch_bounds__(TP_BLOCK) void k_tp_keys(const u32 *tgt, u64 H, u64 nt, unsigned hit_bits, u64 *key, u64 *fig) {
    for (u64 b = (u64)blockIdx.x * TP_BLOCK; b < H; b += (u64)gridDim.x * TP_BLOCK) {
        const u64 i = b + threadIdx.x;
        bool bad = false;
        if (i < H) {
            const u64 t = tgt[i];
            bad = t >= nt;
            key[i] = (t << hit_bits) | i;  // (a bad target's key is never sorted: the call is refused)
        }
        tp_flag_bad(bad, fig);
    }
}

// out[t] = the sorted keys below target t (out[nt] = H): the first j with key[j] >> hit_bits >= t.  33 halvings cover H < 2^32.
__global__ __launch_bounds__(TP_BLOCK) void k_tp_offsets(const u64 *key, u64 H, u64 nt, unsigned hit_bits, u64 *out) {
    for (u64 t = (u64)blockIdx.x * TP_BLOCK + threadIdx.x; t <= nt; t += (u64)gridDim.x * TP_BLOCK) {
        u64 lo = 0, hi = H;  // the answer lies in [lo, hi]
        for (int it = 0; it < 33 && lo < hi; ++it) {
            const u64 mid = (lo + hi) >> 1;
            if ((key[mid] >> hit_bits) < t) lo = mid + 1;
            else hi = mid;
        }
        out[t] = lo;
    }
}

// the last q with off[q] <= i (off[0] = 0 <= i < off[nq]; rows without hits are passed over).  33 halvings cover nq < 2^32.
__device__ __forceinline__ u64 tp_row_of(const u64 *off, u64 nq, u64 i) {
    u64 lo = 0, hi = nq;
    for (int it = 0; it < 33 && hi - lo > 1; ++it) {
        const u64 mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(TP_BLOCK) void k_tp_place(TpHits h, const u64 *key, unsigned hit_bits, TpOut o) {
    const u64 mask = (1ULL << hit_bits) - 1;  // (hit_bits <= 32)
    for (u64 j = (u64)blockIdx.x * TP_BLOCK + threadIdx.x; j < h.H; j += (u64)gridDim.x * TP_BLOCK) {
        const u64 src = key[j] & mask;  // (< H: the keys are a permutation of those k_tp_keys wrote)
        o.tgt[j] = (u32)tp_row_of(h.off, h.nq, src);
        o.sh[j] = h.sh[src];
        if (h.total) o.total[j] = h.total[src];
        if (h.dot) {
            o.dot[j] = h.dot[src];
            o.msum[j] = h.msum[src];
        }
        if (h.members) o.members[j] = h.members[src];
    }
}

// ---- the tally ----
__global__ __launch_bounds__(TP_BLOCK) void k_tl_check(const u32 *tgt, u64 H, u64 nt, u64 *fig) {
    for (u64 b = (u64)blockIdx.x * TP_BLOCK; b < H; b += (u64)gridDim.x * TP_BLOCK) {
        const u64 i = b + threadIdx.x;
        tp_flag_bad(i < H && (u64)tgt[i] >= nt, fig);
    }
}

typedef unsigned long long ull;

// One trip of a whole wavefront over the hits: lane `live` adds (1, sh) to target t's rows and shared in `rows` / `shared` (LDS or
// global).  Where every live lane names one target the wavefront sums on its lanes and its first live lane adds once.
__device__ __forceinline__ void tl_add_hit(bool live, u32 t, u32 sh, ull *rows, ull *shared) {
    const u64 m = __ballot(live);
    if (!m) return;
    const int first = __ffsll((ull)m) - 1;
    const u32 t0 = __shfl(t, first, 64);
    if (__ballot(live && t != t0) == 0) {
        u64 sum = live ? sh : 0;
        for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d, 64);
        if ((int)(threadIdx.x & 63) == first) {
            atomicAdd(rows + t0, (ull)__popcll(m));
            if (sum) atomicAdd(shared + t0, (ull)sum);
        }
    } else if (live) {
        atomicAdd(rows + t, 1ULL);
        if (sh) atomicAdd(shared + t, (ull)sh);
    }
}

// TILE_LDS: the counters are the workgroup's LDS, flushed at the end (nt <= TL_LDS_TARGETS); else the table itself
template <bool TILE_LDS>
__global__ __launch_bounds__(TL_BLOCK) void k_tl_add(const u64 *off, const u32 *tgt, const u32 *shv, u64 nq, u64 H, u64 nt, u64 *table) {
    __shared__ ull s_bins[TILE_LDS ? 3 * TL_LDS_TARGETS : 1];
    ull *rows = TILE_LDS ? s_bins : (ull *)table, *unique = rows + nt, *shared = rows + 2 * nt;
    if (TILE_LDS) {
        for (u64 x = threadIdx.x; x < 3 * nt; x += TL_BLOCK) s_bins[x] = 0;
        __syncthreads();
    }
    for (u64 b = (u64)blockIdx.x * TL_BLOCK; b < H; b += (u64)gridDim.x * TL_BLOCK) {
        const u64 i = b + threadIdx.x;
        const bool live = i < H;
        tl_add_hit(live, live ? tgt[i] : 0u, live ? shv[i] : 0u, rows, shared);
    }
    for (u64 q = (u64)blockIdx.x * TL_BLOCK + threadIdx.x; q < nq; q += (u64)gridDim.x * TL_BLOCK) {
        const u64 a = off[q];
        if (off[q + 1] - a == 1) atomicAdd(unique + tgt[a], 1ULL);
    }
    if (TILE_LDS) {
        __syncthreads();
        for (u64 x = threadIdx.x; x < 3 * nt; x += TL_BLOCK) {
            const ull v = s_bins[x];
            if (v) atomicAdd((ull *)table + x, v);
        }
    }
}

inline unsigned tp_grid(const bsk_ctx *ctx, u64 items) { return grid_for(ctx, items, TP_BLOCK, 16); }

// the checks both entries share, in the header's order; nothing touches the device and *out is not looked into before the arguments are there
template <class T>
int tp_check_args(bsk_ctx *ctx, const char *entry, const bsk_hits *h, u64 n_targets, T *const *out) {
    static thread_local char msg[160];
    const char *why = nullptr;
    int rc = BSK_ERR_ARG;
    if (!ctx || !h || !out) why = "null argument";
    else if ((const void *)*out == (const void *)h) why = "the result slot holds h itself";
    else if (h->ctx != ctx || (*out && (*out)->ctx != ctx)) why = "the hits or the result belong to another context";
    else if (n_targets >= (1ULL << 32) || h->n_queries >= (1ULL << 32) || h->n_hits >= (1ULL << 32))
        why = "2^32 targets, rows or hits or more (split the hits)", rc = BSK_ERR_UNSUPPORTED;
    if (!why) return BSK_OK;
    snprintf(msg, sizeof msg, "%s: %s", entry, why);
    if (ctx) ctx->err = msg;
    return rc;
}

struct TpScratch {
    u64 *fig = nullptr, *kin = nullptr, *kout = nullptr;
    void *stmp = nullptr;
    size_t stmp_bytes = 0;
    unsigned hit_bits = 1, key_bits = 1;
};

// what runs on the object take_over hands over: the keys are written and the targets checked
int transpose_impl(bsk_ctx *ctx, const bsk_hits *h, u64 nt, TpScratch &s, bsk_hits *res) {
    hipStream_t st = ctx->stream;
    const u64 nq = h->n_queries, H = h->n_hits, k = H ? H : 1;
    res->n_queries = nt;
    res->n_hits = 0;
    res->n_large = 0;
    res->has_total = res->has_weights = res->has_members = false;
    HIPCHK(ctx, grow_array(&res->offsets, &res->c_offsets, (nt + 1) * 8));
    HIPCHK(ctx, grow_array(&res->target, &res->c_target, k * 4));
    HIPCHK(ctx, grow_array(&res->shared, &res->c_shared, k * 4));
    if (h->has_total) HIPCHK(ctx, grow_array(&res->total, &res->c_total, k * 4));
    if (h->has_weights) {
        HIPCHK(ctx, grow_array(&res->dot, &res->c_dot, k * 8));
        HIPCHK(ctx, grow_array(&res->msum, &res->c_msum, k * 8));
    }
    if (h->has_members) HIPCHK(ctx, grow_array(&res->members, &res->c_members, k * 4));
    if (H) {
        size_t tb = s.stmp_bytes;
        HIPCHK(ctx, sets_sort_u64(s.stmp, tb, s.kin, s.kout, (size_t)H, 0, s.key_bits, st));
        const TpHits in{h->offsets, h->target, h->shared, h->has_total ? h->total : nullptr, h->has_weights ? h->dot : nullptr, h->has_weights ? h->msum : nullptr,
                        h->has_members ? h->members : nullptr, nq, H};
        const TpOut o{res->target, res->shared, res->total, res->dot, res->msum, res->members};
        hipLaunchKernelGGL(k_tp_offsets, dim3(tp_grid(ctx, nt + 1)), dim3(TP_BLOCK), 0, st, (const u64 *)s.kout, H, nt, s.hit_bits, res->offsets);
        hipLaunchKernelGGL(k_tp_place, dim3(tp_grid(ctx, H)), dim3(TP_BLOCK), 0, st, in, (const u64 *)s.kout, s.hit_bits, o);
        HIPCHK(ctx, hipGetLastError());
    } else {
        HIPCHK(ctx, hipMemsetAsync(res->offsets, 0, (nt + 1) * 8, st));
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    res->n_hits = H;
    res->has_total = h->has_total;
    res->has_weights = h->has_weights;
    res->has_members = h->has_members;
    snprintf(res->plan, sizeof res->plan, "bsk_hits_transpose: k_tp_keys + sort + k_tp_offsets + k_tp_place, targets=%llu hits=%llu key_bits=%u", (unsigned long long)nt,
             (unsigned long long)H, H ? s.key_bits : 0u);
    return BSK_OK;
}

int tally_impl(bsk_ctx *ctx, const bsk_hits *h, u64 nt, bool add, bsk_tally *res, bool reused) {
    hipStream_t st = ctx->stream;
    const u64 nq = h->n_queries, H = h->n_hits;
    const bool fresh = !(add && reused);
    HIPCHK(ctx, grow_array(&res->table, &res->c_table, (nt ? nt : 1) * 24));  // (adding: n_targets is the table's, nothing moves)
    if (fresh) {
        res->n_targets = nt;
        res->queries = res->hits = res->calls = 0;
        HIPCHK(ctx, hipMemsetAsync(res->table, 0, (nt ? nt : 1) * 24, st));
    }
    const bool lds = nt <= TL_LDS_TARGETS;
    if (H) {
        if (lds)
            hipLaunchKernelGGL(k_tl_add<true>, dim3(grid_for(ctx, H > nq ? H : nq, TL_BLOCK * TL_HITS_PER_LANE, 3)), dim3(TL_BLOCK), 0, st, (const u64 *)h->offsets,
                               (const u32 *)h->target, (const u32 *)h->shared, nq, H, nt, res->table);
        else
            hipLaunchKernelGGL(k_tl_add<false>, dim3(grid_for(ctx, H > nq ? H : nq, TL_BLOCK, 8)), dim3(TL_BLOCK), 0, st, (const u64 *)h->offsets, (const u32 *)h->target,
                               (const u32 *)h->shared, nq, H, nt, res->table);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    res->queries += nq;
    res->hits += H;
    res->calls += 1;
    snprintf(res->plan, sizeof res->plan, "bsk_hits_tally%s: k_tl_check + %s, targets=%llu hits=%llu", add ? " add" : "",
             !H ? "nothing (no hits)" : lds ? "k_tl_add<lds> (counters in LDS, one add per counter and workgroup)" : "k_tl_add<global> (adds to the table)",
             (unsigned long long)nt, (unsigned long long)H);
    return BSK_OK;
}

}  // namespace

extern "C" int bsk_hits_transpose(bsk_ctx *ctx, const bsk_hits *h, uint64_t n_targets, bsk_hits **out) {
    int rc = tp_check_args(ctx, "bsk_hits_transpose", h, n_targets, out);
    if (rc != BSK_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the scratch and the one pass over the hits that can refuse them: before the slot is taken over, *out stays as it was
    hipStream_t st = ctx->stream;
    const u64 H = h->n_hits;
    TpScratch s;
    if (H) {
        s.hit_bits = std::max(1u, bits_of(H - 1));
        s.key_bits = s.hit_bits + bits_of(n_targets ? n_targets - 1 : 0);
        HIPCHK(ctx, sets_sort_u64(nullptr, s.stmp_bytes, nullptr, nullptr, (size_t)H, 0, s.key_bits, st));
        Carve c;
        const size_t o_fig = c.add<u64>(TP_WORDS), o_kin = c.add<u64>(H), o_kout = c.add<u64>(H), o_tmp = c.add<char>(s.stmp_bytes ? s.stmp_bytes : 8);
        void *b = nullptr;
        HIPCHK(ctx, ctx_pool(ctx, SLOT_TRANSPOSE_WORK, c.bytes, &b));
        s.fig = at<u64>(b, o_fig), s.kin = at<u64>(b, o_kin), s.kout = at<u64>(b, o_kout), s.stmp = at<char>(b, o_tmp);
        HIPCHK(ctx, hipMemsetAsync(s.fig, 0, TP_WORDS * 8, st));
        hipLaunchKernelGGL(k_tp_keys, dim3(tp_grid(ctx, H)), dim3(TP_BLOCK), 0, st, (const u32 *)h->target, H, n_targets, s.hit_bits, s.kin, s.fig);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, read_back(ctx, s.fig + TP_BAD, 1));
        if (ctx->h_pinned[0]) return fail_arg(ctx, "bsk_hits_transpose: a target >= n_targets");
    }
    return take_over(ctx, out, bsk_hits_release, [&](bsk_hits *res, bool) { return transpose_impl(ctx, h, n_targets, s, res); });
}

extern "C" int bsk_hits_tally(bsk_ctx *ctx, const bsk_hits *h, uint64_t n_targets, uint32_t flags, bsk_tally **out) {
    int rc = tp_check_args(ctx, "bsk_hits_tally", h, n_targets, out);
    if (rc != BSK_OK) return rc;
    if (flags & ~(uint32_t)BSK_TALLY_ADD) return fail_arg(ctx, "bsk_hits_tally: unknown flag");
    const bool add = (flags & BSK_TALLY_ADD) != 0;
    if (add && *out && (*out)->n_targets != n_targets) return fail_arg(ctx, "bsk_hits_tally: BSK_TALLY_ADD into a table of another n_targets");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the one pass over the hits that can refuse them: its answer is read before the slot is taken over and before anything is added
    hipStream_t st = ctx->stream;
    const u64 H = h->n_hits;
    if (H) {
        u64 *fig = nullptr;
        HIPCHK(ctx, ctx_pool(ctx, SLOT_TALLY_WORK, TP_WORDS * 8, &fig));
        HIPCHK(ctx, hipMemsetAsync(fig, 0, TP_WORDS * 8, st));
        hipLaunchKernelGGL(k_tl_check, dim3(tp_grid(ctx, H)), dim3(TP_BLOCK), 0, st, (const u32 *)h->target, H, n_targets, fig);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, read_back(ctx, fig + TP_BAD, 1));
        if (ctx->h_pinned[0]) return fail_arg(ctx, "bsk_hits_tally: a target >= n_targets");
    }
    return take_over(ctx, out, bsk_tally_release, [&](bsk_tally *res, bool reused) { return tally_impl(ctx, h, n_targets, add, res, reused); });
}

extern "C" int bsk_tally_info(const bsk_tally *t, uint64_t *n_targets, uint64_t *queries, uint64_t *hits, uint64_t *calls) {
    if (!t) return BSK_ERR_ARG;
    if (n_targets) *n_targets = t->n_targets;
    if (queries) *queries = t->queries;
    if (hits) *hits = t->hits;
    if (calls) *calls = t->calls;
    return BSK_OK;
}

extern "C" int bsk_tally_plan(const bsk_tally *t, const char **plan) {
    if (!t) return BSK_ERR_ARG;
    if (plan) *plan = t->plan;
    return BSK_OK;
}

extern "C" int bsk_tally_device(const bsk_tally *t, const uint64_t **rows, const uint64_t **unique, const uint64_t **shared) {
    if (!t) return BSK_ERR_ARG;
    if (rows) *rows = (const uint64_t *)t->table;
    if (unique) *unique = (const uint64_t *)(t->table + t->n_targets);
    if (shared) *shared = (const uint64_t *)(t->table + 2 * t->n_targets);
    return BSK_OK;
}

extern "C" int bsk_tally_fetch(bsk_ctx *ctx, const bsk_tally *t, uint64_t first, uint64_t count, uint64_t *rows, uint64_t *unique, uint64_t *shared) {
    if (!ctx || !t) return fail_arg(ctx, "bsk_tally_fetch: null argument");
    if (t->ctx != ctx) return fail_arg(ctx, "bsk_tally_fetch: the table belongs to another context");
    if (first > t->n_targets || count > t->n_targets - first) return fail_arg(ctx, "bsk_tally_fetch: range outside the table");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    uint64_t *const dst[3] = {rows, unique, shared};
    for (int a = 0; a < 3; ++a)
        if (dst[a] && count) HIPCHK(ctx, hipMemcpyAsync(dst[a], t->table + a * t->n_targets + first, count * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BSK_OK;
}

extern "C" void bsk_tally_release(bsk_tally *t) {
    if (!t) return;
    if (t->ctx) (void)hipSetDevice(t->ctx->device);
    (void)hipFree(t->table);
    delete t;
}
