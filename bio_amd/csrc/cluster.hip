// cluster.hip -- clusters of a neighbour graph that is already on the device (include/biosketch.h "clusters of a neighbour graph"):
// connected components and greedy representative clustering of a bsk_hits, n labels and at most n representatives out.
//
// Everything runs in RANK space (rank 0 = the best node), so that "best" is a minimum and a 32-bit atomicMin picks it.
//
// The visibility rule every kernel here keeps (the XCDs' L2s are not coherent with each other, a CU's L1 is not refreshed inside a launch):
// inside one launch workgroups meet ONLY in agent-scope 32-bit atomics (min / or / add), and nothing reads those words back before the
// launch ends; everything a kernel reads was written by an EARLIER launch.  No kernel spins, retries a compare-and-swap or waits for
// another workgroup: the host drives the rounds, reads one word back and caps the rounds at n + 1 -- a defect ends in an error code,
// not in a hang.  The same snapshot discipline makes the number of rounds a function of the input.  (It rules out the single-pass
// atomic union-find, which would probably be faster: a deliberate choice.)
//
//   ranks       score == NULL: the identity, nothing runs.  Else two key sorts with the one rocprim::radix_sort_keys<u64> the library
//               instantiates (sets_sort_u64): ~score; then (first place of ~score[v] among the sorted << 32) | v -> order[], rank[].
//   edges       k_cl_check finds the row of every hit once (a bounded binary search of the offsets), refuses a target >= n and counts
//               the hits off the diagonal -- before the result slot is taken over; k_cl_edges maps both ends through rank[] and orients
//               every edge (lower rank first; a diagonal hit has two equal ends and every kernel skips it).
//   components  f[r] = r.  A round: k_cl_hook, a lane per edge (u, v): with fu = f[u], fv = f[v] and fu < fv, atomicMin(fn[fv], fu) and
//               atomicMin(fn[v], fu) (the mirror image for fv < fu); k_cl_jump, a lane per node: fn[v] = min(fn[v], f[f[v]]), one atomicOr
//               per wavefront on a "changed" word, and the new f written to the array the next round reads.  Stops after the first round
//               that changed nothing (counted).  The minimum of a component moves at least one hop a round: n + 1 rounds cannot be reached.
//   greedy      states UNDECIDED / REP / OUT.  A round: k_cl_mis_scan, a lane per edge (u before v) with v UNDECIDED: u REP -> out[v] = 1,
//               u UNDECIDED -> blocked[v] = round (plain stores of a value every writer agrees on); k_cl_mis_apply, a lane per UNDECIDED
//               node: out -> OUT, else not blocked this round -> REP; the nodes still undecided are counted with one atomic per wavefront.
//               The best undecided node is decided every round: at most n rounds (the path ranked from one end to the other takes n).
//               CL_MIS_BATCH rounds go out per read-back; the device records the last round that decided a node.  Then k_cl_assign, a
//               lane per edge with one end REP and the other OUT: atomicMin(best[out end], rep end).
//   grouping    rep-of-node in node space; the flags rep[v] == v through scan_counts -> cluster numbers ascending by representative;
//               label; sizes by atomicAdd (the value does not depend on the order); scan_counts over the sizes -> offsets and the largest;
//               keys (label << 32) | v through sets_sort_u64 -> members.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>

#include "biosketch.h"
#include "host_types.hpp"
#include "search_internal.hpp"
#include "sets_internal.hpp"

#define CL_BLOCK 256
#define CL_MIS_BATCH 8  // greedy rounds per read-back

namespace {

enum : u32 { CL_UNDECIDED = 0, CL_REP = 1, CL_OUT = 2 };
// the figures, one u64 word each (the 32-bit atomics work on the low halves: the device is little-endian)
enum { FIG_BAD = 0, FIG_EDGES = 1, FIG_ROUND = 2, FIG_LAST = 3, FIG_CLUSTERS = 4, FIG_TOTAL = 5, FIG_LARGEST = 6, FIG_WORDS = 8 };

__device__ __forceinline__ u32 *fig32(u64 *fig, int i) { return reinterpret_cast<u32 *>(fig + i); }

// the row of hit h: the last i with off[i] <= h (off[0] = 0 <= h < off[n]; empty rows are passed over).  33 halvings cover n < 2^32.
__device__ __forceinline__ u32 cl_row_of(const u64 *off, u64 n, u64 h) {
    u64 lo = 0, hi = n;
    for (int it = 0; it < 33 && hi - lo > 1; ++it) {
        const u64 mid = (lo + hi) >> 1;
        if (off[mid] <= h) lo = mid;
        else hi = mid;
    }
    return (u32)lo;
}

// ---- the hits: rows, the target check, the count of hits off the diagonal ----
__global__ __launch_bounds__(CL_BLOCK) void k_cl_check(const u64 *off, const u32 *tgt, u64 n, u64 H, u32 *src, u64 *fig) {
    const int lane = threadIdx.x & 63;
    for (u64 b = (u64)blockIdx.x * CL_BLOCK; b < H; b += (u64)gridDim.x * CL_BLOCK) {
        const u64 h = b + threadIdx.x;
        bool bad = false, edge = false;
        if (h < H) {
            const u32 row = cl_row_of(off, n, h), j = tgt[h];
            src[h] = row;
            bad = (u64)j >= n;
            edge = j != row;
        }
        const u64 mb = __ballot(bad), me = __ballot(edge);
        if (lane == 0 && mb) atomicOr(fig32(fig, FIG_BAD), 1u);
        if (lane == 0 && me) atomicAdd(fig32(fig, FIG_EDGES), (u32)__popcll(me));
    }
}

// ---- ranks ----
__global__ __launch_bounds__(CL_BLOCK) void k_cl_score_keys(const u64 *score, u64 n, u64 *keys) {
    for (u64 v = (u64)blockIdx.x * CL_BLOCK + threadIdx.x; v < n; v += (u64)gridDim.x * CL_BLOCK) keys[v] = ~score[v];
}
// (first place of ~score[v] in the sorted keys << 32) | v: equal scores share the first half, the index breaks the tie
__global__ __launch_bounds__(CL_BLOCK) void k_cl_class_keys(const u64 *score, const u64 *sorted, u64 n, u64 *keys) {
    for (u64 v = (u64)blockIdx.x * CL_BLOCK + threadIdx.x; v < n; v += (u64)gridDim.x * CL_BLOCK) {
        const u64 k = ~score[v];
        u64 lo = 0, hi = n;  // the first place whose key is >= k lies in [lo, hi]
        for (int it = 0; it < 33 && lo < hi; ++it) {
            const u64 mid = (lo + hi) >> 1;
            if (sorted[mid] < k) lo = mid + 1;
            else hi = mid;
        }
        keys[v] = (lo << 32) | v;
    }
}
__global__ __launch_bounds__(CL_BLOCK) void k_cl_ranks(const u64 *sorted, u64 n, u32 *order, u32 *rank) {
    for (u64 r = (u64)blockIdx.x * CL_BLOCK + threadIdx.x; r < n; r += (u64)gridDim.x * CL_BLOCK) {
        const u32 v = (u32)sorted[r];  // (a permutation of 0 .. n - 1: every v written once)
        order[r] = v;
        rank[v] = (u32)r;
    }
}

// both ends of every hit in rank space, the better end first (rank == NULL: the identity)
__global__ __launch_bounds__(CL_BLOCK) void k_cl_edges(const u32 *src, const u32 *tgt, const u32 *rank, u64 H, u32 *eu, u32 *ev) {
    for (u64 h = (u64)blockIdx.x * CL_BLOCK + threadIdx.x; h < H; h += (u64)gridDim.x * CL_BLOCK) {
        const u32 i = src[h], j = tgt[h];  // (both < n: k_cl_check)
        const u32 a = rank ? rank[i] : i, b = rank ? rank[j] : j;
        eu[h] = a < b ? a : b;
        ev[h] = a < b ? b : a;
    }
}

// ---- components ----
__global__ __launch_bounds__(CL_BLOCK) void k_cl_init(u64 n, u32 *f, u32 *fn) {
    for (u64 r = (u64)blockIdx.x * CL_BLOCK + threadIdx.x; r < n; r += (u64)gridDim.x * CL_BLOCK) f[r] = fn[r] = (u32)r;
}
__global__ __launch_bounds__(CL_BLOCK) void k_cl_hook(const u32 *eu, const u32 *ev, u64 E, const u32 *f, u32 *fn) {
    for (u64 e = (u64)blockIdx.x * CL_BLOCK + threadIdx.x; e < E; e += (u64)gridDim.x * CL_BLOCK) {
        const u32 u = eu[e], v = ev[e];
        if (u == v) continue;
        const u32 fu = f[u], fv = f[v];
        if (fu < fv) {
            atomicMin(fn + fv, fu);
            atomicMin(fn + v, fu);
        } else if (fv < fu) {
            atomicMin(fn + fu, fv);
            atomicMin(fn + u, fv);
        }
    }
}
// fn[v] is touched by lane v alone here; f is only read (other lanes read f[f[v]]), the new state goes to g, which the next round reads as f
__global__ __launch_bounds__(CL_BLOCK) void k_cl_jump(u64 n, const u32 *f, u32 *fn, u32 *g, u64 *fig) {
    const int lane = threadIdx.x & 63;
    for (u64 b = (u64)blockIdx.x * CL_BLOCK; b < n; b += (u64)gridDim.x * CL_BLOCK) {
        const u64 v = b + threadIdx.x;
        bool changed = false;
        if (v < n) {
            const u32 old = f[v], up = f[old], hooked = fn[v];  // (f[.] <= its index < n)
            const u32 x = hooked < up ? hooked : up;
            fn[v] = x;
            g[v] = x;
            changed = x != old;
        }
        const u64 m = __ballot(changed);
        if (lane == 0 && m) atomicOr(fig32(fig, FIG_ROUND), 1u);
    }
}

// ---- greedy ----
__global__ __launch_bounds__(CL_BLOCK) void k_cl_mis_scan(const u32 *eu, const u32 *ev, u64 E, const u32 *state, u32 *out, u32 *blocked, u32 round) {
    for (u64 e = (u64)blockIdx.x * CL_BLOCK + threadIdx.x; e < E; e += (u64)gridDim.x * CL_BLOCK) {
        const u32 u = eu[e], v = ev[e];  // u before v
        if (u == v || state[v] != CL_UNDECIDED) continue;
        const u32 su = state[u];
        if (su == CL_REP) out[v] = 1u;
        else if (su == CL_UNDECIDED) blocked[v] = round;
    }
}
// count == true in the last round of a batch: the nodes it leaves undecided
__global__ __launch_bounds__(CL_BLOCK) void k_cl_mis_apply(u64 n, u32 *state, const u32 *out, const u32 *blocked, u32 round, bool count, u64 *fig) {
    const int lane = threadIdx.x & 63;
    for (u64 b = (u64)blockIdx.x * CL_BLOCK; b < n; b += (u64)gridDim.x * CL_BLOCK) {
        const u64 v = b + threadIdx.x;
        bool decided = false, left = false;
        if (v < n && state[v] == CL_UNDECIDED) {
            if (out[v]) {
                state[v] = CL_OUT;
                decided = true;
            } else if (blocked[v] != round) {
                state[v] = CL_REP;
                decided = true;
            } else {
                left = true;
            }
        }
        const u64 md = __ballot(decided), ml = __ballot(left);
        if (lane == 0 && md) atomicMax(fig32(fig, FIG_LAST), round);
        if (lane == 0 && count && ml) atomicAdd(fig32(fig, FIG_ROUND), (u32)__popcll(ml));
    }
}
__global__ __launch_bounds__(CL_BLOCK) void k_cl_assign(const u32 *eu, const u32 *ev, u64 E, const u32 *state, u32 *best) {
    for (u64 e = (u64)blockIdx.x * CL_BLOCK + threadIdx.x; e < E; e += (u64)gridDim.x * CL_BLOCK) {
        const u32 u = eu[e], v = ev[e];
        if (u == v) continue;
        const u32 su = state[u], sv = state[v];
        if (su == CL_REP && sv == CL_OUT) atomicMin(best + v, u);
        else if (sv == CL_REP && su == CL_OUT) atomicMin(best + u, v);
    }
}

// ---- grouping ----
// the representative of every node, in node space.  Components: root = f; greedy: a REP is its own, an OUT node has best[] (state != NULL)
__global__ __launch_bounds__(CL_BLOCK) void k_cl_rep(u64 n, const u32 *rank, const u32 *order, const u32 *root, const u32 *state, const u32 *best, u32 *repv) {
    for (u64 v = (u64)blockIdx.x * CL_BLOCK + threadIdx.x; v < n; v += (u64)gridDim.x * CL_BLOCK) {
        const u32 r = rank ? rank[v] : (u32)v;
        u32 x = state ? (state[r] == CL_REP ? r : best[r]) : root[r];
        if ((u64)x >= n) x = r;  // (an OUT node has a REP neighbour: never taken, and no index leaves the arrays)
        repv[v] = order ? order[x] : x;
    }
}
struct IsRep {
    const u32 *repv;
    __device__ __forceinline__ u64 operator()(u64 v) const { return repv[v] == (u32)v ? 1 : 0; }
};
__global__ __launch_bounds__(CL_BLOCK) void k_cl_label(u64 n, const u32 *repv, const u64 *cnum, u32 *label, u32 *rep, u32 *size) {
    for (u64 v = (u64)blockIdx.x * CL_BLOCK + threadIdx.x; v < n; v += (u64)gridDim.x * CL_BLOCK) {
        const u32 p = repv[v], c = (u32)cnum[p];  // (repv[p] == p: c < the number of clusters)
        label[v] = c;
        atomicAdd(size + c, 1u);
        if (p == (u32)v) rep[c] = p;
    }
}
__global__ __launch_bounds__(CL_BLOCK) void k_cl_member_keys(u64 n, const u32 *label, u64 *keys) {
    for (u64 v = (u64)blockIdx.x * CL_BLOCK + threadIdx.x; v < n; v += (u64)gridDim.x * CL_BLOCK) keys[v] = ((u64)label[v] << 32) | v;
}
__global__ __launch_bounds__(CL_BLOCK) void k_cl_members(const u64 *sorted, u64 n, u32 *members) {
    for (u64 i = (u64)blockIdx.x * CL_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * CL_BLOCK) members[i] = (u32)sorted[i];
}

inline u32 bits_of(u64 x) { return x ? 64 - (u32)__builtin_clzll(x) : 0; }  // bits that hold 0 .. x
inline unsigned cl_grid(const bsk_ctx *ctx, u64 items) { return grid_for(ctx, items, CL_BLOCK, 16); }

// the scratch of one call: everything is taken from the pool ONCE, before the first launch (a pool buffer that grows moves)
struct ClScratch {
    u64 *fig = nullptr, *part = nullptr, *cnum = nullptr;
    u32 *order = nullptr, *rank = nullptr, *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr, *repv = nullptr, *size = nullptr;
    u32 *src = nullptr, *eu = nullptr, *ev = nullptr;
    u64 *kin = nullptr, *kout = nullptr, *dscore = nullptr;
    void *stmp = nullptr;
    size_t stmp_bytes = 0;
    unsigned class_bits = 0;
};

int cl_scratch(bsk_ctx *ctx, u64 n, u64 H, bool scored, ClScratch &s) {
    hipStream_t st = ctx->stream;
    Carve cn;
    const size_t o_fig = cn.add<u64>(FIG_WORDS), o_part = cn.add<u64>(scan_parts(n)), o_cnum = cn.add<u64>(n + 1), o_order = cn.add<u32>(n), o_rank = cn.add<u32>(n),
                 o_a = cn.add<u32>(n), o_b = cn.add<u32>(n), o_c = cn.add<u32>(n), o_d = cn.add<u32>(n), o_repv = cn.add<u32>(n), o_size = cn.add<u32>(n + 1);
    Carve ce;
    const size_t o_src = ce.add<u32>(H), o_eu = ce.add<u32>(H), o_ev = ce.add<u32>(H);
    // the sorts: ~score over 64 bits, the class keys and the member keys over the bits of (a number below n, an index below n)
    s.class_bits = 32 + std::max(1u, bits_of(n ? n - 1 : 0));
    size_t tb = 0, t2 = 0;
    HIPCHK(ctx, sets_sort_u64(nullptr, tb, nullptr, nullptr, (size_t)n, 0, s.class_bits, st));
    if (scored) {
        HIPCHK(ctx, sets_sort_u64(nullptr, t2, nullptr, nullptr, (size_t)n, 0, 64, st));
        tb = std::max(tb, t2);
    }
    Carve cs;
    const size_t o_kin = cs.add<u64>(n), o_kout = cs.add<u64>(n), o_score = cs.add<u64>(scored ? n : 0), o_tmp = cs.add<char>(tb ? tb : 8);
    void *bn = nullptr, *be = nullptr, *bs = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_CLUSTER_NODES, cn.bytes, &bn));
    HIPCHK(ctx, ctx_pool(ctx, SLOT_CLUSTER_EDGES, ce.bytes, &be));
    HIPCHK(ctx, ctx_pool(ctx, SLOT_CLUSTER_SORT, cs.bytes, &bs));
    s.fig = at<u64>(bn, o_fig), s.part = at<u64>(bn, o_part), s.cnum = at<u64>(bn, o_cnum);
    s.order = at<u32>(bn, o_order), s.rank = at<u32>(bn, o_rank), s.a = at<u32>(bn, o_a), s.b = at<u32>(bn, o_b), s.c = at<u32>(bn, o_c), s.d = at<u32>(bn, o_d);
    s.repv = at<u32>(bn, o_repv), s.size = at<u32>(bn, o_size);
    s.src = at<u32>(be, o_src), s.eu = at<u32>(be, o_eu), s.ev = at<u32>(be, o_ev);
    s.kin = at<u64>(bs, o_kin), s.kout = at<u64>(bs, o_kout), s.dscore = at<u64>(bs, o_score), s.stmp = at<char>(bs, o_tmp);
    s.stmp_bytes = tb;
    return BSK_OK;
}

int cluster_impl(bsk_ctx *ctx, const bsk_hits *h, u32 method, const uint64_t *score, const ClScratch &s, u64 edges, bsk_clusters *res) {
    hipStream_t st = ctx->stream;
    const u64 n = h->n_queries, H = h->n_hits;
    res->n = n;
    res->n_clusters = res->largest = res->rounds = 0;
    res->edges = edges;
    HIPCHK(ctx, grow_array(&res->label, &res->c_label, (n ? n : 1) * 4));
    HIPCHK(ctx, grow_array(&res->members, &res->c_members, (n ? n : 1) * 4));
    if (n == 0) {
        HIPCHK(ctx, grow_array(&res->rep, &res->c_rep, 4));
        HIPCHK(ctx, grow_array(&res->offsets, &res->c_offsets, 8));
        HIPCHK(ctx, hipMemsetAsync(res->offsets, 0, 8, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        snprintf(res->plan, sizeof res->plan, "%s, n=0 edges=0 rounds=0", method == BSK_CLUSTER_GREEDY ? "k_cl_mis" : "k_cl_hook+k_cl_jump");
        return BSK_OK;
    }
    const unsigned gn = cl_grid(ctx, n), ge = cl_grid(ctx, H);
    size_t tb = s.stmp_bytes;
    // 1. ranks
    const u32 *rank = nullptr, *order = nullptr;
    if (score) {
        HIPCHK(ctx, hipMemcpyAsync(s.dscore, score, n * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_cl_score_keys, dim3(gn), dim3(CL_BLOCK), 0, st, (const u64 *)s.dscore, n, s.kin);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, sets_sort_u64(s.stmp, tb, s.kin, s.kout, (size_t)n, 0, 64, st));
        hipLaunchKernelGGL(k_cl_class_keys, dim3(gn), dim3(CL_BLOCK), 0, st, (const u64 *)s.dscore, (const u64 *)s.kout, n, s.kin);
        HIPCHK(ctx, hipGetLastError());
        tb = s.stmp_bytes;
        HIPCHK(ctx, sets_sort_u64(s.stmp, tb, s.kin, s.kout, (size_t)n, 0, s.class_bits, st));
        hipLaunchKernelGGL(k_cl_ranks, dim3(gn), dim3(CL_BLOCK), 0, st, (const u64 *)s.kout, n, s.order, s.rank);
        HIPCHK(ctx, hipGetLastError());
        rank = s.rank, order = s.order;
    }
    // 2. edges in rank space
    if (H) {
        hipLaunchKernelGGL(k_cl_edges, dim3(ge), dim3(CL_BLOCK), 0, st, (const u32 *)s.src, (const u32 *)h->target, rank, H, s.eu, s.ev);
        HIPCHK(ctx, hipGetLastError());
    }
    u64 rounds = 0;
    const u64 cap = n + 1;
    const u32 *root = nullptr, *state = nullptr, *best = nullptr;
    if (method == BSK_CLUSTER_COMPONENTS) {
        // 3. hook + jump until a round changes nothing
        u32 *f = s.a, *fn = s.b, *g = s.c;
        hipLaunchKernelGGL(k_cl_init, dim3(gn), dim3(CL_BLOCK), 0, st, n, f, fn);
        HIPCHK(ctx, hipGetLastError());
        for (;;) {
            if (rounds == cap) {
                ctx->err = "bsk_hits_cluster: the components did not settle in n + 1 rounds";
                return BSK_ERR_DEVICE;
            }
            HIPCHK(ctx, hipMemsetAsync(s.fig + FIG_ROUND, 0, 8, st));
            if (H) hipLaunchKernelGGL(k_cl_hook, dim3(ge), dim3(CL_BLOCK), 0, st, (const u32 *)s.eu, (const u32 *)s.ev, H, (const u32 *)f, fn);
            hipLaunchKernelGGL(k_cl_jump, dim3(gn), dim3(CL_BLOCK), 0, st, n, (const u32 *)f, fn, g, s.fig);
            HIPCHK(ctx, hipGetLastError());
            HIPCHK(ctx, read_back(ctx, s.fig + FIG_ROUND, 1));
            ++rounds;
            std::swap(f, g);  // fn == the new f: the next hook starts from it
            if (ctx->h_pinned[0] == 0) break;
        }
        root = f;
    } else {
        // 4. scan + apply until no node is undecided, CL_MIS_BATCH rounds per read-back
        u32 *st8 = s.a, *out = s.b, *blocked = s.c, *bst = s.d;
        HIPCHK(ctx, hipMemsetAsync(st8, 0, n * 4, st));
        HIPCHK(ctx, hipMemsetAsync(out, 0, n * 4, st));
        HIPCHK(ctx, hipMemsetAsync(blocked, 0, n * 4, st));
        HIPCHK(ctx, hipMemsetAsync(bst, 0xff, n * 4, st));
        HIPCHK(ctx, hipMemsetAsync(s.fig + FIG_LAST, 0, 8, st));
        u64 issued = 0;
        for (;;) {
            if (issued == cap) {
                ctx->err = "bsk_hits_cluster: nodes left undecided after n + 1 rounds";
                return BSK_ERR_DEVICE;
            }
            const u64 batch = std::min<u64>(CL_MIS_BATCH, cap - issued);
            HIPCHK(ctx, hipMemsetAsync(s.fig + FIG_ROUND, 0, 8, st));
            for (u64 i = 0; i < batch; ++i) {
                const u32 round = (u32)(issued + i + 1);  // (<= n + 1 <= 2^32)
                if (H) hipLaunchKernelGGL(k_cl_mis_scan, dim3(ge), dim3(CL_BLOCK), 0, st, (const u32 *)s.eu, (const u32 *)s.ev, H, (const u32 *)st8, out, blocked, round);
                hipLaunchKernelGGL(k_cl_mis_apply, dim3(gn), dim3(CL_BLOCK), 0, st, n, st8, (const u32 *)out, (const u32 *)blocked, round, i + 1 == batch, s.fig);
            }
            HIPCHK(ctx, hipGetLastError());
            HIPCHK(ctx, read_back(ctx, s.fig + FIG_ROUND, 2));
            issued += batch;
            if ((u32)ctx->h_pinned[0] == 0) break;
        }
        rounds = (u32)ctx->h_pinned[1];
        if (H) {
            hipLaunchKernelGGL(k_cl_assign, dim3(ge), dim3(CL_BLOCK), 0, st, (const u32 *)s.eu, (const u32 *)s.ev, H, (const u32 *)st8, bst);
            HIPCHK(ctx, hipGetLastError());
        }
        state = st8, best = bst;
    }
    // 5. grouping
    hipLaunchKernelGGL(k_cl_rep, dim3(gn), dim3(CL_BLOCK), 0, st, n, rank, order, root, state, best, s.repv);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemsetAsync(s.fig + FIG_CLUSTERS, 0, 3 * 8, st));
    HIPCHK(ctx, scan_counts(st, IsRep{s.repv}, n, s.part, s.cnum, s.fig + FIG_CLUSTERS, (u64 *)nullptr));
    HIPCHK(ctx, read_back(ctx, s.fig + FIG_CLUSTERS, 1));
    const u64 nc = ctx->h_pinned[0];
    if (nc == 0 || nc > n) {
        ctx->err = "bsk_hits_cluster: a cluster count outside 1 .. n";
        return BSK_ERR_DEVICE;
    }
    HIPCHK(ctx, grow_array(&res->rep, &res->c_rep, nc * 4));
    HIPCHK(ctx, grow_array(&res->offsets, &res->c_offsets, (nc + 1) * 8));
    HIPCHK(ctx, hipMemsetAsync(s.size, 0, nc * 4, st));
    hipLaunchKernelGGL(k_cl_label, dim3(gn), dim3(CL_BLOCK), 0, st, n, (const u32 *)s.repv, (const u64 *)s.cnum, res->label, res->rep, s.size);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, scan_counts(st, KeepOf{s.size}, nc, s.part, res->offsets, s.fig + FIG_TOTAL, s.fig + FIG_LARGEST));
    hipLaunchKernelGGL(k_cl_member_keys, dim3(gn), dim3(CL_BLOCK), 0, st, n, (const u32 *)res->label, s.kin);
    HIPCHK(ctx, hipGetLastError());
    tb = s.stmp_bytes;
    HIPCHK(ctx, sets_sort_u64(s.stmp, tb, s.kin, s.kout, (size_t)n, 0, 32 + std::max(1u, bits_of(nc - 1)), st));
    hipLaunchKernelGGL(k_cl_members, dim3(gn), dim3(CL_BLOCK), 0, st, (const u64 *)s.kout, n, res->members);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, read_back(ctx, s.fig + FIG_TOTAL, 2));
    if (ctx->h_pinned[0] != n) {
        ctx->err = "bsk_hits_cluster: the cluster sizes do not sum to n";
        return BSK_ERR_DEVICE;
    }
    res->n_clusters = nc;
    res->largest = ctx->h_pinned[1];
    res->rounds = rounds;
    snprintf(res->plan, sizeof res->plan, "%s, n=%llu edges=%llu rounds=%llu", method == BSK_CLUSTER_GREEDY ? "k_cl_mis" : "k_cl_hook+k_cl_jump", (unsigned long long)n,
             (unsigned long long)edges, (unsigned long long)rounds);
    return BSK_OK;
}

}  // namespace

extern "C" void bsk_clusters_release(bsk_clusters *c) {
    if (!c) return;
    if (c->ctx) (void)hipSetDevice(c->ctx->device);
    (void)hipFree(c->label);
    (void)hipFree(c->rep);
    (void)hipFree(c->offsets);
    (void)hipFree(c->members);
    delete c;
}

extern "C" int bsk_hits_cluster(bsk_ctx *ctx, const bsk_hits *h, const bsk_cluster_params *cp, const uint64_t *score, bsk_clusters **out) {
    if (!ctx || !h || !out) return fail_arg(ctx, "bsk_hits_cluster: null argument");
    const u32 method = cp ? cp->method : (u32)BSK_CLUSTER_COMPONENTS;
    if (method != BSK_CLUSTER_COMPONENTS && method != BSK_CLUSTER_GREEDY) return fail_arg(ctx, "bsk_hits_cluster: unknown method");
    if (cp && cp->flags != 0) return fail_arg(ctx, "bsk_hits_cluster: unknown flag");
    if (h->ctx != ctx || (*out && (*out)->ctx != ctx)) return fail_arg(ctx, "bsk_hits_cluster: the hits or the clusters belong to another context");
    const u64 n = h->n_queries, H = h->n_hits;
    if (n >= (1ULL << 32) || H >= (1ULL << 32)) {
        ctx->err = "bsk_hits_cluster: 2^32 nodes or hits or more (split the graph)";
        return BSK_ERR_UNSUPPORTED;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the scratch and the one pass over the hits that can refuse them: before the slot is taken over, *out stays as it was
    ClScratch s;
    u64 edges = 0;
    if (n) {
        const int rc = cl_scratch(ctx, n, H, score != nullptr, s);
        if (rc != BSK_OK) return rc;
        HIPCHK(ctx, hipMemsetAsync(s.fig, 0, FIG_WORDS * 8, ctx->stream));
        if (H) {
            hipLaunchKernelGGL(k_cl_check, dim3(cl_grid(ctx, H)), dim3(CL_BLOCK), 0, ctx->stream, (const u64 *)h->offsets, (const u32 *)h->target, n, H, s.src, s.fig);
            HIPCHK(ctx, hipGetLastError());
        }
        HIPCHK(ctx, read_back(ctx, s.fig + FIG_BAD, 2));
        if (ctx->h_pinned[0]) return fail_arg(ctx, "bsk_hits_cluster: a target >= n_queries (the hits are not those of a set against itself)");
        edges = ctx->h_pinned[1];
    }
    return take_over(ctx, out, bsk_clusters_release, [&](bsk_clusters *res, bool) { return cluster_impl(ctx, h, method, score, s, edges, res); });
}

extern "C" int bsk_clusters_info(const bsk_clusters *c, uint64_t *n_items, uint64_t *n_clusters, uint64_t *largest) {
    if (!c) return BSK_ERR_ARG;
    if (n_items) *n_items = c->n;
    if (n_clusters) *n_clusters = c->n_clusters;
    if (largest) *largest = c->largest;
    return BSK_OK;
}

extern "C" int bsk_clusters_plan(const bsk_clusters *c, const char **plan, uint64_t figures[2]) {
    if (!c) return BSK_ERR_ARG;
    if (plan) *plan = c->plan;
    if (figures) figures[0] = c->rounds, figures[1] = c->edges;
    return BSK_OK;
}

extern "C" int bsk_clusters_device(const bsk_clusters *c, const uint32_t **label, const uint32_t **rep, const uint64_t **offsets, const uint32_t **members) {
    if (!c) return BSK_ERR_ARG;
    if (label) *label = (const uint32_t *)c->label;
    if (rep) *rep = (const uint32_t *)c->rep;
    if (offsets) *offsets = (const uint64_t *)c->offsets;
    if (members) *members = (const uint32_t *)c->members;
    return BSK_OK;
}

extern "C" int bsk_clusters_fetch(bsk_ctx *ctx, const bsk_clusters *c, uint32_t *label, uint32_t *rep, uint64_t *offsets, uint32_t *members) {
    if (!ctx || !c) return fail_arg(ctx, "bsk_clusters_fetch: null argument");
    if (c->ctx != ctx) return fail_arg(ctx, "bsk_clusters_fetch: the clusters belong to another context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (label && c->n) HIPCHK(ctx, hipMemcpyAsync(label, c->label, c->n * 4, hipMemcpyDeviceToHost, st));
    if (rep && c->n_clusters) HIPCHK(ctx, hipMemcpyAsync(rep, c->rep, c->n_clusters * 4, hipMemcpyDeviceToHost, st));
    if (offsets) HIPCHK(ctx, hipMemcpyAsync(offsets, c->offsets, (c->n_clusters + 1) * 8, hipMemcpyDeviceToHost, st));
    if (members && c->n) HIPCHK(ctx, hipMemcpyAsync(members, c->members, c->n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return BSK_OK;
}
