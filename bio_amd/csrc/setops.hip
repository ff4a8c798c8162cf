// setops.hip -- set algebra on bsk_sets: union / intersection / difference / symmetric difference of two collections pair by pair
// (or of every set of a collection with one broadcast set), and the reduction of runs of consecutive sets to the values that at
// least m of their members hold.  What unikmer's union / inter / diff do on disk, done where the sets already are: a multi-contig
// genome is the union of its contigs' sets, a read pair the union of its mates', a masked read its set minus the host's.
//
// bsk_sets_op is a MERGE, not a sort: both inputs are sorted and distinct.  A pair is classified by t = |a_i| + |b_i|:
//   t <= SO_GROUP_CAP  k_so_group  a group of 16 lanes per pair (four pairs per wavefront), the pair's values in LDS
//   t <= SO_WAVE_CAP   k_so_wave   one wavefront per pair, both sets in LDS (8 KB per wavefront, four per workgroup)
//   beyond             k_so_tile   the merged sequence is cut into tiles of SO_TILE consecutive merged ranks; a binary search along
//                                  each tile's diagonal (merge path; on a tie a's element comes first) gives the tile's start in
//                                  a_i and b_i (k_so_cuts, a thread per tile), and one wavefront per tile runs the wave kernel's
//                                  body on its two slices
// All three run ONE body (so_merge): the lanes take consecutive merged ranks, a rank finds its element by a short merge-path
// search over the two slices in LDS, so_rank decides whether the op keeps it, and a ballot gives the kept elements their places:
// the output leaves in order, in whole lines.  Every kernel runs twice: a count pass (per pair, per tile for tiled pairs), the
// library's scan over the counts, then the same kernel in write mode, where every value lands at its final place -- no staging
// span, no compaction: the inputs are read twice (8 t bytes each time) and the output written once.
//
// The tile rule.  A value both sets hold sits at two neighbouring merged ranks, a's copy first, and a tile boundary can fall
// between them.  so_rank decides every rank from its own element and ONE look at the other set: for an element of a the first
// element of b that does not precede it, for an element of b the last element of a that does.  Inside a tile that neighbour is
// in the other slice -- or it is the one element next to the slice (SoEdge: a[a0 - 1] before the a slice, b[b1] behind the
// b slice), which the tile loads besides its slices.  Count and write mode call the same so_rank, so they cannot disagree.
//
// bsk_sets_reduce: the members of a group are consecutive sets, so a group's values are one contiguous range of the values
// array; sets.hip's segmented radix sort orders every range, and since member sets are distinct a value's run length is the
// number of members that hold it: element i is kept iff it heads its run and v[i + m - 1] is in the same range and equal.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <cstdio>
#include <new>

#include "biosketch.h"
#include "host_types.hpp"
#include "sets_internal.hpp"

#define SO_GROUP_CAP 64     // t up to which a pair takes 16 lanes (a pair of 150-base reads' minimizer sets: t ~ 44)
#define SO_WAVE_CAP 1024    // t up to which a pair takes one wavefront: 8 KB of LDS
#define SO_TILE SO_WAVE_CAP // merged ranks per tile of a larger pair
// grid caps, in workgroups of 256 threads per compute unit (the kernels loop over the rest)
#define SO_GROUP_BLOCKS_PER_CU 32  // 16 pairs per workgroup
#define SO_WAVE_BLOCKS_PER_CU 16   // 4 pairs per workgroup
#define SO_TILE_BLOCKS_PER_CU 3    // 4 tiles per workgroup
#define SO_WAVES 4
#define RD_CHUNK 2048       // elements per workgroup trip of k_rd_flags

namespace {

// where pair p's two sets are (bstep 0: every set of a against b's only set)
struct SoSpan {
    const u64 *ao, *bo;
    u64 bstep;
    __device__ __forceinline__ void get(u64 p, u64 &a0, u32 &na, u64 &b0, u32 &nb) const {
        a0 = ao[p];
        na = (u32)(ao[p + 1] - a0);
        b0 = bo[p * bstep];
        nb = (u32)(bo[p * bstep + 1] - b0);
    }
    __device__ __forceinline__ u64 t(u64 p) const { return (ao[p + 1] - ao[p]) + (bo[p * bstep + 1] - bo[p * bstep]); }
};
// bsk_sets_op_counted's pairs: a second step factor (astep 0: a's only set against every set of b -- one sample against every genome)
struct SoSpanAB {
    const u64 *ao, *bo;
    u64 astep, bstep;
    __device__ __forceinline__ void get(u64 p, u64 &a0, u32 &na, u64 &b0, u32 &nb) const {
        a0 = ao[p * astep];
        na = (u32)(ao[p * astep + 1] - a0);
        b0 = bo[p * bstep];
        nb = (u32)(bo[p * bstep + 1] - b0);
    }
    __device__ __forceinline__ u64 t(u64 p) const { return (ao[p * astep + 1] - ao[p * astep]) + (bo[p * bstep + 1] - bo[p * bstep]); }
};
// the counts that ride along in a counted write pass: an operand without counts (NULL) counts 1 for every value
struct SoCounts {
    const u32 *ca = nullptr, *cb = nullptr;
    u32 *out = nullptr;
};
template <class SP>
struct SoWaveOf {  // 1 for the pairs of k_so_wave
    SP s;
    __device__ __forceinline__ u64 operator()(u64 p) const {
        const u64 t = s.t(p);
        return t > SO_GROUP_CAP && t <= SO_WAVE_CAP ? 1 : 0;
    }
};
template <class SP>
struct SoTilesOf {  // tiles of a pair of k_so_tile (tiled: only whether it has any)
    SP s;
    bool tiled;
    __device__ __forceinline__ u64 operator()(u64 p) const {
        const u64 t = s.t(p);
        return t > SO_WAVE_CAP ? (tiled ? 1 : (t + SO_TILE - 1) / SO_TILE) : 0;
    }
};
struct SoPairCount {  // what a pair keeps: its own count, or the sum over its tiles
    const u64 *cnt, *tfirst, *tpos;
    __device__ __forceinline__ u64 operator()(u64 p) const {
        const u64 f = tfirst[p], e = tfirst[p + 1];
        return e > f ? tpos[e] - tpos[f] : cnt[p];
    }
};

// ---- the rule: does `op` keep an element, given the set it comes from and whether the other set holds the same value ----
__device__ __forceinline__ bool so_keep(int op, bool from_a, bool matched) {
    if (from_a) return op == BSK_SETOP_UNION ? true : op == BSK_SETOP_INTERSECT ? matched : !matched;
    return (op == BSK_SETOP_UNION || op == BSK_SETOP_SYMDIFF) && !matched;  // (a's copy stands for a shared value)
}
// the elements next to a tile's slices (a whole pair has none)
struct SoEdge {
    u64 a_prev = 0, b_next = 0;  // a[a0 - 1], b[b1]
    bool has_prev = false, has_next = false;
};
// number of elements of A among the first r merged ones (merge path; A[i] precedes B[j] iff A[i] <= B[j]), known to lie in [from, from + span]
__device__ __forceinline__ u32 so_diag(const u64 *A, u32 na, const u64 *B, u32 nb, u32 r, u32 from, u32 span) {
    u32 lo = r > nb ? r - nb : 0, hi = r < na ? r : na;
    lo = lo > from ? lo : from;
    hi = hi - from > span ? from + span : hi;  // (from <= hi: from is the answer for a smaller rank)
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (A[mid] <= B[r - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ u32 so_diag(const u64 *A, u32 na, const u64 *B, u32 nb, u32 r) { return so_diag(A, na, B, nb, r, 0, na); }
// merged rank r of the slices A[0 .. na), B[0 .. nb), of which i elements of A precede it: its value, the slice it comes from, and
// whether `op` keeps it.  Used by the count AND the write pass.
__device__ __forceinline__ bool so_rank(const u64 *A, u32 na, const u64 *B, u32 nb, const SoEdge &e, u32 r, u32 i, int op, u64 &x, bool &from_a) {
    const u32 j = r - i;
    from_a = i < na && (j >= nb || A[i] <= B[j]);
    bool matched;
    if (from_a) {  // its copy in b, if any, is the first element of b that does not precede it: B[j], or the one behind the slice
        x = A[i];
        matched = j < nb ? B[j] == x : (e.has_next && e.b_next == x);
    } else {  // its copy in a, if any, is the last element of a that precedes it: A[i - 1], or the one before the slice
        x = B[j];
        matched = i > 0 ? A[i - 1] == x : (e.has_prev && e.a_prev == x);
    }
    return so_keep(op, from_a, matched);
}
// the same rule for the counted kernels, which also need to know whether the other set holds the value (the partner whose count ADD adds)
__device__ __forceinline__ bool so_rank(const u64 *A, u32 na, const u64 *B, u32 nb, const SoEdge &e, u32 r, u32 i, int op, u64 &x, bool &from_a, bool &matched) {
    const u32 j = r - i;
    from_a = i < na && (j >= nb || A[i] <= B[j]);
    if (from_a) {  // its copy in b, if any, is the first element of b that does not precede it: B[j], or the one behind the slice
        x = A[i];
        matched = j < nb ? B[j] == x : (e.has_next && e.b_next == x);
    } else {  // its copy in a, if any, is the last element of a that precedes it: A[i - 1], or the one before the slice
        x = B[j];
        matched = i > 0 ? A[i - 1] == x : (e.has_prev && e.a_prev == x);
    }
    return so_keep(op, from_a, matched);
}
// LANES (16: a row of the wavefront, bits [shift, shift + 16) of a ballot; 64: all of it) take the merged ranks in order; tmax:
// a bound of t that is the same in every lane of the wavefront.  Lane l's rank lies l ranks behind the first of its trip, whose
// count of A's elements (i0) the trip before left behind: the merge-path search spans l + 1 candidates, log2(LANES) steps at most.
// Returns the number of kept elements.
template <int LANES, bool WRITE>
__device__ __forceinline__ u32 so_merge(const u64 *A, u32 na, const u64 *B, u32 nb, const SoEdge &e, int op, u32 tmax, int l, int shift, u64 *dst) {
    const u32 t = na + nb;
    u32 base = 0, i0 = 0;
    for (u32 r0 = 0; r0 < tmax; r0 += LANES) {
        const u32 r = r0 + (u32)l;
        u64 x = 0;
        bool from_a = false, keep = false;
        if (r < t) keep = so_rank(A, na, B, nb, e, r, so_diag(A, na, B, nb, r, i0, (u32)l), op, x, from_a);
        u64 bits = __ballot(keep), abits = __ballot(from_a);
        if (LANES == 16) {
            bits = (bits >> shift) & 0xffffull;
            abits = (abits >> shift) & 0xffffull;
        }
        if (WRITE && keep) dst[base + (u32)__builtin_popcountll(bits & ((1ull << l) - 1ull))] = x;
        base += (u32)__builtin_popcountll(bits);
        i0 += (u32)__builtin_popcountll(abits);
    }
    return base;
}
// The counted body (bsk_sets_op_counted): the same trips; in write mode the kept element's count goes to c.out beside its value.  c.ca /
// c.cb point at the counts of A[0] / B[0] in global memory (NULL: every count is 1), c.out at the counts of dst[0].  An element of a that
// b holds adds its partner's count under BSK_COUNTOP_ADD -- the partner so_rank matched it with, B[j], which for j == nb is the edge
// element behind the b slice: cb[nb], read by index like any other.
template <int LANES, bool WRITE>
__device__ __forceinline__ u32 so_merge(const u64 *A, u32 na, const u64 *B, u32 nb, const SoEdge &e, int op, u32 tmax, int l, int shift, u64 *dst, SoCounts c) {
    const u32 t = na + nb;
    u32 base = 0, i0 = 0;
    for (u32 r0 = 0; r0 < tmax; r0 += LANES) {
        const u32 r = r0 + (u32)l;
        u64 x = 0;
        bool from_a = false, keep = false, matched = false;
        u32 i = 0;
        if (r < t) {
            i = so_diag(A, na, B, nb, r, i0, (u32)l);
            keep = so_rank(A, na, B, nb, e, r, i, op, x, from_a, matched);
        }
        u64 bits = __ballot(keep), abits = __ballot(from_a);
        if (LANES == 16) {
            bits = (bits >> shift) & 0xffffull;
            abits = (abits >> shift) & 0xffffull;
        }
        if (WRITE && keep) {
            const u32 slot = base + (u32)__builtin_popcountll(bits & ((1ull << l) - 1ull)), j = r - i;
            dst[slot] = x;
            u64 n;
            if (from_a) {
                n = c.ca ? c.ca[i] : 1u;
                if (op == BSK_COUNTOP_ADD && matched) n += c.cb ? c.cb[j] : 1u;
            } else {
                n = c.cb ? c.cb[j] : 1u;
            }
            c.out[slot] = n > 0xffffffffull ? 0xffffffffu : (u32)n;  // ADD saturates
        }
        base += (u32)__builtin_popcountll(bits);
        i0 += (u32)__builtin_popcountll(abits);
    }
    return base;
}
// the counts of a slice that starts a0 / b0 / o values into a's, b's and the output's arrays
__device__ __forceinline__ SoCounts so_counts_at(SoCounts c, u64 a0, u64 b0, u64 o) {
    return SoCounts{c.ca ? c.ca + a0 : nullptr, c.cb ? c.cb + b0 : nullptr, c.out ? c.out + o : nullptr};
}

// The three kernels take the counts as a trailing parameter PACK: bsk_sets_op launches them with an empty one -- the signatures, the
// kernel arguments and the body (the first so_merge above) are those of the uncounted library --, bsk_sets_op_counted with one SoCounts.
// ---- t <= SO_GROUP_CAP: a group of 16 lanes per pair ----
template <bool WRITE, class SP = SoSpan, class... C>
__global__ __launch_bounds__(256) void k_so_group(SP sp, const u64 *av, const u64 *bv, u64 n, int op, u64 *cnt, const u64 *ooff, u64 *out, C... sc) {
    __shared__ u64 lds[16][SO_GROUP_CAP];
    const int lane = threadIdx.x & 63, l = lane & 15, row = lane >> 4;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((u64)gridDim.x * blockDim.x) >> 6;
    u64 *A = lds[threadIdx.x >> 4];
    for (u64 p0 = wave * 4; p0 < n; p0 += nw * 4) {  // (the same trip count in the four rows: so_merge's ballots are wave-wide)
        const u64 p = p0 + (u64)row;
        u64 a0 = 0, b0 = 0;
        u32 na = 0, nb = 0;
        bool mine = false;
        if (p < n) {
            sp.get(p, a0, na, b0, nb);
            mine = (u64)na + nb <= SO_GROUP_CAP;
            if (!mine) na = nb = 0;
        }
        for (u32 e = (u32)l; e < na + nb; e += 16) A[e] = e < na ? av[a0 + e] : bv[b0 + (e - na)];
        wave_sync_lds();
        const u32 c = so_merge<16, WRITE>(A, na, A + na, nb, SoEdge{}, op, SO_GROUP_CAP, l, row * 16, WRITE && mine ? out + ooff[p] : nullptr,
                                          so_counts_at(sc, a0, b0, WRITE && mine ? ooff[p] : 0)...);
        if (!WRITE && mine && l == 0) cnt[p] = c;
        wave_sync_lds();
    }
}

// ---- t <= SO_WAVE_CAP: one wavefront per pair of the list ----
template <bool WRITE, class SP = SoSpan, class... C>
__global__ __launch_bounds__(64 * SO_WAVES) void k_so_wave(SP sp, const u64 *av, const u64 *bv, const u32 *list, u64 nlist, int op, u64 *cnt, const u64 *ooff,
                                                           u64 *out, C... sc) {
    __shared__ u64 lds[SO_WAVES][SO_WAVE_CAP];
    const int lane = threadIdx.x & 63;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((u64)gridDim.x * blockDim.x) >> 6;
    u64 *A = lds[threadIdx.x >> 6];
    for (u64 s = wave; s < nlist; s += nw) {
        const u64 p = list[s];
        u64 a0, b0;
        u32 na, nb;
        sp.get(p, a0, na, b0, nb);
        for (u32 e = (u32)lane; e < na + nb; e += 64) A[e] = e < na ? av[a0 + e] : bv[b0 + (e - na)];
        wave_sync_lds();
        const u32 c = so_merge<64, WRITE>(A, na, A + na, nb, SoEdge{}, op, na + nb, lane, 0, WRITE ? out + ooff[p] : nullptr, so_counts_at(sc, a0, b0, WRITE ? ooff[p] : 0)...);
        if (!WRITE && lane == 0) cnt[p] = c;
        wave_sync_lds();
    }
}

// ---- beyond: one wavefront per tile of SO_TILE merged ranks ----
// tfirst[p]: the first tile of pair p (exclusive scan of the pairs' tile counts: pairs of the other kernels have none).
// k_so_cuts, a thread per tile, once per call: the tile's pair (the last p with tfirst[p] <= tile: it owns tiles, tfirst[p + 1] > tile)
// and where the tile starts in a_i (merge path along the tile's first diagonal; its start in b_i is the rest of the rank).  Twenty
// dependent loads a tile -- hidden behind a million threads here, exposed in a kernel of twelve wavefronts per CU (the first version
// searched inside k_so_tile, in both passes: 22.0 ms for P3 of DESIGN 3.7).
template <class SP>
__global__ void k_so_cuts(SP sp, const u64 *av, const u64 *bv, const u64 *tfirst, u64 n, u64 ntiles, u32 *tpair, u32 *ta0) {
    for (u64 tile = (u64)blockIdx.x * blockDim.x + threadIdx.x; tile < ntiles; tile += (u64)gridDim.x * blockDim.x) {
        u64 lo = 0, hi = n - 1;
        while (lo < hi) {
            const u64 mid = (lo + hi + 1) >> 1;
            if (tfirst[mid] <= tile) lo = mid;
            else hi = mid - 1;
        }
        u64 pa, pb;
        u32 na, nb;
        sp.get(lo, pa, na, pb, nb);
        tpair[tile] = (u32)lo;
        ta0[tile] = so_diag(av + pa, na, bv + pb, nb, (u32)(tile - tfirst[lo]) * SO_TILE);
    }
}
template <bool WRITE, class SP = SoSpan, class... C>
__global__ __launch_bounds__(64 * SO_WAVES) void k_so_tile(SP sp, const u64 *av, const u64 *bv, const u64 *tfirst, const u32 *tpair, const u32 *ta0, u64 ntiles, int op,
                                                           u64 *tcnt, const u64 *tpos, const u64 *ooff, u64 *out, C... sc) {
    __shared__ u64 lds[SO_WAVES][SO_TILE];
    const int lane = threadIdx.x & 63;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((u64)gridDim.x * blockDim.x) >> 6;
    u64 *A = lds[threadIdx.x >> 6];
    for (u64 tile = wave; tile < ntiles; tile += nw) {
        const u64 p = tpair[tile], t0 = tfirst[p];
        u64 pa, pb;
        u32 na, nb;
        sp.get(p, pa, na, pb, nb);
        const u32 t = na + nb, r0 = (u32)(tile - t0) * SO_TILE, r1 = t - r0 > SO_TILE ? r0 + SO_TILE : t;
        const u32 a0 = ta0[tile], a1 = r1 == t ? na : ta0[tile + 1];  // (the pair's next tile starts where this one ends)
        const u32 b0 = r0 - a0, b1 = r1 - a1;
        SoEdge e;
        e.has_prev = a0 > 0;
        e.has_next = b1 < nb;
        if (e.has_prev) e.a_prev = av[pa + a0 - 1];
        if (e.has_next) e.b_next = bv[pb + b1];
        const u32 sa = a1 - a0, sb = b1 - b0;  // sa + sb = r1 - r0 <= SO_TILE
        for (u32 i = (u32)lane; i < sa + sb; i += 64) A[i] = i < sa ? av[pa + a0 + i] : bv[pb + b0 + (i - sa)];
        wave_sync_lds();
        const u32 c = so_merge<64, WRITE>(A, sa, A + sa, sb, e, op, sa + sb, lane, 0, WRITE ? out + ooff[p] + (tpos[tile] - tpos[t0]) : nullptr,
                                          so_counts_at(sc, pa + a0, pb + b0, WRITE ? ooff[p] + (tpos[tile] - tpos[t0]) : 0)...);
        if (!WRITE && lane == 0) tcnt[tile] = c;
        wave_sync_lds();
    }
}

template <class SP>
__global__ void k_so_list(SoWaveOf<SP> f, const u64 *slot, u64 n, u32 *list) {
    for (u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (u64)gridDim.x * blockDim.x)
        if (f(p)) list[slot[p]] = (u32)p;
}

// ---- bsk_sets_reduce ----
// value offsets of the groups: goff[g] = offsets[group_offsets[g]]
__global__ void k_rd_goff(const u64 *offs, const u64 *gmem, u64 ng1, u64 *goff) {
    for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g < ng1; g += (u64)gridDim.x * blockDim.x) goff[g] = offs[gmem[g]];
}
// the last g of [lo, hi] with goff[g] <= i (goff[lo] <= i)
__device__ __forceinline__ u64 rd_group_of(const u64 *goff, u64 lo, u64 hi, u64 i) {
    while (lo < hi) {
        const u64 mid = (lo + hi + 1) >> 1;
        if (goff[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// keep[i] = 1 iff sorted value i heads its run and the run reaches m elements inside its group's range: ONE comparison with
// v[i + m - 1].  m: min_members, or the group's member count (BSK_MEMBERS_ALL).  A workgroup brackets the groups of its RD_CHUNK
// elements once, every element then searches that bracket only.
__global__ __launch_bounds__(256) void k_rd_flags(const u64 *v, u64 N, const u64 *goff, const u64 *gmem, u64 G, u32 min_members, u32 *keep) {
    for (u64 c0 = (u64)blockIdx.x * RD_CHUNK; c0 < N; c0 += (u64)gridDim.x * RD_CHUNK) {
        const u64 c1 = c0 + RD_CHUNK < N ? c0 + RD_CHUNK : N;
        const u64 glo = rd_group_of(goff, 0, G - 1, c0), ghi = rd_group_of(goff, glo, G - 1, c1 - 1);
        for (u64 i = c0 + threadIdx.x; i < c1; i += 256) {
            const u64 g = rd_group_of(goff, glo, ghi, i), first = goff[g], end = goff[g + 1];
            const u64 m = min_members == BSK_MEMBERS_ALL ? gmem[g + 1] - gmem[g] : (u64)min_members;  // >= 1: the group has an element
            const u64 x = v[i];
            keep[i] = ((i == first || v[i - 1] != x) && m - 1 < end - i && v[i + (m - 1)] == x) ? 1u : 0u;
        }
    }
}
__global__ void k_rd_scatter(const u64 *v, const u32 *keep, const u64 *pos, u64 n, u64 *out) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        if (keep[i]) out[pos[i]] = v[i];
}
__global__ void k_rd_offsets(const u64 *goff, const u64 *pos, u64 G, u64 n_in, u64 n_out, u64 *offs_out) {
    for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g <= G; g += (u64)gridDim.x * blockDim.x)
        offs_out[g] = goff[g] < n_in ? pos[goff[g]] : n_out;
}

// SP = SoSpan, COUNTED = false: bsk_sets_op; SoSpanAB, true: bsk_sets_op_counted (the count pass is the same, the write pass also
// writes res->counts)
template <class SP, bool COUNTED>
int op_impl(bsk_ctx *ctx, const SP sp, const u64 n, bool broadcast, const bsk_sets *a, const bsk_sets *b, int op, bsk_sets *res) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    res->n_sets = n;
    res->n_values = 0;
    res->counted = false;
    res->plan[0] = 0;
    res->by_path[0] = res->by_path[1] = res->by_path[2] = 0;
    HIPCHK(ctx, grow_array(&res->offsets, &res->c_offsets, (n + 1) * 8));
    if (n == 0) {
        HIPCHK(ctx, grow_array(&res->values, &res->c_values, 8));
        if (COUNTED) HIPCHK(ctx, sets_grow_counts(res, 1, true));
        HIPCHK(ctx, hipMemsetAsync(res->offsets, 0, 8, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        res->counted = COUNTED;
        snprintf(res->plan, sizeof res->plan, "%s: no pairs", COUNTED ? "bsk_sets_op_counted" : "bsk_sets_op");
        return BSK_OK;
    }
    Carve cp;
    const size_t o_wslot = cp.add<u64>(n + 1), o_tfirst = cp.add<u64>(n + 1), o_tslot = cp.add<u64>(n + 1), o_cnt = cp.add<u64>(n), o_part = cp.add<u64>(scan_parts(n)),
                 o_tot = cp.add<u64>(8), o_list = cp.add<u32>(n);
    void *bp = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_OP_PAIRS, cp.bytes, &bp));
    u64 *wslot = at<u64>(bp, o_wslot), *tfirst = at<u64>(bp, o_tfirst), *tslot = at<u64>(bp, o_tslot), *cnt = at<u64>(bp, o_cnt), *part = at<u64>(bp, o_part),
        *tot = at<u64>(bp, o_tot);
    u32 *list = at<u32>(bp, o_list);
    HIPCHK(ctx, hipMemsetAsync(tot, 0, 64, st));  // [0] wave pairs, [1] tiles, [2] tiled pairs, [3] values of the tiles, [4] values
    // 1. the classes: the wave kernel's list, the tiled pairs' first tiles
    HIPCHK(ctx, scan_counts(st, SoWaveOf<SP>{sp}, n, part, wslot, tot + 0, (u64 *)nullptr));
    HIPCHK(ctx, scan_counts(st, SoTilesOf<SP>{sp, false}, n, part, tfirst, tot + 1, (u64 *)nullptr));
    HIPCHK(ctx, scan_counts(st, SoTilesOf<SP>{sp, true}, n, part, tslot, tot + 2, (u64 *)nullptr));
    HIPCHK(ctx, read_back(ctx, tot, 3));
    const u64 NW = ctx->h_pinned[0], NT = ctx->h_pinned[1], NTP = ctx->h_pinned[2], NG = n - NW - NTP;
    u64 *tcnt = nullptr, *tpos = nullptr, *part2 = nullptr;
    u32 *tpair = nullptr, *ta0 = nullptr;
    if (NT) {
        Carve ct;
        const size_t o_tcnt = ct.add<u64>(NT), o_tpos = ct.add<u64>(NT + 1), o_part2 = ct.add<u64>(scan_parts(NT)), o_tpair = ct.add<u32>(NT), o_ta0 = ct.add<u32>(NT);
        void *bt = nullptr;
        HIPCHK(ctx, ctx_pool(ctx, SLOT_OP_TILES, ct.bytes, &bt));
        tcnt = at<u64>(bt, o_tcnt);
        tpos = at<u64>(bt, o_tpos);
        part2 = at<u64>(bt, o_part2);
        tpair = at<u32>(bt, o_tpair);
        ta0 = at<u32>(bt, o_ta0);
        hipLaunchKernelGGL(k_so_cuts<SP>, dim3(grid_for(ctx, NT, 256, 16)), dim3(256), 0, st, sp, a->values, b->values, tfirst, n, NT, tpair, ta0);
    }
    if (NW) hipLaunchKernelGGL(k_so_list<SP>, dim3(grid_for(ctx, n, 256, 16)), dim3(256), 0, st, SoWaveOf<SP>{sp}, wslot, n, list);
    const unsigned g_group = grid_for(ctx, n, 16, SO_GROUP_BLOCKS_PER_CU), g_wave = grid_for(ctx, NW, SO_WAVES, SO_WAVE_BLOCKS_PER_CU),
                   g_tile = grid_for(ctx, NT, SO_WAVES, SO_TILE_BLOCKS_PER_CU);
    // 2. count pass
    if (NG) hipLaunchKernelGGL((k_so_group<false, SP>), dim3(g_group), dim3(256), 0, st, sp, a->values, b->values, n, op, cnt, (const u64 *)nullptr, (u64 *)nullptr);
    if (NW)
        hipLaunchKernelGGL((k_so_wave<false, SP>), dim3(g_wave), dim3(64 * SO_WAVES), 0, st, sp, a->values, b->values, list, NW, op, cnt, (const u64 *)nullptr, (u64 *)nullptr);
    if (NT)
        hipLaunchKernelGGL((k_so_tile<false, SP>), dim3(g_tile), dim3(64 * SO_WAVES), 0, st, sp, a->values, b->values, tfirst, tpair, ta0, NT, op, tcnt, (const u64 *)nullptr,
                           (const u64 *)nullptr, (u64 *)nullptr);
    HIPCHK(ctx, hipGetLastError());
    // 3. the tiles' places inside their pairs, the pairs' places in the output
    if (NT) HIPCHK(ctx, scan_counts(st, ArrayOf{tcnt}, NT, part2, tpos, tot + 3, (u64 *)nullptr));
    HIPCHK(ctx, scan_counts(st, SoPairCount{cnt, tfirst, tpos}, n, part, res->offsets, tot + 4, (u64 *)nullptr));
    HIPCHK(ctx, read_back(ctx, tot + 4, 1));
    const u64 M = ctx->h_pinned[0];
    HIPCHK(ctx, grow_array(&res->values, &res->c_values, (M ? M : 1) * 8));
    if (COUNTED) HIPCHK(ctx, sets_grow_counts(res, M ? M : 1, true));
    // 4. write pass: the same kernels, every kept value to its final place (c: nothing, or the counts that ride along)
    auto write = [&](auto... c) {
        if (NG)
            hipLaunchKernelGGL((k_so_group<true, SP, decltype(c)...>), dim3(g_group), dim3(256), 0, st, sp, a->values, b->values, n, op, (u64 *)nullptr, res->offsets, res->values, c...);
        if (NW)
            hipLaunchKernelGGL((k_so_wave<true, SP, decltype(c)...>), dim3(g_wave), dim3(64 * SO_WAVES), 0, st, sp, a->values, b->values, list, NW, op, (u64 *)nullptr, res->offsets,
                               res->values, c...);
        if (NT)
            hipLaunchKernelGGL((k_so_tile<true, SP, decltype(c)...>), dim3(g_tile), dim3(64 * SO_WAVES), 0, st, sp, a->values, b->values, tfirst, tpair, ta0, NT, op, (u64 *)nullptr, tpos,
                               res->offsets, res->values, c...);
    };
    if (M) {
        if constexpr (COUNTED) write(SoCounts{a->counted ? a->counts : nullptr, b->counted ? b->counts : nullptr, res->counts});
        else write();
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    res->n_values = M;
    res->counted = COUNTED;
    res->by_path[0] = NG;
    res->by_path[1] = NW;
    res->by_path[2] = NTP;
    static const char *const names[4] = {"union", "intersect", "diff", "symdiff"};
    static const char *const cnames[3] = {"add", "keep", "drop"};
    snprintf(res->plan, sizeof res->plan, "%s %s%s: k_so_group (t <= %d) %llu pairs, k_so_wave (t <= %d) %llu, k_so_tile %llu pairs in %llu tiles of %d",
             COUNTED ? "bsk_sets_op_counted" : "bsk_sets_op", COUNTED ? cnames[op] : names[op], broadcast ? " (broadcast)" : "", SO_GROUP_CAP, (unsigned long long)NG, SO_WAVE_CAP, (unsigned long long)NW, (unsigned long long)NTP, (unsigned long long)NT,
             SO_TILE);
    return BSK_OK;
}

int reduce_impl(bsk_ctx *ctx, const bsk_sets *s, const uint64_t *group_offsets, u64 G, u32 min_members, bsk_sets *res) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u64 N = s->n_values;
    res->n_sets = G;
    res->n_values = 0;
    res->counted = false;
    res->plan[0] = 0;
    res->by_path[0] = res->by_path[1] = res->by_path[2] = 0;
    HIPCHK(ctx, grow_array(&res->offsets, &res->c_offsets, (G + 1) * 8));
    if (G == 0 || N == 0) {
        HIPCHK(ctx, grow_array(&res->values, &res->c_values, 8));
        HIPCHK(ctx, hipMemsetAsync(res->offsets, 0, (G + 1) * 8, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        snprintf(res->plan, sizeof res->plan, "bsk_sets_reduce: no values");
        return BSK_OK;
    }
    Carve cg;
    const size_t o_gmem = cg.add<u64>(G + 1), o_goff = cg.add<u64>(G + 1), o_tot = cg.add<u64>(8);
    Carve cv;
    const size_t o_pos = cv.add<u64>(N + 1), o_part = cv.add<u64>(scan_parts(N)), o_keep = cv.add<u32>(N);
    void *bg = nullptr, *bsorted = nullptr, *bv = nullptr, *btmp = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_REDUCE_GROUPS, cg.bytes, &bg));
    HIPCHK(ctx, ctx_pool(ctx, SLOT_REDUCE_SORTED, N * 8, &bsorted));
    HIPCHK(ctx, ctx_pool(ctx, SLOT_REDUCE_VALUES, cv.bytes, &bv));
    u64 *gmem = at<u64>(bg, o_gmem), *goff = at<u64>(bg, o_goff), *tot = at<u64>(bg, o_tot), *sorted = static_cast<u64 *>(bsorted), *pos = at<u64>(bv, o_pos),
        *part = at<u64>(bv, o_part);
    u32 *keep = at<u32>(bv, o_keep);
    HIPCHK(ctx, hipMemsetAsync(tot, 0, 64, st));
    HIPCHK(ctx, hipMemcpyAsync(gmem, group_offsets, (G + 1) * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_rd_goff, dim3(grid_for(ctx, G + 1, 256, 16)), dim3(256), 0, st, s->offsets, gmem, G + 1, goff);
    HIPCHK(ctx, hipGetLastError());
    // every group's range of the values array, sorted (sets.hip's instantiation of the segmented radix sort)
    size_t tb = 0;
    HIPCHK(ctx, sets_sort_segments_u64(nullptr, tb, s->values, sorted, N, G, goff, st));
    HIPCHK(ctx, ctx_pool(ctx, SLOT_REDUCE_SORT_TMP, tb ? tb : 8, &btmp));
    HIPCHK(ctx, sets_sort_segments_u64(btmp, tb, s->values, sorted, N, G, goff, st));
    hipLaunchKernelGGL(k_rd_flags, dim3(grid_for(ctx, N, RD_CHUNK, 16)), dim3(256), 0, st, sorted, N, goff, gmem, G, min_members, keep);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, scan_counts(st, KeepOf{keep}, N, part, pos, tot, (u64 *)nullptr));
    HIPCHK(ctx, read_back(ctx, tot, 1));  // (the caller's group_offsets are not needed past this point)
    const u64 M = ctx->h_pinned[0];
    HIPCHK(ctx, grow_array(&res->values, &res->c_values, (M ? M : 1) * 8));
    if (M) hipLaunchKernelGGL(k_rd_scatter, dim3(grid_for(ctx, N, 256, 16)), dim3(256), 0, st, sorted, keep, pos, N, res->values);
    hipLaunchKernelGGL(k_rd_offsets, dim3(grid_for(ctx, G + 1, 256, 16)), dim3(256), 0, st, goff, pos, G, N, M, res->offsets);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));
    res->n_values = M;
    if (min_members == BSK_MEMBERS_ALL)
        snprintf(res->plan, sizeof res->plan, "bsk_sets_reduce: %llu groups, segmented sort + run test, every member", (unsigned long long)G);
    else
        snprintf(res->plan, sizeof res->plan, "bsk_sets_reduce: %llu groups, segmented sort + run test, >= %u members", (unsigned long long)G, min_members);
    return BSK_OK;
}

}  // namespace

extern "C" int bsk_sets_op(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, int op, bsk_sets **out) {
    if (!ctx || !a || !b || !out) return fail_arg(ctx, "bsk_sets_op: null argument");
    if (a->ctx != ctx || b->ctx != ctx || (*out && (*out)->ctx != ctx)) return fail_arg(ctx, "bsk_sets_op: the sets belong to another context");
    if (*out == a || *out == b) return fail_arg(ctx, "bsk_sets_op: *out is one of the inputs");
    if (op != BSK_SETOP_UNION && op != BSK_SETOP_INTERSECT && op != BSK_SETOP_DIFF && op != BSK_SETOP_SYMDIFF) return fail_arg(ctx, "bsk_sets_op: unknown op");
    if (b->n_sets != a->n_sets && b->n_sets != 1) return fail_arg(ctx, "bsk_sets_op: b must hold as many sets as a, or exactly one");
    if (a->n_sets >= (1ULL << 32) || a->n_values + b->n_values >= (1ULL << 32)) {
        ctx->err = "bsk_sets_op: 2^32 sets or values or more (split the sets)";
        return BSK_ERR_UNSUPPORTED;
    }
    const u64 n = a->n_sets;
    const SoSpan sp{a->offsets, b->offsets, b->n_sets == n ? 1ull : 0ull};
    return take_over(ctx, out, bsk_sets_release, [&](bsk_sets *res, bool) { return op_impl<SoSpan, false>(ctx, sp, n, sp.bstep == 0, a, b, op, res); });
}

// The counted algebra: BSK_COUNTOP_ADD / KEEP / DROP are union / intersection / difference on the values (the same numbers as
// BSK_SETOP_*), the write pass also writes every kept value's count.  Pairing as bsk_sets_op, and besides: an a of exactly one set
// against a b of n sets gives n sets, a op b[i].
extern "C" int bsk_sets_op_counted(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, int op, bsk_sets **out) {
    static_assert(BSK_COUNTOP_ADD == BSK_SETOP_UNION && BSK_COUNTOP_KEEP == BSK_SETOP_INTERSECT && BSK_COUNTOP_DROP == BSK_SETOP_DIFF, "so_keep takes the op as it is");
    if (!ctx || !a || !b || !out) return fail_arg(ctx, "bsk_sets_op_counted: null argument");
    if (a->ctx != ctx || b->ctx != ctx || (*out && (*out)->ctx != ctx)) return fail_arg(ctx, "bsk_sets_op_counted: the sets belong to another context");
    if (*out == a || *out == b) return fail_arg(ctx, "bsk_sets_op_counted: *out is one of the inputs");
    if (op != BSK_COUNTOP_ADD && op != BSK_COUNTOP_KEEP && op != BSK_COUNTOP_DROP) return fail_arg(ctx, "bsk_sets_op_counted: unknown op");
    if (b->n_sets != a->n_sets && b->n_sets != 1 && a->n_sets != 1) return fail_arg(ctx, "bsk_sets_op_counted: a and b must hold as many sets, or one of them exactly one");
    const u64 n = b->n_sets == a->n_sets || b->n_sets == 1 ? a->n_sets : b->n_sets;
    if (n >= (1ULL << 32) || a->n_values + b->n_values >= (1ULL << 32)) {
        ctx->err = "bsk_sets_op_counted: 2^32 sets or values or more (split the sets)";
        return BSK_ERR_UNSUPPORTED;
    }
    const SoSpanAB sp{a->offsets, b->offsets, a->n_sets == n ? 1ull : 0ull, b->n_sets == n ? 1ull : 0ull};
    return take_over(ctx, out, bsk_sets_release, [&](bsk_sets *res, bool) { return op_impl<SoSpanAB, true>(ctx, sp, n, sp.astep == 0 || sp.bstep == 0, a, b, op, res); });
}

extern "C" int bsk_sets_reduce(bsk_ctx *ctx, const bsk_sets *s, const uint64_t *group_offsets, uint64_t n_groups, uint32_t min_members, bsk_sets **out) {
    if (!ctx || !s || !group_offsets || !out) return fail_arg(ctx, "bsk_sets_reduce: null argument");
    if (s->ctx != ctx || (*out && (*out)->ctx != ctx)) return fail_arg(ctx, "bsk_sets_reduce: the sets belong to another context");
    if (*out == s) return fail_arg(ctx, "bsk_sets_reduce: *out is the input");
    if (min_members == 0) return fail_arg(ctx, "bsk_sets_reduce: min_members == 0");
    if (group_offsets[0] != 0) return fail_arg(ctx, "bsk_sets_reduce: group_offsets[0] != 0");
    for (u64 g = 0; g < n_groups; ++g)
        if (group_offsets[g + 1] < group_offsets[g]) return fail_arg(ctx, "bsk_sets_reduce: group_offsets decrease");
    if (group_offsets[n_groups] != s->n_sets) return fail_arg(ctx, "bsk_sets_reduce: group_offsets must end at the number of sets");
    if (s->n_sets >= (1ULL << 32) || s->n_values >= (1ULL << 32) || n_groups >= (1ULL << 32)) {
        ctx->err = "bsk_sets_reduce: 2^32 sets, groups or values or more (split the sets)";
        return BSK_ERR_UNSUPPORTED;
    }
    return take_over(ctx, out, bsk_sets_release, [&](bsk_sets *res, bool) { return reduce_impl(ctx, s, group_offsets, n_groups, min_members, res); });
}

extern "C" int bsk_sets_plan(const bsk_sets *s, const char **plan, uint64_t n_by_path[3]) {
    if (!s) return BSK_ERR_ARG;
    if (plan) *plan = s->plan;
    if (n_by_path)
        for (int i = 0; i < 3; ++i) n_by_path[i] = s->by_path[i];
    return BSK_OK;
}
