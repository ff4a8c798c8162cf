// search.hip -- containment search of sketch sets against a device-resident inverted index (include/biosketch.h "containment
// search").  For every query set q and target set t: s = |q & t|, listed when it passes the caller's thresholds; CSR hits by query.
// This is what a kmcp-style consumer does with the sets bsk_result_sets leaves on the device -- the sets never cross the link, only
// the hits do.
//
// Index (bsk_index_build): every (value, target) posting gets the key mix64(value) -- a bijection, so distinct values stay distinct
// keys, and the keys are uniform whatever the values are (k-mer codes of k = 11 live in the low 22 bits, host-loaded sets can be
// clustered: a directory over raw top bits would put them all in bucket 0).  One rocprim::radix_sort_pairs<u64, u32> of
// (key, target): the sort is stable and the input is target-major, so the targets of a key leave ascending.  Run-length of the keys
// -> keys[U], post_off[U + 1], post_tgt[P]; a directory dir[2^b + 1] of bucket starts over the top b bits of the key, 2^b <= U <
// 2^(b+1): one or two keys per bucket on average (a lookup scans its whole bucket, however full).
//
// Search (bsk_index_search): A. lookups, a group of 16 lanes per query -- mix, one directory entry, a bucket scan -- store every
// query value's posting range and the query's sum of posting lengths (coalesced); B. scans of those sums give every query a staging
// span (its hits are at most min(sum, targets)); C. one wavefront per query copies the target ids of its postings into LDS, sorts
// them (bitonic), counts the runs, applies the threshold and writes (target, shared) ascending into its span; then a scan of the hit
// counts and a move.  Queries whose sum exceeds the LDS budget (SR_CAP: a genome against genomes, a value held by thousands of
// targets) are listed and take the large path: (slot << 32) | target keys, the rocprim::radix_sort_keys<u64> sets.hip already
// instantiates, run-length, threshold.  Exact, and no new template.
//
// With counts (bsk_index_build_counted, bsk_index_search_counted): the build sorts (key, posting number) with the same instantiation and one
// gather fills post_tgt and post_cnt from the permutation; the search runs as it is, and a payload pass over rng[] and the finished rows adds
// cq * ct and min(cq, ct) of every posting whose target the row lists -- in LDS for small-path rows of at most SW_ROW hits (k_sw_row), with
// 64-bit atomics for chunks of SW_CHUNK values of everything else (k_sw_chunk).  DESIGN.md 3.16.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "biosketch.h"
#include "host_types.hpp"
#include "search_internal.hpp"
#include "sets_internal.hpp"

// The device arrays of an index, on one device: read-only once built, shared by every handle of that device (bsk_index_attach) and
// freed when the last of them is released.
struct IndexArrays {
    std::atomic<int> refs{1};
    int device = 0;
    u64 *keys = nullptr;       // [U] distinct mixed keys, ascending
    u32 *post_off = nullptr;   // [U + 1] postings of key u: post_tgt[post_off[u] .. post_off[u + 1])
    u32 *post_tgt = nullptr;   // [P] target ids, ascending inside a key
    u32 *dir = nullptr;        // [2^bits + 1] first key of every bucket
    u32 *tsize = nullptr;      // [n_targets] |t|
    // a counted index (bsk_index_build_counted of counted sets) only; NULL otherwise
    u32 *post_cnt = nullptr;   // [P] the target's count of the key's value, parallel to post_tgt
    u64 *tsumsq = nullptr;     // [n_targets] sum of t's squared counts, saturating (bsk_sets_sumsq)
    u64 *ttotal = nullptr;     // [n_targets] sum of t's counts (bsk_sets_totals)
};
struct bsk_index {
    bsk_ctx *ctx = nullptr;    // the context this handle is searched on (never dereferenced by a release: it may be gone by then)
    u64 n_targets = 0, n_postings = 0, n_distinct = 0, max_bucket = 0, device_bytes = 0;
    int bits = 0;              // directory over the top `bits` bits of the mixed key
    bool counted = false;      // the arrays hold post_cnt, tsumsq and ttotal
    IndexArrays *a = nullptr;
};

#define SR_CAP 2048  // target ids pass C holds per query: 8 KB of LDS per wavefront
#define SR_WAVES 4   // wavefronts per workgroup of pass C
// the payload pass of bsk_index_search_counted
#define SW_ROW 512    // hits of a small-path query whose (target, dot, min_sum) row one wavefront holds in LDS: 10 KB
#define SW_WAVES 4    // wavefronts per workgroup of k_sw_row: 40 KB of LDS, four workgroups a CU
#define SW_CHUNK 256  // query values one wavefront of k_sw_chunk walks (four trips of 64 lanes)

namespace {

// splitmix64's finalizer: every step (xor-shift, odd multiply) is invertible, so distinct values keep distinct keys
__device__ __forceinline__ u64 mix64(u64 x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
}
__device__ __forceinline__ u64 bucket_of(u64 key, int bits) { return bits ? key >> (64 - bits) : 0; }

struct Thr {
    u32 min_shared;
    double qc, tc;
};
// the contract's expression, term for term (no sum: nothing the compiler could contract)
__device__ __forceinline__ bool listed(u32 s, u64 qn, u32 tn, const Thr &p) {
    return s >= p.min_shared && (double)s >= p.qc * (double)qn && (double)s >= p.tc * (double)tn;
}

// ---- index build ----
// posting i -> (mix64(value), its target); the target by a binary search over the sets' offsets (a thread per posting: a group per
// target left most of the device idle on a thousand genome-size targets)
__global__ __launch_bounds__(256) void k_ix_pairs(const u64 *offs, const u64 *vals, u64 T, u64 P, u64 *key, u32 *tgt) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (u64)gridDim.x * blockDim.x) {
        u64 lo = 0, hi = T;  // the last set whose first value is <= i: offs[lo] <= i < offs[lo + 1]
        while (hi - lo > 1) {
            const u64 mid = (lo + hi) >> 1;
            if (offs[mid] <= i) lo = mid;
            else hi = mid;
        }
        key[i] = mix64(vals[i]);
        tgt[i] = (u32)lo;
    }
}
__global__ __launch_bounds__(256) void k_ix_sizes(const u64 *offs, u64 T, u32 *tsize) {
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (u64)gridDim.x * blockDim.x) tsize[t] = (u32)(offs[t + 1] - offs[t]);
}
// flag[i] = 1 iff key i starts a run of equal keys
__global__ __launch_bounds__(256) void k_run_heads(const u64 *k, u64 n, u32 *flag) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) flag[i] = (i == 0 || k[i] != k[i - 1]) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_ix_scatter(const u64 *k, const u32 *flag, const u64 *pos, u64 P, u64 *keys, u32 *post_off) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (u64)gridDim.x * blockDim.x) {
        if (flag[i]) {
            keys[pos[i]] = k[i];
            post_off[pos[i]] = (u32)i;
        }
        if (i == 0) post_off[pos[P]] = (u32)P;
    }
}
// dir[j] = the first key whose bucket is >= j (j = 0 .. 2^bits): key u writes the entries between its predecessor's bucket and its own
__global__ __launch_bounds__(256) void k_ix_dir(const u64 *keys, u64 U, int bits, u32 *dir) {
    for (u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x; u <= U; u += (u64)gridDim.x * blockDim.x) {
        const u64 b = u < U ? bucket_of(keys[u], bits) : (1ULL << bits);
        const u64 j0 = u == 0 ? 0 : bucket_of(keys[u - 1], bits) + 1;
        for (u64 j = j0; j <= b; ++j) dir[j] = (u32)u;
    }
}
__global__ __launch_bounds__(256) void k_ix_maxb(const u32 *dir, u64 nb, u64 *mx) {
    u32 m = 0;
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < nb; j += (u64)gridDim.x * blockDim.x) {
        const u32 d = dir[j + 1] - dir[j];
        m = d > m ? d : m;
    }
    m = wave_max_u32(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax((unsigned long long *)mx, (unsigned long long)m);
}
// the counted build sorts (key, posting number) instead of (key, target): ord[i] = i going in, the permutation coming out -- the sort is
// stable, so the postings of a key leave in posting order, which is target order -- and one gather fills both posting arrays from it
__global__ __launch_bounds__(256) void k_ix_ord(u64 P, u32 *ord) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (u64)gridDim.x * blockDim.x) ord[i] = (u32)i;
}
__global__ __launch_bounds__(256) void k_ix_gather(const u32 *perm, const u32 *tgt, const u32 *cnt, u64 P, u32 *post_tgt, u32 *post_cnt) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (u64)gridDim.x * blockDim.x) {
        const u32 j = perm[i];  // < P: a permutation of 0 .. P - 1
        post_tgt[i] = tgt[j];
        post_cnt[i] = cnt[j];
    }
}

// ---- search ----
// A: a group of 16 lanes per query; rng[i] = (first posting << 32) | posting count of query value i (0: not in the index),
// qsum[q] = the query's sum of posting counts
__global__ __launch_bounds__(256) void k_sr_lookup(const u64 *qoff, const u64 *qvals, u64 nq, const u64 *keys, const u32 *post_off, const u32 *dir,
                                                   int bits, u64 *rng, u64 *qsum) {
    const u64 grp = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 4, ng = ((u64)gridDim.x * blockDim.x) >> 4;
    const u32 l = threadIdx.x & 15;
    for (u64 q = grp; q < nq; q += ng) {
        const u64 a = qoff[q], e = qoff[q + 1];
        u64 sum = 0;
        for (u64 i = a + l; i < e; i += 16) {
            const u64 k = mix64(qvals[i]);
            const u64 j = bucket_of(k, bits);
            const u32 lo = dir[j], hi = dir[j + 1];
            u64 r = 0;
            for (u32 u = lo; u < hi; ++u) {
                const u64 ku = keys[u];
                if (ku >= k) {
                    if (ku == k) {
                        const u32 s = post_off[u];
                        r = ((u64)s << 32) | (post_off[u + 1] - s);
                    }
                    break;
                }
            }
            rng[i] = r;
            sum += (u32)r;
        }
        sum += __shfl_xor(sum, 8, 16);
        sum += __shfl_xor(sum, 4, 16);
        sum += __shfl_xor(sum, 2, 16);
        sum += __shfl_xor(sum, 1, 16);
        if (l == 0) qsum[q] = sum;
    }
}
struct StageOf {  // a query's staging span: it lists at most min(sum of its posting counts, targets) hits
    const u64 *qsum;
    u64 T;
    __device__ __forceinline__ u64 operator()(u64 q) const { return qsum[q] < T ? qsum[q] : T; }
};
struct LargeOf {  // queries beyond pass C's LDS: their count (count_only) or their target ids
    const u64 *qsum;
    bool count_only;
    __device__ __forceinline__ u64 operator()(u64 q) const { return qsum[q] > SR_CAP ? (count_only ? 1 : qsum[q]) : 0; }
};
__global__ __launch_bounds__(256) void k_sr_list_large(const u64 *qsum, u64 nq, const u64 *lslot, u32 *lq) {
    for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (u64)gridDim.x * blockDim.x)
        if (qsum[q] > SR_CAP) lq[lslot[q]] = (u32)q;
}

// C: one wavefront per query of at most SR_CAP target ids: collect them in LDS, bitonic sort, runs = shared counts, threshold,
// (target, shared) ascending into the query's staging span; hcnt[q] = hits (0 for the large queries: the large path overwrites it)
__global__ __launch_bounds__(64 * SR_WAVES) void k_sr_small(const u64 *qoff, const u64 *rng, const u64 *qsum, u64 nq, const u32 *post_tgt,
                                                            const u32 *tsize, const u64 *stage_off, Thr thr, u32 *st_tgt, u32 *st_sh, u64 *hcnt) {
    __shared__ u32 lds[SR_WAVES][SR_CAP];
    u32 *buf = lds[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    const u64 lt_mask = (1ULL << lane) - 1;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 q = wave; q < nq; q += nw) {
        const u64 n64 = qsum[q];
        if (n64 == 0 || n64 > SR_CAP) {
            if (lane == 0) hcnt[q] = 0;
            continue;
        }
        const u32 n = (u32)n64;
        const u64 a = qoff[q], e = qoff[q + 1];
        u32 base = 0;
        for (u64 i0 = a; i0 < e; i0 += 64) {
            const u64 i = i0 + lane;
            const u64 r = i < e ? rng[i] : 0;
            const u32 len = (u32)r, s = (u32)(r >> 32);
            const u32 incl = wave_incl_scan_u32(len, lane);
            const u32 d = base + incl - len;  // d + len <= n <= SR_CAP: the sums are the lookups' own
            for (u32 t = 0; t < len; ++t) buf[d + t] = post_tgt[s + t];
            base += (u32)__builtin_amdgcn_readlane((int)incl, 63);
        }
        const u32 n2 = n <= 1 ? 1u : 1u << (32 - __builtin_clz(n - 1));  // <= SR_CAP (a power of two)
        for (u32 i = n + lane; i < n2; i += 64) buf[i] = 0xffffffffu;  // (target ids are < 2^32 - 1)
        wave_sync_lds();
        for (u32 k = 2; k <= n2; k <<= 1) {
            for (u32 j = k >> 1; j > 0; j >>= 1) {
                for (u32 i = lane; i < n2; i += 64) {
                    const u32 p = i ^ j;
                    if (p > i) {
                        const u32 x = buf[i], y = buf[p];
                        if ((x > y) == ((i & k) == 0)) {
                            buf[i] = y;
                            buf[p] = x;
                        }
                    }
                }
                wave_sync_lds();
            }
        }
        const u64 out = stage_off[q], qn = e - a;
        u32 nh = 0;
        for (u32 i0 = 0; i0 < n; i0 += 64) {
            const u32 i = i0 + lane;
            bool keep = false;
            u32 x = 0, c = 0;
            if (i < n) {
                x = buf[i];
                if (i == 0 || buf[i - 1] != x) {
                    c = 1;
                    while (i + c < n && buf[i + c] == x) ++c;
                    keep = listed(c, qn, tsize[x], thr);
                }
            }
            const u64 m = __ballot(keep);
            if (keep) {
                const u64 o = out + nh + (u32)__builtin_popcountll(m & lt_mask);
                st_tgt[o] = x;
                st_sh[o] = c;
            }
            nh += (u32)__builtin_popcountll(m);
        }
        if (lane == 0) hcnt[q] = nh;
        wave_sync_lds();  // every lane is done with the buffer before the next query fills it
    }
}

// large path: one wavefront per listed query writes (slot << 32) | target for every posting of its values at loff[q]; values with
// long posting lists (a value held by thousands of targets) are copied by the whole wavefront
__global__ __launch_bounds__(256) void k_lg_emit(const u64 *qoff, const u64 *rng, const u32 *lq, u64 nl, const u64 *loff, const u32 *post_tgt, u64 *lkeys) {
    const int lane = threadIdx.x & 63;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 slot = wave; slot < nl; slot += nw) {
        const u32 q = lq[slot];
        const u64 a = qoff[q], e = qoff[q + 1], hi = slot << 32;
        u64 dst = loff[q];
        for (u64 i0 = a; i0 < e; i0 += 64) {
            const u64 i = i0 + lane;
            const u64 r = i < e ? rng[i] : 0;
            const u32 len = (u32)r, s = (u32)(r >> 32);
            const u32 incl = wave_incl_scan_u32(len, lane);  // (the ranges of distinct values are disjoint: sums stay below 2^32)
            const u32 ex = incl - len;
            if (len <= 64)
                for (u32 t = 0; t < len; ++t) lkeys[dst + ex + t] = hi | post_tgt[s + t];
            u64 big = __ballot(len > 64);
            while (big) {
                const int src = __builtin_ctzll(big);
                big &= big - 1;
                const u32 s2 = (u32)__builtin_amdgcn_readlane((int)s, src), len2 = (u32)__builtin_amdgcn_readlane((int)len, src),
                          ex2 = (u32)__builtin_amdgcn_readlane((int)ex, src);
                for (u32 t = lane; t < len2; t += 64) lkeys[dst + ex2 + t] = hi | post_tgt[s2 + t];
            }
            dst += (u32)__builtin_amdgcn_readlane((int)incl, 63);
        }
    }
}
// rstart[ridx[i]] = i at every run head of the sorted keys, rstart[R] = L
__global__ __launch_bounds__(256) void k_lg_runs(const u32 *flag, const u64 *ridx, u64 L, u64 *rstart) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < L; i += (u64)gridDim.x * blockDim.x) {
        if (flag[i]) rstart[ridx[i]] = i;
        if (i == 0) rstart[ridx[L]] = L;
    }
}
// run r = (slot, target) shared by rstart[r + 1] - rstart[r] values: keep[r] (0 for r >= R), sfirst[slot] = its first run
__global__ __launch_bounds__(256) void k_lg_keep(const u64 *k, const u64 *rstart, const u64 *ridx, u64 L, const u32 *lq, const u64 *qoff, const u32 *tsize,
                                                 Thr thr, u32 *keep, u64 *sfirst) {
    const u64 R = ridx[L];
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < L; r += (u64)gridDim.x * blockDim.x) {
        if (r >= R) {
            keep[r] = 0;
            continue;
        }
        const u64 s0 = rstart[r], key = k[s0], slot = key >> 32;
        const u32 q = lq[slot];
        keep[r] = listed((u32)(rstart[r + 1] - s0), qoff[q + 1] - qoff[q], tsize[(u32)key], thr) ? 1u : 0u;
        if (r == 0 || (k[rstart[r - 1]] >> 32) != slot) sfirst[slot] = r;
    }
}
__global__ __launch_bounds__(256) void k_lg_place(const u64 *k, const u64 *rstart, const u64 *ridx, u64 L, const u32 *keep, const u64 *kpos, const u64 *sfirst,
                                                  const u32 *lq, const u64 *stage_off, u32 *st_tgt, u32 *st_sh, u64 *hcnt) {
    const u64 R = ridx[L];
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (u64)gridDim.x * blockDim.x) {
        const u64 s0 = rstart[r], key = k[s0], slot = key >> 32;
        const u32 q = lq[slot];
        const u64 f = kpos[sfirst[slot]];
        if (keep[r]) {
            const u64 o = stage_off[q] + (kpos[r] - f);
            st_tgt[o] = (u32)key;
            st_sh[o] = (u32)(rstart[r + 1] - s0);
        }
        if (r + 1 == R || (k[rstart[r + 1]] >> 32) != slot) hcnt[q] = kpos[r + 1] - f;
    }
}

// final placement: query q's hits [stage_off[q], +hcnt[q]) -> [off[q], ...); a group of 16 lanes per query
__global__ __launch_bounds__(256) void k_sr_move(const u64 *stage_off, const u64 *off, const u64 *hcnt, u64 nq, const u32 *st_tgt, const u32 *st_sh,
                                                 u32 *tgt, u32 *sh) {
    const u64 grp = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 4, ng = ((u64)gridDim.x * blockDim.x) >> 4;
    for (u64 q = grp; q < nq; q += ng) {
        const u64 s0 = stage_off[q], d0 = off[q], c = hcnt[q];
        for (u64 i = threadIdx.x & 15; i < c; i += 16) {
            tgt[d0 + i] = st_tgt[s0 + i];
            sh[d0 + i] = st_sh[s0 + i];
        }
    }
}

// ---- the payload pass of bsk_index_search_counted: dot and min_sum of every listed pair ----
// The search has finished: rng[] and qsum[] are still in the pool, the hits' rows are in place.  For every posting (t, ct) of every query
// value (v, cq) the pass looks t up in the query's row (its targets ascend: a binary search) and, where t is listed, adds cq * ct to the
// hit's dot and min(cq, ct) to its min_sum.  Integer adds commute, so the order the lanes arrive in does not show.  An add to dot that
// wraps (old + x < old) happens iff the true sum reaches 2^64: it sets the hit's sticky bit, and the hit's dot becomes 2^64 - 1.
struct SwRow {
    const u32 *tg;  // the row's targets, ascending
    u64 *d, *m;     // its dot and min_sum
    u32 *f;         // sticky saturation bits: bit (f0 + j) & 31 of word (f0 + j) >> 5 for hit j of the row
    u64 f0;
    u32 h;          // hits of the row
    __device__ __forceinline__ void add(u32 t, u32 cq, u32 ct) const {
        u32 lo = 0, hi = h;
        while (lo < hi) {
            const u32 mid = (lo + hi) >> 1;
            if (tg[mid] < t) lo = mid + 1;
            else hi = mid;
        }
        if (lo < h && tg[lo] == t) {
            const u64 x = (u64)cq * ct;
            const u64 old = atomicAdd((unsigned long long *)&d[lo], (unsigned long long)x);
            if (old + x < old) atomicOr(&f[(f0 + lo) >> 5], 1u << ((f0 + lo) & 31));
            atomicAdd((unsigned long long *)&m[lo], (unsigned long long)(cq < ct ? cq : ct));
        }
    }
};
// the postings of query values [a, e) against `row`, 64 values a trip: a lane walks its value's list, lists longer than 64 are walked by the
// whole wavefront (as k_lg_emit copies them).  qcnt / post_cnt == NULL: an uncounted operand, every count 1.
__device__ __forceinline__ void sw_walk(const u64 *rng, const u32 *qcnt, u64 a, u64 e, int lane, const u32 *post_tgt, const u32 *post_cnt, const SwRow &row) {
    for (u64 i0 = a; i0 < e; i0 += 64) {
        const u64 i = i0 + lane;
        const u64 r = i < e ? rng[i] : 0;
        const u32 len = (u32)r, s = (u32)(r >> 32);
        const u32 cq = (qcnt && i < e) ? qcnt[i] : 1u;
        if (len <= 64)
            for (u32 t = 0; t < len; ++t) row.add(post_tgt[s + t], cq, post_cnt ? post_cnt[s + t] : 1u);
        u64 big = __ballot(len > 64);
        while (big) {
            const int src = __builtin_ctzll(big);
            big &= big - 1;
            const u32 s2 = (u32)__builtin_amdgcn_readlane((int)s, src), len2 = (u32)__builtin_amdgcn_readlane((int)len, src),
                      cq2 = (u32)__builtin_amdgcn_readlane((int)cq, src);
            for (u32 t = lane; t < len2; t += 64) row.add(post_tgt[s2 + t], cq2, post_cnt ? post_cnt[s2 + t] : 1u);
        }
    }
}
// which kernel a query with hits takes: k_sw_row when it was on the search's small path and its row fits the LDS row, else k_sw_chunk
__device__ __forceinline__ bool sw_in_lds(u64 qsum, u64 h) { return qsum <= SR_CAP && h <= SW_ROW; }
struct SwRowsOf {  // 1 for a query of k_sw_row
    const u64 *qsum, *hoff;
    __device__ __forceinline__ u64 operator()(u64 q) const {
        const u64 h = hoff[q + 1] - hoff[q];
        return h && sw_in_lds(qsum[q], h) ? 1 : 0;
    }
};
struct SwChunksOf {  // the chunks of SW_CHUNK values a query of k_sw_chunk is cut into
    const u64 *qsum, *hoff, *qoff;
    __device__ __forceinline__ u64 operator()(u64 q) const {
        const u64 h = hoff[q + 1] - hoff[q];
        return h && !sw_in_lds(qsum[q], h) ? (qoff[q + 1] - qoff[q] + SW_CHUNK - 1) / SW_CHUNK : 0;
    }
};
// one wavefront per query: the row's targets and zeroed accumulators in LDS, the walk, one coalesced write of the finished row
__global__ __launch_bounds__(64 * SW_WAVES) void k_sw_row(const u64 *qoff, const u64 *rng, const u64 *qsum, u64 nq, const u32 *qcnt, const u32 *post_tgt,
                                                          const u32 *post_cnt, const u64 *hoff, const u32 *htgt, u64 *dot, u64 *msum) {
    __shared__ u64 s_d[SW_WAVES][SW_ROW], s_m[SW_WAVES][SW_ROW];
    __shared__ u32 s_t[SW_WAVES][SW_ROW], s_f[SW_WAVES][SW_ROW / 32];
    static_assert(SW_ROW % 32 == 0 && SW_ROW / 32 <= 64 && SW_ROW <= SR_CAP, "a lane per word of saturation bits; a small-path row has at most SR_CAP hits");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 q = wave; q < nq; q += nw) {
        const u64 h0 = hoff[q], h64 = hoff[q + 1] - h0;
        if (h64 == 0 || !sw_in_lds(qsum[q], h64)) continue;  // (the same for every lane)
        const u32 h = (u32)h64;  // <= SW_ROW
        for (u32 j = lane; j < h; j += 64) {
            s_t[w][j] = htgt[h0 + j];
            s_d[w][j] = 0;
            s_m[w][j] = 0;
        }
        if (lane < SW_ROW / 32) s_f[w][lane] = 0;
        wave_sync_lds();
        sw_walk(rng, qcnt, qoff[q], qoff[q + 1], lane, post_tgt, post_cnt, SwRow{s_t[w], s_d[w], s_m[w], s_f[w], 0, h});
        wave_sync_lds();
        for (u32 j = lane; j < h; j += 64) {
            dot[h0 + j] = ((s_f[w][j >> 5] >> (j & 31)) & 1u) ? ~0ULL : s_d[w][j];
            msum[h0 + j] = s_m[w][j];
        }
        wave_sync_lds();  // every lane is done with the row before the next query fills it
    }
}
// one wavefront per chunk of SW_CHUNK values of a query: its query by a binary search over the chunk offsets (coff[q] <= c < coff[q + 1]; a
// query without chunks has coff[q] == coff[q + 1] and is never found), the adds as 64-bit atomics into the zeroed global row
__global__ __launch_bounds__(256) void k_sw_chunk(const u64 *qoff, const u64 *rng, const u64 *coff, u64 nq, u64 nc, const u32 *qcnt, const u32 *post_tgt,
                                                  const u32 *post_cnt, const u64 *hoff, const u32 *htgt, u64 *dot, u64 *msum, u32 *flags) {
    const int lane = threadIdx.x & 63;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 c = wave; c < nc; c += nw) {
        u64 lo = 0, hi = nq;  // nc != 0: nq != 0.  The last query whose first chunk is <= c
        while (hi - lo > 1) {
            const u64 mid = (lo + hi) >> 1;
            if (coff[mid] <= c) lo = mid;
            else hi = mid;
        }
        const u64 a = qoff[lo] + (c - coff[lo]) * SW_CHUNK, end = qoff[lo + 1], e = a + SW_CHUNK < end ? a + SW_CHUNK : end;
        const u64 h0 = hoff[lo];
        sw_walk(rng, qcnt, a, e, lane, post_tgt, post_cnt, SwRow{htgt + h0, dot + h0, msum + h0, flags, h0, (u32)(hoff[lo + 1] - h0)});
    }
}
// dot = min(true sum, 2^64 - 1): the hits whose sticky bit is set
__global__ __launch_bounds__(256) void k_sw_finish(const u32 *flags, u64 H, u64 *dot) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < H; i += (u64)gridDim.x * blockDim.x)
        if ((flags[i >> 5] >> (i & 31)) & 1u) dot[i] = ~0ULL;
}

// ---- the n best hits of every query (bsk_hits_top) ----
// A hit's rank is the key (shared << 32) | ~target: larger is better, and the keys of one query are distinct (its targets are).
#define TOP_GROUP 16       // hits a group of 16 lanes ranks in registers, one per lane
#define TOP_SELECT_N 16    // the largest n taken by n rounds of a wave-wide maximum (any number of hits)
#define TOP_LDS_KEYS 1024  // keys one wavefront sorts in LDS: 8 KB, the budget of k_sr_small (SR_CAP u32 there, u64 keys here)
#define TOP_WAVES 4        // wavefronts per workgroup of k_top_select / k_top_lds
__device__ __forceinline__ u64 top_key(u32 s, u32 t) { return ((u64)s << 32) | (u32)~t; }
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
    for (int d = 32; d; d >>= 1) {
        const u64 t = __shfl_xor(v, d, 64);
        v = t > v ? t : v;
    }
    return v;
}
struct TopCnt {  // what a query keeps: min(n, its hits)
    const u64 *off;
    u64 n;
    __device__ __forceinline__ u64 operator()(u64 q) const {
        const u64 c = off[q + 1] - off[q];
        return c < n ? c : n;
    }
};
struct TopLargeOf {  // queries beyond one wavefront's LDS: their count (count_only) or their hits
    const u64 *off;
    bool count_only;
    __device__ __forceinline__ u64 operator()(u64 q) const {
        const u64 c = off[q + 1] - off[q];
        return c > TOP_LDS_KEYS ? (count_only ? 1 : c) : 0;
    }
};
// cnt[0] = queries of 1 .. TOP_GROUP hits, cnt[1] = queries of TOP_GROUP + 1 .. wave_hi hits
__global__ __launch_bounds__(256) void k_top_classes(const u64 *off, u64 nq, u64 wave_hi, u64 *cnt) {
    u32 g = 0, w = 0;
    for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (u64)gridDim.x * blockDim.x) {
        const u64 c = off[q + 1] - off[q];
        g += c >= 1 && c <= TOP_GROUP;
        w += c > TOP_GROUP && c <= wave_hi;
    }
    for (int d = 32; d; d >>= 1) {
        g += __shfl_xor(g, d, 64);
        w += __shfl_xor(w, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (g) atomicAdd((unsigned long long *)cnt, (unsigned long long)g);
        if (w) atomicAdd((unsigned long long *)cnt + 1, (unsigned long long)w);
    }
}
__global__ __launch_bounds__(256) void k_top_maxshared(const u32 *sh, u64 n, u64 *mx) {
    u32 m = 0;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) m = sh[i] > m ? sh[i] : m;
    m = wave_max_u32(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax((unsigned long long *)mx, (unsigned long long)m);
}
// queries of at most TOP_GROUP hits, a group of 16 lanes each: a lane's hit goes to the place (number of better keys of the group)
__global__ __launch_bounds__(256) void k_top_group(const u64 *off, const u32 *tgt, const u32 *sh, u64 nq, u32 n, const u64 *toff, u32 *otgt, u32 *osh) {
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((u64)gridDim.x * blockDim.x) >> 6;
    const u32 l = threadIdx.x & 15, g = (threadIdx.x & 63) >> 4;
    for (u64 q0 = wave * 4; q0 < nq; q0 += nw * 4) {  // (the whole wavefront stays in step: the shuffles read every lane)
        const u64 q = q0 + g;
        u64 a = 0, c = 0;
        if (q < nq) {
            a = off[q];
            c = off[q + 1] - a;
        }
        const bool mine = c <= TOP_GROUP && l < c;
        u32 t = 0, s = 0;
        if (mine) {
            t = tgt[a + l];
            s = sh[a + l];
        }
        const u64 key = mine ? top_key(s, t) : 0;  // (a listed pair shares a value: its key is not 0)
        u32 rank = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) rank += __shfl(key, j, 16) > key;
        if (mine && rank < n) {
            const u64 o = toff[q] + rank;
            otgt[o] = t;
            osh[o] = s;
        }
    }
}
// queries of more than TOP_GROUP hits and n <= TOP_SELECT_N: round r takes the largest key below round r - 1's.  A wavefront looks at
// qb (a power of two <= 64) consecutive queries at a time, one per lane, and then serves those that are its kind one after the other.
__global__ __launch_bounds__(64 * TOP_WAVES) void k_top_select(const u64 *off, const u32 *tgt, const u32 *sh, u64 nq, u32 n, u32 qb, const u64 *toff, u32 *otgt,
                                                               u32 *osh) {
    const u32 lane = threadIdx.x & 63;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 q0 = wave * qb; q0 < nq; q0 += nw * qb) {
        const u64 ql = q0 + lane;
        const u64 cl = lane < qb && ql < nq ? off[ql + 1] - off[ql] : 0;
        u64 todo = __ballot(cl > TOP_GROUP);
        while (todo) {
            const u64 q = q0 + (u64)__builtin_ctzll(todo);
            todo &= todo - 1;
            const u64 a = off[q], c = off[q + 1] - a, o = toff[q];
            const u32 keep = c < n ? (u32)c : n;
            const bool one = c <= 64;  // a key per lane: read once
            const u64 held = one && lane < c ? top_key(sh[a + lane], tgt[a + lane]) : 0;
            u64 prev = 0;
            for (u32 r = 0; r < keep; ++r) {
                u64 best = 0;
                if (one) {
                    best = (r == 0 || held < prev) ? held : 0;
                } else {
                    for (u64 i = lane; i < c; i += 64) {
                        const u64 k = top_key(sh[a + i], tgt[a + i]);
                        if ((r == 0 || k < prev) && k > best) best = k;
                    }
                }
                best = wave_max_u64(best);
                prev = best;
                if (lane == 0) {
                    otgt[o + r] = ~(u32)best;
                    osh[o + r] = (u32)(best >> 32);
                }
            }
        }
    }
}
// queries of TOP_GROUP + 1 .. TOP_LDS_KEYS hits and n > TOP_SELECT_N: the inverted keys (~shared << 32) | target sorted ascending in
// LDS (bitonic, as k_sr_small sorts its target ids), the first min(n, hits) written out
__global__ __launch_bounds__(64 * TOP_WAVES) void k_top_lds(const u64 *off, const u32 *tgt, const u32 *sh, u64 nq, u32 n, u32 qb, const u64 *toff, u32 *otgt,
                                                            u32 *osh) {
    __shared__ u64 lds[TOP_WAVES][TOP_LDS_KEYS];
    u64 *buf = lds[threadIdx.x >> 6];
    const u32 lane = threadIdx.x & 63;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 q0 = wave * qb; q0 < nq; q0 += nw * qb) {
        const u64 ql = q0 + lane;
        const u64 cl = lane < qb && ql < nq ? off[ql + 1] - off[ql] : 0;
        u64 todo = __ballot(cl > TOP_GROUP && cl <= TOP_LDS_KEYS);
        while (todo) {
            const u64 q = q0 + (u64)__builtin_ctzll(todo);
            todo &= todo - 1;
            const u64 a = off[q], o = toff[q];
            const u32 c = (u32)(off[q + 1] - a);  // TOP_GROUP < c <= TOP_LDS_KEYS
            const u32 keep = c < n ? c : n;
            const u32 c2 = 1u << (32 - __builtin_clz(c - 1));  // <= TOP_LDS_KEYS (a power of two)
            for (u32 i = lane; i < c2; i += 64) buf[i] = i < c ? ~top_key(sh[a + i], tgt[a + i]) : ~0ULL;  // (no inverted key is ~0: shared >= 1)
            wave_sync_lds();
            for (u32 k = 2; k <= c2; k <<= 1) {
                for (u32 j = k >> 1; j > 0; j >>= 1) {
                    for (u32 i = lane; i < c2; i += 64) {
                        const u32 p = i ^ j;
                        if (p > i) {
                            const u64 x = buf[i], y = buf[p];
                            if ((x > y) == ((i & k) == 0)) {
                                buf[i] = y;
                                buf[p] = x;
                            }
                        }
                    }
                    wave_sync_lds();
                }
            }
            for (u32 i = lane; i < keep; i += 64) {
                const u64 k = buf[i];
                otgt[o + i] = (u32)k;
                osh[o + i] = ~(u32)(k >> 32);
            }
            wave_sync_lds();  // every lane is done with the buffer before the next query fills it
        }
    }
}
// queries of more than TOP_LDS_KEYS hits and n > TOP_SELECT_N: slot s = the s-th of them; hit p of the query (its targets ascend with
// p) gets the key (slot << (bs + bp)) | ((max_shared - shared) << bp) | p, so one ascending sort of all keys leaves every slot's hits
// where the emit put them, best first
__global__ __launch_bounds__(256) void k_top_list(const u64 *off, u64 nq, const u64 *lslot, u32 *lq) {
    for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (u64)gridDim.x * blockDim.x)
        if (off[q + 1] - off[q] > TOP_LDS_KEYS) lq[lslot[q]] = (u32)q;
}
__global__ __launch_bounds__(256) void k_top_emit(const u64 *off, const u32 *sh, const u32 *lq, u64 nl, const u64 *loff, u64 max_shared, u32 bs, u32 bp, u64 *lkeys) {
    const u32 lane = threadIdx.x & 63;
    const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 slot = wave; slot < nl; slot += nw) {
        const u32 q = lq[slot];
        const u64 a = off[q], c = off[q + 1] - a, d = loff[q], hi = slot << (bs + bp);
        for (u64 p = lane; p < c; p += 64) lkeys[d + p] = hi | ((max_shared - sh[a + p]) << bp) | p;
    }
}
__global__ __launch_bounds__(256) void k_top_place(const u64 *lkeys, u64 L, const u64 *off, const u32 *tgt, const u32 *lq, const u64 *loff, u64 max_shared, u32 bs,
                                                   u32 bp, u32 n, const u64 *toff, u32 *otgt, u32 *osh) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < L; i += (u64)gridDim.x * blockDim.x) {
        const u64 k = lkeys[i];
        const u32 q = lq[k >> (bs + bp)];
        const u64 r = i - loff[q];  // the slot's hits lie at [loff[q], ...), as emitted
        if (r < n) {
            const u64 o = toff[q] + r;
            otgt[o] = tgt[off[q] + (k & ((1ULL << bp) - 1))];
            osh[o] = (u32)(max_shared - ((k >> bp) & ((1ULL << bs) - 1)));
        }
    }
}
__global__ __launch_bounds__(256) void k_off_u32(const u64 *in, u64 n, u32 *out) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) out[i] = (u32)in[i];
}

// device temporaries of one call, freed on every way out
struct Temps {
    std::vector<void *> p;
    ~Temps() {
        for (void *x : p) (void)hipFree(x);
    }
    hipError_t get(void **out, size_t bytes) {
        *out = nullptr;
        const hipError_t e = hipMalloc(out, bytes ? bytes : 8);
        if (e == hipSuccess) p.push_back(*out);
        return e;
    }
};
}  // namespace

extern "C" int bsk_sets_from_host(bsk_ctx *ctx, const uint64_t *offsets, uint64_t n_sets, const uint64_t *values, bsk_sets **out) {
    if (out) *out = nullptr;
    if (!ctx || !offsets || !out) return fail_arg(ctx, "bsk_sets_from_host: null argument");
    if (offsets[0] != 0) return fail_arg(ctx, "bsk_sets_from_host: offsets[0] != 0");
    if (offsets[n_sets] && !values) return fail_arg(ctx, "bsk_sets_from_host: null values");
    for (u64 s = 0; s < n_sets; ++s)  // (first: then every offset is <= offsets[n_sets], the number of values)
        if (offsets[s + 1] < offsets[s]) return fail_arg(ctx, "bsk_sets_from_host: offsets decrease");
    for (u64 s = 0; s < n_sets; ++s)
        for (u64 i = offsets[s] + 1; i < offsets[s + 1]; ++i)
            if (values[i] <= values[i - 1]) return fail_arg(ctx, "bsk_sets_from_host: values not strictly ascending inside a set");
    const u64 N = offsets[n_sets];
    HIPCHK(ctx, hipSetDevice(ctx->device));
    bsk_sets *s = new (std::nothrow) bsk_sets();
    if (!s) return BSK_ERR_NOMEM;
    s->ctx = ctx;
    s->n_sets = n_sets;
    s->n_values = N;
    hipError_t e = hipMalloc(&s->offsets, (n_sets + 1) * 8);
    if (e == hipSuccess) {
        s->c_offsets = (n_sets + 1) * 8;
        e = hipMalloc(&s->values, (N ? N : 1) * 8);
    }
    if (e == hipSuccess) {
        s->c_values = (N ? N : 1) * 8;
        e = hipMemcpyAsync(s->offsets, offsets, (n_sets + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
    }
    if (e == hipSuccess && N) e = hipMemcpyAsync(s->values, values, N * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // (the caller's buffers are not retained)
    if (e != hipSuccess) {
        bsk_sets_release(s);
        return fail_hip(ctx, e, "bsk_sets_from_host");
    }
    *out = s;
    return BSK_OK;
}

extern "C" void bsk_index_release(bsk_index *ix) {
    if (!ix) return;
    IndexArrays *a = ix->a;
    if (a && a->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) {  // the last handle of this device's arrays
        (void)hipSetDevice(a->device);
        (void)hipFree(a->keys);
        (void)hipFree(a->post_off);
        (void)hipFree(a->post_tgt);
        (void)hipFree(a->dir);
        (void)hipFree(a->tsize);
        (void)hipFree(a->post_cnt);
        (void)hipFree(a->tsumsq);
        (void)hipFree(a->ttotal);
        delete a;
    }
    delete ix;
}

extern "C" int bsk_index_attach(bsk_ctx *ctx, const bsk_index *ix, bsk_index **handle) {
    if (handle) *handle = nullptr;
    if (!ctx || !ix || !handle) return fail_arg(ctx, "bsk_index_attach: null argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    bsk_index *h = new (std::nothrow) bsk_index(*ix);
    if (!h) return BSK_ERR_NOMEM;
    h->ctx = ctx;
    const IndexArrays *src = ix->a;
    if (src->device == ctx->device) {  // same device: the arrays are shared
        ix->a->refs.fetch_add(1, std::memory_order_relaxed);
        *handle = h;
        return BSK_OK;
    }
    h->a = new (std::nothrow) IndexArrays();  // another device: one copy of the arrays, owned by this handle (and those attached from it)
    if (!h->a) {
        delete h;
        return BSK_ERR_NOMEM;
    }
    std::unique_ptr<bsk_index, void (*)(bsk_index *)> hold(h, bsk_index_release);
    IndexArrays *d = h->a;
    d->device = ctx->device;
    const u64 U = ix->n_distinct, P = ix->n_postings, T = ix->n_targets, nb = 1ULL << ix->bits;
    const size_t b_keys = (U ? U : 1) * 8, b_off = (U + 1) * 4, b_tgt = (P ? P : 1) * 4, b_dir = (nb + 1) * 4, b_ts = (T ? T : 1) * 4;
    HIPCHK(ctx, hipMalloc(&d->keys, b_keys));
    HIPCHK(ctx, hipMalloc(&d->post_off, b_off));
    HIPCHK(ctx, hipMalloc(&d->post_tgt, b_tgt));
    HIPCHK(ctx, hipMalloc(&d->dir, b_dir));
    HIPCHK(ctx, hipMalloc(&d->tsize, b_ts));
    // (the source arrays were complete when their build returned; the copies are complete when this returns)
    HIPCHK(ctx, hipMemcpyPeer(d->keys, d->device, src->keys, src->device, b_keys));
    HIPCHK(ctx, hipMemcpyPeer(d->post_off, d->device, src->post_off, src->device, b_off));
    HIPCHK(ctx, hipMemcpyPeer(d->post_tgt, d->device, src->post_tgt, src->device, b_tgt));
    HIPCHK(ctx, hipMemcpyPeer(d->dir, d->device, src->dir, src->device, b_dir));
    HIPCHK(ctx, hipMemcpyPeer(d->tsize, d->device, src->tsize, src->device, b_ts));
    if (ix->counted) {  // a counted index: its counts and norms go along
        const size_t b_norm = (T ? T : 1) * 8;
        HIPCHK(ctx, hipMalloc(&d->post_cnt, b_tgt));
        HIPCHK(ctx, hipMalloc(&d->tsumsq, b_norm));
        HIPCHK(ctx, hipMalloc(&d->ttotal, b_norm));
        HIPCHK(ctx, hipMemcpyPeer(d->post_cnt, d->device, src->post_cnt, src->device, b_tgt));
        HIPCHK(ctx, hipMemcpyPeer(d->tsumsq, d->device, src->tsumsq, src->device, b_norm));
        HIPCHK(ctx, hipMemcpyPeer(d->ttotal, d->device, src->ttotal, src->device, b_norm));
    }
    HIPCHK(ctx, hipDeviceSynchronize());
    *handle = hold.release();
    return BSK_OK;
}

// bsk_index_build (keep_counts == false) and bsk_index_build_counted: the same checks, limits and slot rule under the entry's own name; with
// counts the sort carries the posting number instead of the target and k_ix_gather fills post_tgt and post_cnt from the permutation
static int index_build(bsk_ctx *ctx, const bsk_sets *targets, bsk_index **out, bool keep_counts) {
    if (out) *out = nullptr;
    if (!ctx || !targets || !out) return fail_arg(ctx, keep_counts ? "bsk_index_build_counted: null argument" : "bsk_index_build: null argument");
    if (targets->ctx != ctx)
        return fail_arg(ctx, keep_counts ? "bsk_index_build_counted: the sets belong to another context" : "bsk_index_build: the sets belong to another context");
    const u64 T = targets->n_sets, P = targets->n_values;
    if (T >= (1ULL << 32) || P >= (1ULL << 32)) {
        ctx->err = keep_counts ? "bsk_index_build_counted: 2^32 targets or postings or more" : "bsk_index_build: 2^32 targets or postings or more";
        return BSK_ERR_UNSUPPORTED;
    }
    const bool counted = keep_counts && targets->counted;  // uncounted sets: an index without counts, whichever entry built it
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    bsk_index *ix = new (std::nothrow) bsk_index();
    if (!ix) return BSK_ERR_NOMEM;
    std::unique_ptr<bsk_index, void (*)(bsk_index *)> hold(ix, bsk_index_release);
    ix->ctx = ctx;
    ix->a = new (std::nothrow) IndexArrays();
    if (!ix->a) return BSK_ERR_NOMEM;
    ix->a->device = ctx->device;
    ix->n_targets = T;
    ix->n_postings = P;
    Temps tmp;
    u64 *kin = nullptr, *kout = nullptr, *pos = nullptr, *part = nullptr, *tot = nullptr;
    u32 *tin = nullptr, *flag = nullptr, *ord = nullptr, *perm = nullptr;
    HIPCHK(ctx, hipMalloc(&ix->a->post_tgt, (P ? P : 1) * 4));
    HIPCHK(ctx, hipMalloc(&ix->a->tsize, (T ? T : 1) * 4));
    if (counted) {
        ix->counted = true;
        HIPCHK(ctx, hipMalloc(&ix->a->post_cnt, (P ? P : 1) * 4));
        HIPCHK(ctx, hipMalloc(&ix->a->tsumsq, (T ? T : 1) * 8));
        HIPCHK(ctx, hipMalloc(&ix->a->ttotal, (T ? T : 1) * 8));
        if (T) {  // the norms, as bsk_sets_sumsq and bsk_sets_totals give them (on the stream; the read-backs below wait for them)
            int rc = sets_sumsq_device(ctx, targets, 0, T, ix->a->tsumsq);
            if (rc == BSK_OK) rc = sets_totals_device(ctx, targets, 0, T, ix->a->ttotal);
            if (rc != BSK_OK) return rc;
        }
    }
    HIPCHK(ctx, tmp.get((void **)&tot, 64));
    HIPCHK(ctx, hipMemsetAsync(tot, 0, 64, st));
    if (T) {
        hipLaunchKernelGGL(k_ix_sizes, dim3(grid_for(ctx, T, 256, 8)), dim3(256), 0, st, targets->offsets, T, ix->a->tsize);
        HIPCHK(ctx, hipGetLastError());
    }
    u64 U = 0;
    if (P) {
        HIPCHK(ctx, tmp.get((void **)&kin, (P + 1) * 8));
        HIPCHK(ctx, tmp.get((void **)&kout, P * 8));
        HIPCHK(ctx, tmp.get((void **)&tin, P * 4));
        hipLaunchKernelGGL(k_ix_pairs, dim3(grid_for(ctx, P, 256, 16)), dim3(256), 0, st, targets->offsets, targets->values, T, P, kin, tin);
        HIPCHK(ctx, hipGetLastError());
        if (counted) {
            HIPCHK(ctx, tmp.get((void **)&ord, P * 4));
            HIPCHK(ctx, tmp.get((void **)&perm, P * 4));
            hipLaunchKernelGGL(k_ix_ord, dim3(grid_for(ctx, P, 256, 16)), dim3(256), 0, st, P, ord);
            HIPCHK(ctx, hipGetLastError());
        }
        u32 *vin = counted ? ord : tin, *vout = counted ? perm : ix->a->post_tgt;
        size_t tb = 0;
        HIPCHK(ctx, rocprim::radix_sort_pairs(nullptr, tb, kin, kout, vin, vout, (size_t)P, 0, 64, st));
        void *stmp = nullptr;
        HIPCHK(ctx, tmp.get(&stmp, tb));
        HIPCHK(ctx, rocprim::radix_sort_pairs(stmp, tb, kin, kout, vin, vout, (size_t)P, 0, 64, st));
        if (counted) {
            hipLaunchKernelGGL(k_ix_gather, dim3(grid_for(ctx, P, 256, 16)), dim3(256), 0, st, perm, tin, targets->counts, P, ix->a->post_tgt, ix->a->post_cnt);
            HIPCHK(ctx, hipGetLastError());
        }
        flag = tin;  // (both free after the sort)
        pos = kin;
        HIPCHK(ctx, tmp.get((void **)&part, (scan_parts(P)) * 8));
        hipLaunchKernelGGL(k_run_heads, dim3(grid_for(ctx, P, 256, 16)), dim3(256), 0, st, kout, P, flag);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, scan_counts(st, KeepOf{flag}, P, part, pos, tot, (u64 *)nullptr));
        HIPCHK(ctx, read_back(ctx, tot, 1));
        U = ctx->h_pinned[0];
    }
    int bits = 0;
    while (bits < 62 && (2ULL << bits) <= U) ++bits;  // 2^bits <= U < 2^(bits + 1): one or two keys per bucket
    const u64 nb = 1ULL << bits;
    ix->bits = bits;
    ix->n_distinct = U;
    HIPCHK(ctx, hipMalloc(&ix->a->keys, (U ? U : 1) * 8));
    HIPCHK(ctx, hipMalloc(&ix->a->post_off, (U + 1) * 4));
    HIPCHK(ctx, hipMalloc(&ix->a->dir, (nb + 1) * 4));
    if (P) {
        hipLaunchKernelGGL(k_ix_scatter, dim3(grid_for(ctx, P, 256, 16)), dim3(256), 0, st, kout, flag, pos, P, ix->a->keys, ix->a->post_off);
        HIPCHK(ctx, hipGetLastError());
    } else {
        HIPCHK(ctx, hipMemsetAsync(ix->a->post_off, 0, 4, st));
    }
    hipLaunchKernelGGL(k_ix_dir, dim3(grid_for(ctx, U + 1, 256, 16)), dim3(256), 0, st, ix->a->keys, U, bits, ix->a->dir);
    hipLaunchKernelGGL(k_ix_maxb, dim3(grid_for(ctx, nb, 256, 8)), dim3(256), 0, st, ix->a->dir, nb, tot + 1);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, read_back(ctx, tot + 1, 1, 1));
    ix->max_bucket = ctx->h_pinned[1];
    ix->device_bytes = (U ? U : 1) * 8 + (U + 1) * 4 + (P ? P : 1) * 4 + (nb + 1) * 4 + (T ? T : 1) * 4;
    if (counted) ix->device_bytes += (P ? P : 1) * 4 + 2 * (T ? T : 1) * 8;
    *out = hold.release();
    return BSK_OK;
}

extern "C" int bsk_index_build(bsk_ctx *ctx, const bsk_sets *targets, bsk_index **out) { return index_build(ctx, targets, out, false); }
extern "C" int bsk_index_build_counted(bsk_ctx *ctx, const bsk_sets *targets, bsk_index **out) { return index_build(ctx, targets, out, true); }

extern "C" int bsk_index_counted(const bsk_index *ix, int *counted) {
    if (!ix || !counted) return BSK_ERR_ARG;
    *counted = ix->counted ? 1 : 0;
    return BSK_OK;
}

// the norms of targets first .. first + count - 1: the arrays a counted index keeps, |t| for an index without counts
extern "C" int bsk_index_fetch_norms(bsk_ctx *ctx, const bsk_index *ix, uint64_t first, uint64_t count, uint64_t *sumsq, uint64_t *totals) {
    if (!ctx || !ix) return fail_arg(ctx, "bsk_index_fetch_norms: null argument");
    if (ix->ctx != ctx) return fail_arg(ctx, "bsk_index_fetch_norms: the index belongs to another context");
    if (first > ix->n_targets || count > ix->n_targets - first) return fail_arg(ctx, "bsk_index_fetch_norms: range outside the targets");
    if (count == 0 || (!sumsq && !totals)) return BSK_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ix->counted) {
        if (sumsq) HIPCHK(ctx, hipMemcpyAsync(sumsq, ix->a->tsumsq + first, count * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (totals) HIPCHK(ctx, hipMemcpyAsync(totals, ix->a->ttotal + first, count * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return BSK_OK;
    }
    std::vector<u32> sz(count);
    HIPCHK(ctx, hipMemcpyAsync(sz.data(), ix->a->tsize + first, count * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (u64 t = 0; t < count; ++t) {
        if (sumsq) sumsq[t] = sz[t];
        if (totals) totals[t] = sz[t];
    }
    return BSK_OK;
}

extern "C" int bsk_index_info(const bsk_index *ix, uint64_t *n_targets, uint64_t *n_postings, uint64_t *n_distinct, uint64_t *max_bucket,
                              uint64_t *device_bytes) {
    if (!ix) return BSK_ERR_ARG;
    if (n_targets) *n_targets = ix->n_targets;
    if (n_postings) *n_postings = ix->n_postings;
    if (n_distinct) *n_distinct = ix->n_distinct;
    if (max_bucket) *max_bucket = ix->max_bucket;
    if (device_bytes) *device_bytes = ix->device_bytes;
    return BSK_OK;
}

extern "C" void bsk_hits_release(bsk_hits *h) {
    if (!h) return;
    if (h->ctx) (void)hipSetDevice(h->ctx->device);
    (void)hipFree(h->offsets);
    (void)hipFree(h->target);
    (void)hipFree(h->shared);
    (void)hipFree(h->total);
    (void)hipFree(h->dot);
    (void)hipFree(h->msum);
    (void)hipFree(h->members);
    delete h;
}

// Hits from the host (the counterpart of bsk_sets_from_host): edges computed elsewhere, or a graph a test states directly.  The CSR is
// checked on the host before the slot is taken over; the caller's buffers are not retained.
extern "C" int bsk_hits_from_host(bsk_ctx *ctx, const uint64_t *offsets, uint64_t n_queries, const uint32_t *target, const uint32_t *shared, const uint32_t *total,
                                  bsk_hits **hits) {
    if (!ctx || !offsets || !hits) return fail_arg(ctx, "bsk_hits_from_host: null argument");
    if (*hits && (*hits)->ctx != ctx) return fail_arg(ctx, "bsk_hits_from_host: the hits belong to another context");
    if (offsets[0] != 0) return fail_arg(ctx, "bsk_hits_from_host: offsets[0] != 0");
    for (u64 q = 0; q < n_queries; ++q)  // (first: then every offset is <= offsets[n_queries], the number of hits)
        if (offsets[q + 1] < offsets[q]) return fail_arg(ctx, "bsk_hits_from_host: offsets decrease");
    const u64 H = offsets[n_queries];
    if (H && (!target || !shared)) return fail_arg(ctx, "bsk_hits_from_host: null target or shared");
    for (u64 q = 0; q < n_queries; ++q)
        for (u64 i = offsets[q] + 1; i < offsets[q + 1]; ++i)
            if (target[i] <= target[i - 1]) return fail_arg(ctx, "bsk_hits_from_host: targets not strictly ascending inside a row");
    return take_over(ctx, hits, bsk_hits_release, [&](bsk_hits *res, bool) -> int {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        res->n_queries = n_queries;
        res->n_hits = 0;
        res->n_large = 0;
        res->has_total = false;
        res->has_weights = false;
        res->has_members = false;
        HIPCHK(ctx, grow_array(&res->offsets, &res->c_offsets, (n_queries + 1) * 8));
        HIPCHK(ctx, grow_array(&res->target, &res->c_target, (H ? H : 1) * 4));
        HIPCHK(ctx, grow_array(&res->shared, &res->c_shared, (H ? H : 1) * 4));
        if (total) HIPCHK(ctx, grow_array(&res->total, &res->c_total, (H ? H : 1) * 4));
        HIPCHK(ctx, hipMemcpyAsync(res->offsets, offsets, (n_queries + 1) * 8, hipMemcpyHostToDevice, st));
        if (H) {
            HIPCHK(ctx, hipMemcpyAsync(res->target, target, H * 4, hipMemcpyHostToDevice, st));
            HIPCHK(ctx, hipMemcpyAsync(res->shared, shared, H * 4, hipMemcpyHostToDevice, st));
            if (total) HIPCHK(ctx, hipMemcpyAsync(res->total, total, H * 4, hipMemcpyHostToDevice, st));
        }
        HIPCHK(ctx, hipStreamSynchronize(st));  // (the caller's buffers are not retained)
        res->n_hits = H;
        res->has_total = total != nullptr;
        snprintf(res->plan, sizeof res->plan, "from host");
        return BSK_OK;
    });
}

static int search_impl(bsk_ctx *ctx, const bsk_index *ix, const bsk_sets *qs, const bsk_search_params *sp, bsk_hits *res);
static int weights_impl(bsk_ctx *ctx, const bsk_index *ix, const bsk_sets *qs, bsk_hits *res);
// bsk_index_search and bsk_index_search_counted: the same checks in the same order, each under the entry's own name, all before the slot is
// taken over; the weighted entry runs the search as it is and then the payload pass over what the search left in the pool
static int search_entry(bsk_ctx *ctx, const bsk_index *ix, const bsk_sets *queries, const bsk_search_params *sp, bsk_hits **hits, bool weighted) {
    if (!ctx || !ix || !queries || !sp || !hits) return fail_arg(ctx, weighted ? "bsk_index_search_counted: null argument" : "bsk_index_search: null argument");
    if (ix->ctx != ctx || queries->ctx != ctx || (*hits && (*hits)->ctx != ctx))
        return fail_arg(ctx, weighted ? "bsk_index_search_counted: the index, the queries or the hits belong to another context"
                                      : "bsk_index_search: the index, the queries or the hits belong to another context");
    if (sp->reserved != 0) return fail_arg(ctx, weighted ? "bsk_index_search_counted: reserved != 0" : "bsk_index_search: reserved != 0");
    if (!(sp->min_query_cov >= 0.0 && sp->min_query_cov <= 1.0) || !(sp->min_target_cov >= 0.0 && sp->min_target_cov <= 1.0))
        return fail_arg(ctx, weighted ? "bsk_index_search_counted: a cover outside 0..1 (or NaN)" : "bsk_index_search: a cover outside 0..1 (or NaN)");
    if (queries->n_sets >= (1ULL << 32) || queries->n_values >= (1ULL << 32)) {
        ctx->err = weighted ? "bsk_index_search_counted: 2^32 query sets or query values or more (split the queries)"
                            : "bsk_index_search: 2^32 query sets or query values or more (split the queries)";
        return BSK_ERR_UNSUPPORTED;
    }
    return take_over(ctx, hits, bsk_hits_release, [&](bsk_hits *res, bool) {
        const int rc = search_impl(ctx, ix, queries, sp, res);
        return rc != BSK_OK || !weighted ? rc : weights_impl(ctx, ix, queries, res);
    });
}
extern "C" int bsk_index_search(bsk_ctx *ctx, const bsk_index *ix, const bsk_sets *queries, const bsk_search_params *sp, bsk_hits **hits) {
    return search_entry(ctx, ix, queries, sp, hits, false);
}
extern "C" int bsk_index_search_counted(bsk_ctx *ctx, const bsk_index *ix, const bsk_sets *queries, const bsk_search_params *sp, bsk_hits **hits) {
    return search_entry(ctx, ix, queries, sp, hits, true);
}

// the per-query arrays of one search, one carved buffer of SLOT_SEARCH_QUERY: search_impl fills them, weights_impl reads qsum again
struct SearchCarve {
    Carve c;
    size_t o_qsum, o_stage, o_hcnt, o_lslot, o_loff, o_part, o_tot, o_lq;
    explicit SearchCarve(u64 nq) {
        o_qsum = c.add<u64>(nq);
        o_stage = c.add<u64>(nq + 1);
        o_hcnt = c.add<u64>(nq);
        o_lslot = c.add<u64>(nq + 1);
        o_loff = c.add<u64>(nq + 1);
        o_part = c.add<u64>(scan_parts(nq));
        o_tot = c.add<u64>(8);
        o_lq = c.add<u32>(nq);
    }
};

static int search_impl(bsk_ctx *ctx, const bsk_index *ix, const bsk_sets *qs, const bsk_search_params *sp, bsk_hits *res) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u64 nq = qs->n_sets, nv = qs->n_values, T = ix->n_targets;
    const Thr thr{sp->min_shared ? sp->min_shared : 1u, sp->min_query_cov, sp->min_target_cov};
    res->n_queries = nq;
    res->n_hits = 0;
    res->n_large = 0;
    res->has_total = false;  // (a search into hits with totals keeps the array, like a counted bsk_sets written by an uncounted entry)
    res->has_weights = false;  // (... and so for the weights)
    res->has_members = false;  // (... and the members of folded hits)
    HIPCHK(ctx, grow_array(&res->offsets, &res->c_offsets, (nq + 1) * 8));
    // per-query arrays (one carved buffer) and the query values' posting ranges
    const SearchCarve cq(nq);
    void *bq = nullptr, *brng = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_SEARCH_QUERY, cq.c.bytes, &bq));
    HIPCHK(ctx, ctx_pool(ctx, SLOT_SEARCH_RANGES, (nv ? nv : 1) * 8, &brng));
    u64 *qsum = at<u64>(bq, cq.o_qsum), *stage_off = at<u64>(bq, cq.o_stage), *hcnt = at<u64>(bq, cq.o_hcnt), *lslot = at<u64>(bq, cq.o_lslot),
        *loff = at<u64>(bq, cq.o_loff), *part = at<u64>(bq, cq.o_part), *tot = at<u64>(bq, cq.o_tot), *rng = static_cast<u64 *>(brng);
    u32 *lq = at<u32>(bq, cq.o_lq);
    HIPCHK(ctx, hipMemsetAsync(tot, 0, 64, st));  // [0] staging, [1] large target ids, [2] large queries, [3] large runs, [4] kept runs, [5] hits
    // A. lookups
    if (nq) {
        hipLaunchKernelGGL(k_sr_lookup, dim3(grid_for(ctx, nq * 16, 256, 32)), dim3(256), 0, st, qs->offsets, qs->values, nq, ix->a->keys, ix->a->post_off, ix->a->dir,
                           ix->bits, rng, qsum);
        HIPCHK(ctx, hipGetLastError());
    }
    // B. staging spans, the large queries' slots and target-id offsets
    HIPCHK(ctx, scan_counts(st, StageOf{qsum, T}, nq, part, stage_off, tot + 0, (u64 *)nullptr));
    HIPCHK(ctx, scan_counts(st, LargeOf{qsum, false}, nq, part, loff, tot + 1, (u64 *)nullptr));
    HIPCHK(ctx, scan_counts(st, LargeOf{qsum, true}, nq, part, lslot, tot + 2, (u64 *)nullptr));
    HIPCHK(ctx, read_back(ctx, tot, 3));
    const u64 S = ctx->h_pinned[0], L = ctx->h_pinned[1], NL = ctx->h_pinned[2];
    void *bst = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_SEARCH_STAGE, (S ? S : 1) * 8, &bst));
    u32 *st_tgt = static_cast<u32 *>(bst), *st_sh = st_tgt + (S ? S : 1);
    // C. queries of at most SR_CAP target ids
    if (nq) {
        hipLaunchKernelGGL(k_sr_small, dim3(grid_for(ctx, nq, SR_WAVES, 40)), dim3(64 * SR_WAVES), 0, st, qs->offsets, rng, qsum, nq, ix->a->post_tgt, ix->a->tsize,
                           stage_off, thr, st_tgt, st_sh, hcnt);
        HIPCHK(ctx, hipGetLastError());
    }
    // the large path
    if (NL) {
        Carve cl;
        const size_t o_in = cl.add<u64>(L + 1), o_out = cl.add<u64>(L), o_rstart = cl.add<u64>(L + 1), o_kpos = cl.add<u64>(L + 1),
                     o_flag = cl.add<u32>(L), o_sfirst = cl.add<u64>(NL), o_part2 = cl.add<u64>(scan_parts(L));
        void *bl = nullptr;
        HIPCHK(ctx, ctx_pool(ctx, SLOT_SEARCH_LARGE, cl.bytes, &bl));
        u64 *lin = at<u64>(bl, o_in), *lout = at<u64>(bl, o_out), *rstart = at<u64>(bl, o_rstart), *kpos = at<u64>(bl, o_kpos), *sfirst = at<u64>(bl, o_sfirst),
            *part2 = at<u64>(bl, o_part2);
        u32 *flag = at<u32>(bl, o_flag);
        hipLaunchKernelGGL(k_sr_list_large, dim3(grid_for(ctx, nq, 256, 8)), dim3(256), 0, st, qsum, nq, lslot, lq);
        hipLaunchKernelGGL(k_lg_emit, dim3(grid_for(ctx, NL, 4, 16)), dim3(256), 0, st, qs->offsets, rng, lq, NL, loff, ix->a->post_tgt, lin);
        HIPCHK(ctx, hipGetLastError());
        const unsigned end_bit = 32 + (NL > 1 ? 64 - __builtin_clzll(NL - 1) : 0);
        size_t tb = 0;
        HIPCHK(ctx, sets_sort_u64(nullptr, tb, lin, lout, (size_t)L, 0, end_bit, st));
        void *stmp = nullptr;
        HIPCHK(ctx, ctx_pool(ctx, SLOT_SEARCH_SORT_TMP, tb ? tb : 8, &stmp));
        HIPCHK(ctx, sets_sort_u64(stmp, tb, lin, lout, (size_t)L, 0, end_bit, st));
        u64 *ridx = lin;  // (free after the sort; L + 1 entries)
        hipLaunchKernelGGL(k_run_heads, dim3(grid_for(ctx, L, 256, 16)), dim3(256), 0, st, lout, L, flag);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, scan_counts(st, KeepOf{flag}, L, part2, ridx, tot + 3, (u64 *)nullptr));
        hipLaunchKernelGGL(k_lg_runs, dim3(grid_for(ctx, L, 256, 16)), dim3(256), 0, st, flag, ridx, L, rstart);
        u32 *keep = flag;  // (free once the runs are known)
        hipLaunchKernelGGL(k_lg_keep, dim3(grid_for(ctx, L, 256, 16)), dim3(256), 0, st, lout, rstart, ridx, L, lq, qs->offsets, ix->a->tsize, thr, keep, sfirst);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, scan_counts(st, KeepOf{keep}, L, part2, kpos, tot + 4, (u64 *)nullptr));
        hipLaunchKernelGGL(k_lg_place, dim3(grid_for(ctx, L, 256, 16)), dim3(256), 0, st, lout, rstart, ridx, L, keep, kpos, sfirst, lq, stage_off, st_tgt, st_sh,
                           hcnt);
        HIPCHK(ctx, hipGetLastError());
    }
    // hit offsets, then the move out of the staging spans
    HIPCHK(ctx, scan_counts(st, ArrayOf{hcnt}, nq, part, res->offsets, tot + 5, (u64 *)nullptr));
    HIPCHK(ctx, read_back(ctx, tot + 5, 1));
    const u64 H = ctx->h_pinned[0];
    HIPCHK(ctx, grow_array(&res->target, &res->c_target, (H ? H : 1) * 4));
    HIPCHK(ctx, grow_array(&res->shared, &res->c_shared, (H ? H : 1) * 4));
    if (H) {
        hipLaunchKernelGGL(k_sr_move, dim3(grid_for(ctx, nq * 16, 256, 32)), dim3(256), 0, st, stage_off, res->offsets, hcnt, nq, st_tgt, st_sh, res->target,
                           res->shared);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    res->n_hits = H;
    res->n_large = NL;
    snprintf(res->plan, sizeof res->plan, "k_sr_lookup + k_sr_small (LDS sort, <= %d target ids per query); large path: %llu queries, %llu target ids",
             SR_CAP, (unsigned long long)NL, (unsigned long long)L);
    return BSK_OK;
}

// The payload pass: res holds the finished hits of search_impl(ctx, ix, qs, ...), whose rng[] (SLOT_SEARCH_RANGES) and qsum[] (SLOT_SEARCH_QUERY)
// are still in the pool -- nothing has run on this context since.  dot[] and msum[] of every hit; the thresholds have been applied already
// and read shared alone.
static int weights_impl(bsk_ctx *ctx, const bsk_index *ix, const bsk_sets *qs, bsk_hits *res) {
    hipStream_t st = ctx->stream;
    const u64 nq = qs->n_sets, nv = qs->n_values, H = res->n_hits;
    HIPCHK(ctx, grow_array(&res->dot, &res->c_dot, (H ? H : 1) * 8));
    HIPCHK(ctx, grow_array(&res->msum, &res->c_msum, (H ? H : 1) * 8));
    u64 n_rows = 0, NC = 0;
    if (H) {
        const SearchCarve cq(nq);
        void *bq = nullptr, *brng = nullptr, *bw = nullptr;
        HIPCHK(ctx, ctx_pool(ctx, SLOT_SEARCH_QUERY, cq.c.bytes, &bq));  // (both as large as the search took them: the buffers it filled)
        HIPCHK(ctx, ctx_pool(ctx, SLOT_SEARCH_RANGES, (nv ? nv : 1) * 8, &brng));
        const u64 *qsum = at<u64>(bq, cq.o_qsum), *rng = static_cast<const u64 *>(brng);
        Carve cw;
        const size_t o_coff = cw.add<u64>(nq + 1), o_rows = cw.add<u64>(nq + 1), o_part = cw.add<u64>(scan_parts(nq)), o_tot = cw.add<u64>(8);
        HIPCHK(ctx, ctx_pool(ctx, SLOT_SW_QUERY, cw.bytes, &bw));
        u64 *coff = at<u64>(bw, o_coff), *rows = at<u64>(bw, o_rows), *part = at<u64>(bw, o_part), *tot = at<u64>(bw, o_tot);
        HIPCHK(ctx, hipMemsetAsync(tot, 0, 64, st));  // [0] chunks of k_sw_chunk, [1] queries of k_sw_row
        HIPCHK(ctx, scan_counts(st, SwChunksOf{qsum, res->offsets, qs->offsets}, nq, part, coff, tot + 0, (u64 *)nullptr));
        HIPCHK(ctx, scan_counts(st, SwRowsOf{qsum, res->offsets}, nq, part, rows, tot + 1, (u64 *)nullptr));
        HIPCHK(ctx, read_back(ctx, tot, 2));
        NC = ctx->h_pinned[0];
        n_rows = ctx->h_pinned[1];
        const u32 *qcnt = qs->counted ? qs->counts : nullptr, *pcnt = ix->counted ? ix->a->post_cnt : nullptr;
        u32 *flags = nullptr;
        if (NC) {  // the rows of k_sw_chunk start from zero (those of k_sw_row are written whole)
            HIPCHK(ctx, ctx_pool(ctx, SLOT_SW_FLAGS, (H / 32 + 1) * 4, &flags));
            HIPCHK(ctx, hipMemsetAsync(flags, 0, (H / 32 + 1) * 4, st));
            HIPCHK(ctx, hipMemsetAsync(res->dot, 0, H * 8, st));
            HIPCHK(ctx, hipMemsetAsync(res->msum, 0, H * 8, st));
        }
        if (n_rows) {
            hipLaunchKernelGGL(k_sw_row, dim3(grid_for(ctx, nq, SW_WAVES, 16)), dim3(64 * SW_WAVES), 0, st, qs->offsets, rng, qsum, nq, qcnt, ix->a->post_tgt, pcnt,
                               res->offsets, res->target, res->dot, res->msum);
            HIPCHK(ctx, hipGetLastError());
        }
        if (NC) {
            hipLaunchKernelGGL(k_sw_chunk, dim3(grid_for(ctx, NC, 4, 16)), dim3(256), 0, st, qs->offsets, rng, coff, nq, NC, qcnt, ix->a->post_tgt, pcnt, res->offsets,
                               res->target, res->dot, res->msum, flags);
            hipLaunchKernelGGL(k_sw_finish, dim3(grid_for(ctx, H, 256, 16)), dim3(256), 0, st, flags, H, res->dot);
            HIPCHK(ctx, hipGetLastError());
        }
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    res->has_weights = true;
    const size_t at_ = strlen(res->plan);
    snprintf(res->plan + at_, sizeof res->plan - at_, "; weights: k_sw_row %llu queries (<= %d hits), k_sw_chunk %llu chunks of %d values", (unsigned long long)n_rows, SW_ROW,
             (unsigned long long)NC, SW_CHUNK);
    return BSK_OK;
}

static int top_impl(bsk_ctx *ctx, const bsk_hits *h, u32 n, bsk_hits *res);
extern "C" int bsk_hits_top(bsk_ctx *ctx, const bsk_hits *h, uint32_t n, bsk_hits **top) {
    if (!ctx || !h || !top) return fail_arg(ctx, "bsk_hits_top: null argument");
    if (h->ctx != ctx || (*top && (*top)->ctx != ctx)) return fail_arg(ctx, "bsk_hits_top: the hits belong to another context");
    if (*top == h) return fail_arg(ctx, "bsk_hits_top: *top is h itself");
    if (n == 0) return fail_arg(ctx, "bsk_hits_top: n == 0");
    return take_over(ctx, top, bsk_hits_release, [&](bsk_hits *res, bool) { return top_impl(ctx, h, n, res); });
}

static inline u32 bits_of(u64 x) { return x ? 64 - (u32)__builtin_clzll(x) : 0; }  // bits that hold 0 .. x

static int top_impl(bsk_ctx *ctx, const bsk_hits *h, u32 n, bsk_hits *res) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u64 nq = h->n_queries, Hin = h->n_hits;
    const bool select = n <= TOP_SELECT_N;  // else: LDS sort, and the sort path beyond TOP_LDS_KEYS hits
    res->n_queries = nq;
    res->n_hits = 0;
    res->n_large = 0;
    res->has_total = false;  // the n best carry no totals
    res->has_weights = false;  // ... and no weights
    res->has_members = false;  // ... and no members
    HIPCHK(ctx, grow_array(&res->offsets, &res->c_offsets, (nq + 1) * 8));
    // scratch: the search's own slots (its temporaries are dead once its hits exist)
    Carve cq;
    const size_t o_part = cq.add<u64>(scan_parts(nq)), o_tot = cq.add<u64>(8), o_lslot = cq.add<u64>(select ? 1 : nq + 1),
                 o_loff = cq.add<u64>(select ? 1 : nq + 1), o_lq = cq.add<u32>(select ? 1 : nq);
    void *bq = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_SEARCH_QUERY, cq.bytes, &bq));
    u64 *part = at<u64>(bq, o_part), *tot = at<u64>(bq, o_tot), *lslot = at<u64>(bq, o_lslot), *loff = at<u64>(bq, o_loff);
    u32 *lq = at<u32>(bq, o_lq);
    // [0] hits kept, [1] hits of the sort path's queries, [2] those queries, [3] the most hits one of them has, [4] the largest shared count,
    // [5] queries of the group kernel, [6] of the wave kernel
    HIPCHK(ctx, hipMemsetAsync(tot, 0, 64, st));
    HIPCHK(ctx, scan_counts(st, TopCnt{h->offsets, n}, nq, part, res->offsets, tot + 0, (u64 *)nullptr));
    if (nq) {
        hipLaunchKernelGGL(k_top_classes, dim3(grid_for(ctx, nq, 256, 8)), dim3(256), 0, st, h->offsets, nq, select ? ~0ULL : (u64)TOP_LDS_KEYS, tot + 5);
        HIPCHK(ctx, hipGetLastError());
    }
    if (!select) {
        HIPCHK(ctx, scan_counts(st, TopLargeOf{h->offsets, false}, nq, part, loff, tot + 1, tot + 3));
        HIPCHK(ctx, scan_counts(st, TopLargeOf{h->offsets, true}, nq, part, lslot, tot + 2, (u64 *)nullptr));
        if (Hin) {
            hipLaunchKernelGGL(k_top_maxshared, dim3(grid_for(ctx, Hin, 256, 8)), dim3(256), 0, st, h->shared, Hin, tot + 4);
            HIPCHK(ctx, hipGetLastError());
        }
    }
    HIPCHK(ctx, read_back(ctx, tot, 7));  // the one read-back
    const u64 H = ctx->h_pinned[0], L = ctx->h_pinned[1], NL = ctx->h_pinned[2], maxc = ctx->h_pinned[3], maxs = ctx->h_pinned[4], n_group = ctx->h_pinned[5],
              n_wave = ctx->h_pinned[6];
    HIPCHK(ctx, grow_array(&res->target, &res->c_target, (H ? H : 1) * 4));
    HIPCHK(ctx, grow_array(&res->shared, &res->c_shared, (H ? H : 1) * 4));
    if (n_group) {
        hipLaunchKernelGGL(k_top_group, dim3(grid_for(ctx, nq * 16, 256, 32)), dim3(256), 0, st, h->offsets, h->target, h->shared, nq, n, res->offsets, res->target,
                           res->shared);
        HIPCHK(ctx, hipGetLastError());
    }
    if (n_wave) {
        // queries a wavefront looks at per step: one while there are fewer queries than wavefronts (a genome query each), 64 at read scale
        const u64 waves = grid_cap_blocks(ctx, 8) * TOP_WAVES;
        u32 qb = 1;
        while (qb < 64 && (u64)qb * waves < nq) qb <<= 1;
        const unsigned grid = grid_for(ctx, (nq + qb - 1) / qb, TOP_WAVES, 8);
        if (select)
            hipLaunchKernelGGL(k_top_select, dim3(grid), dim3(64 * TOP_WAVES), 0, st, h->offsets, h->target, h->shared, nq, n, qb, res->offsets, res->target, res->shared);
        else
            hipLaunchKernelGGL(k_top_lds, dim3(grid), dim3(64 * TOP_WAVES), 0, st, h->offsets, h->target, h->shared, nq, n, qb, res->offsets, res->target, res->shared);
        HIPCHK(ctx, hipGetLastError());
    }
    if (NL) {
        const u32 bs = bits_of(maxs), bp = bits_of(maxc - 1), bslot = bits_of(NL - 1);
        if (bs + bp + bslot > 63) {
            ctx->err = "bsk_hits_top: the sort path's key (query slot, shared count, hit) needs more than 63 bits (split the queries)";
            return BSK_ERR_UNSUPPORTED;
        }
        Carve cl;
        const size_t o_in = cl.add<u64>(L), o_out = cl.add<u64>(L);
        void *bl = nullptr, *stmp = nullptr;
        HIPCHK(ctx, ctx_pool(ctx, SLOT_SEARCH_LARGE, cl.bytes, &bl));
        u64 *lin = at<u64>(bl, o_in), *lout = at<u64>(bl, o_out);
        hipLaunchKernelGGL(k_top_list, dim3(grid_for(ctx, nq, 256, 8)), dim3(256), 0, st, h->offsets, nq, lslot, lq);
        hipLaunchKernelGGL(k_top_emit, dim3(grid_for(ctx, NL, 4, 16)), dim3(256), 0, st, h->offsets, h->shared, lq, NL, loff, maxs, bs, bp, lin);
        HIPCHK(ctx, hipGetLastError());
        size_t tb = 0;
        HIPCHK(ctx, sets_sort_u64(nullptr, tb, lin, lout, (size_t)L, 0, bs + bp + bslot, st));
        HIPCHK(ctx, ctx_pool(ctx, SLOT_SEARCH_SORT_TMP, tb ? tb : 8, &stmp));
        HIPCHK(ctx, sets_sort_u64(stmp, tb, lin, lout, (size_t)L, 0, bs + bp + bslot, st));
        hipLaunchKernelGGL(k_top_place, dim3(grid_for(ctx, L, 256, 16)), dim3(256), 0, st, lout, L, h->offsets, h->target, lq, loff, maxs, bs, bp, n, res->offsets,
                           res->target, res->shared);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    res->n_hits = H;
    res->n_large = NL;
    snprintf(res->plan, sizeof res->plan, "bsk_hits_top n = %u: k_top_group %llu queries (<= %d hits); %s %llu queries; sort path: %llu queries, %llu hits", n,
             (unsigned long long)n_group, TOP_GROUP, select ? "k_top_select" : "k_top_lds", (unsigned long long)n_wave, (unsigned long long)NL,
             (unsigned long long)L);
    return BSK_OK;
}

int hits_fetch_narrow(bsk_ctx *ctx, const bsk_hits *h, uint32_t *offsets, uint32_t *target, uint32_t *shared, uint64_t hit_cap) {
    if (!ctx || !h || !offsets || !target || !shared) return fail_arg(ctx, "hits_fetch_narrow: null argument");
    if (h->ctx != ctx) return fail_arg(ctx, "hits_fetch_narrow: the hits belong to another context");
    if (h->n_hits > hit_cap) return fail_arg(ctx, "hits_fetch_narrow: hit_cap too small");
    if (h->n_hits >= (1ULL << 32)) return BSK_ERR_UNSUPPORTED;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    void *o32 = nullptr;
    const size_t need = (h->n_queries + 1) * 4;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_NARROW_OFFS, need, &o32));
    hipLaunchKernelGGL(k_off_u32, dim3(grid_for(ctx, h->n_queries + 1, 256, 8)), dim3(256), 0, ctx->stream, h->offsets, h->n_queries + 1, (u32 *)o32);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(offsets, o32, need, hipMemcpyDeviceToHost, ctx->stream));
    if (h->n_hits) {
        HIPCHK(ctx, hipMemcpyAsync(target, h->target, h->n_hits * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(shared, h->shared, h->n_hits * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BSK_OK;
}

extern "C" int bsk_hits_info(const bsk_hits *h, uint64_t *n_queries, uint64_t *n_hits) {
    if (!h) return BSK_ERR_ARG;
    if (n_queries) *n_queries = h->n_queries;
    if (n_hits) *n_hits = h->n_hits;
    return BSK_OK;
}

extern "C" int bsk_hits_plan(const bsk_hits *h, const char **plan, uint64_t *n_large_queries) {
    if (!h) return BSK_ERR_ARG;
    if (plan) *plan = h->plan;
    if (n_large_queries) *n_large_queries = h->n_large;
    return BSK_OK;
}

extern "C" int bsk_hits_device(const bsk_hits *h, const uint64_t **offsets, const uint32_t **target, const uint32_t **shared) {
    if (!h) return BSK_ERR_ARG;
    if (offsets) *offsets = (const uint64_t *)h->offsets;
    if (target) *target = (const uint32_t *)h->target;
    if (shared) *shared = (const uint32_t *)h->shared;
    return BSK_OK;
}

extern "C" int bsk_hits_fetch(bsk_ctx *ctx, const bsk_hits *h, uint64_t first, uint64_t count, uint64_t *offsets, uint32_t *target, uint32_t *shared,
                              uint64_t hit_cap) {
    if (!ctx || !h || !offsets) return fail_arg(ctx, "bsk_hits_fetch: null argument");
    if (h->ctx != ctx) return fail_arg(ctx, "bsk_hits_fetch: the hits belong to another context");
    if (first > h->n_queries || count > h->n_queries - first) return fail_arg(ctx, "bsk_hits_fetch: range outside the hits");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<u64> o(count + 1);
    HIPCHK(ctx, hipMemcpyAsync(o.data(), h->offsets + first, (count + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const u64 nh = o[count] - o[0];
    for (u64 i = 0; i <= count; ++i) offsets[i] = o[i] - o[0];
    if (!target && !shared) return BSK_OK;
    if (nh > hit_cap) return fail_arg(ctx, "bsk_hits_fetch: hit_cap too small");
    if (nh && target) HIPCHK(ctx, hipMemcpyAsync(target, h->target + o[0], nh * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (nh && shared) HIPCHK(ctx, hipMemcpyAsync(shared, h->shared + o[0], nh * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BSK_OK;
}
