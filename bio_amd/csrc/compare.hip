// compare.hip -- MinHash on the device: bottom-n sets (bsk_sets_bottom) and the dense all-pairs comparison (bsk_sets_compare), what
// mash dist / triangle, sourmash compare, dereplication and clustering start from.
//
// The tile machine.  A GEMM-shaped problem whose inner product is a merge of two sorted u64 lists.  A workgroup owns a tile of
// CMP_ROWS x CMP_COLS pairs, one lane per pair; the tile's CMP_ROWS + CMP_COLS sets pass through LDS once per tile, not once per pair.
// The pairs advance through their sets at different rates, so the sets are staged BY VALUE RANGE, in rounds.  Every set of the tile
// has an effective prefix of min(limit, size) values (no pair can walk past the limit-th value of either set) and a cursor.  A round:
//   v_hi     among the sets with more than CMP_WINDOW unstaged values, the smallest value[cursor + CMP_WINDOW]; when no set has that
//            many left this is the tile's last round and everything left is staged (a flag: any u64 is a legal value)
//   staging  every set's next min(left, CMP_WINDOW) values go to its LDS window, then a binary search in the window keeps the values
//            < v_hi: at most CMP_WINDOW of them, because value[cursor + CMP_WINDOW] >= v_hi.  The cursor moves past them.
//   merging  both windows of a pair are complete inside the round's value range, so the lane merges them to their ends: no per-pair
//            cursor survives the round, and once one window is exhausted the rest of the other is counted without being read.  A lane
//            whose total has reached the limit does nothing more.  Window ends are indices, never values.
// The set that fixed v_hi advances by a full window, so every round makes progress.  The tile stops after its last round, or as soon
// as every pair of the tile has reached the limit.
// LDS layout: a-window r at s_a[r * CMP_WINDOW + j]: the 16 lanes of a row read one address (broadcast), a 32-lane half holds two
// rows.  b-window c interleaved, s_b[j * CMP_COLS + c]: ds_read_b64 banks are (slot mod 32) = (j & 1) * 16 + c, so the lanes of a row
// -- different c, any j -- never meet on a bank, and the two rows of a half at most 2-way.  The staging thread (j, c) = (k * 16 + t / 16,
// t % 16) writes s_b[k * 256 + t]: consecutive, conflict-free.
//
// All of this is ONE device body, cmp_tile<W, NB>, and three kernels are its instantiations: k_cmp_tile <false, false>
// (bsk_sets_compare), k_cmp_tile_w <true, false> (bsk_sets_compare_counted) and k_cmp_tile_nb <false, true> (bsk_sets_neighbors).
// What a flag does not select is not in the kernel: neither its code nor its LDS (33 544 / 49 928 / 33 568 bytes a workgroup, in that
// order).  The fourth, k_cmp_tile_nb_w (bsk_sets_neighbors_counted; 49 952 bytes), does both things and is still a copy of the
// machine: instantiated from the body it measured 3.3 % slower, so a change to the machine is made twice, not once.
//
// W adds the counts: a u32 count window beside every value window -- s_ac[r * CMP_WINDOW + j] and s_bc[j * CMP_COLS + c], the indices
// of the values -- staged in the loops that stage the values, from the cursors the values use, so a value that is copied again next
// round brings its count again.  A lane reads two counts only where its two values are equal, at the indices they were read from, and
// keeps two more sums: the products (u64, saturating) and the minima (u64, exact).  An uncounted operand's count window is filled with
// ones.  ds_read_b32 banks are (dword mod 32): the lanes of a row read one a-count (broadcast) and the b-counts (j & 1) * 16 + c --
// never two lanes of a row on one bank, the two rows of a 32-lane half at most 2-way, as for the values.  The count windows are 16 KB:
// three workgroups a CU (CMP_W_BLOCKS_PER_CU), not four.
//
// NB replaces the end.  No cell is stored: every lane applies the caller's rule (shared count, exact Jaccard fraction, j > i) to its
// pair -- the rule reads shared and total only, never the weights, so the kept pairs are the same with and without W; the four ballots of
// the workgroup give the tile's kept pairs and the kept pairs of each of its rows; the tile reserves its records with ONE atomic on a
// global cursor, adds its rows' counts to row_count[] (only rows that keep something) and every keeping lane stores one 16-byte record
// (row, column, shared, total) and, in k_cmp_tile_nb_w, 16 bytes of (dot, min_sum) at the same slot of a second array.  The cursor counts every
// kept pair whether or not its record fits, so when the room is too small the host knows the exact need and runs the kernel once more.
// With BSK_NEIGHBORS_UPPER a tile whose every pair has j <= i is not run at all.  The records arrive in the order the tiles finish; the
// order of the RESULT does not depend on it: the scan of row_count[] places the rows, a record takes any free place of its row as the
// key (column << 32) | record (k_nb_keys), the library's segmented key sort orders every row by column (the columns of a row are
// distinct: the record half of a key never decides), and a gather by the sorted keys writes target, shared and total (k_nb_place) and
// the weights too (k_nb_place_w).
//
// bsk_sets_bottom: the sizes min(n, size) through the library's scan, then a gather by groups of lanes (8 per set while the kept sets
// average at most CMP_BT_SMALL values, else a wavefront per set).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "biosketch.h"
#include "host_types.hpp"
#include "search_internal.hpp"
#include "sets_internal.hpp"

#define CMP_ROWS 16            // a-sets of a tile
#define CMP_COLS 16             // b-sets of a tile
#define CMP_WINDOW 128          // values of a set staged per round: 32 windows x 128 x 8 B = 32 KB of LDS, four workgroups a CU
#define CMP_BLOCKS_PER_CU 4     // the tile grid's cap
#define CMP_W_BLOCKS_PER_CU 3   // ... and the weighted tile grid's: its count windows add 16 KB of LDS, three workgroups a CU
#define CMP_NB_FIRST_ROOM 1048576 // bsk_sets_neighbors: records the first run has room for (16 MB; weighted: 32 MB in two arrays), unless a re-used object holds more
#define CMP_BT_SMALL 16        // bsk_sets_bottom: kept values per set (average) up to which a set takes 8 lanes
#define CMP_BT_BLOCKS_PER_CU 16 // ... and its gather's cap
#define CMP_THREADS (CMP_ROWS * CMP_COLS)
#define CMP_SETS (CMP_ROWS + CMP_COLS)

struct bsk_compare {
    bsk_ctx *ctx = nullptr;
    u64 n_a = 0, n_b = 0, limit = 0;
    u32 *shared = nullptr, *total = nullptr;  // [n_a * n_b] row-major
    size_t c_shared = 0, c_total = 0;         // bytes allocated (grow-only)
    char plan[256] = "";
    u64 figures[3] = {};  // tiles run, rounds summed over the tiles, most rounds of one tile
    bool weighted = false;                // the last compare into it was bsk_sets_compare_counted: dot and min_sum are valid
    u64 *dot = nullptr, *msum = nullptr;  // [n_a * n_b] row-major (grow-only, kept by an unweighted compare)
    size_t c_dot = 0, c_msum = 0;
};

namespace {

static_assert(CMP_THREADS == 256 && CMP_THREADS / CMP_COLS == CMP_ROWS && CMP_SETS <= 64, "one lane per pair; the first wavefront keeps the sets' cursors");
static_assert(CMP_WINDOW % CMP_ROWS == 0 && (CMP_ROWS * CMP_WINDOW) % CMP_THREADS == 0, "the staging loops have no tail");

// where a tile's results go: the cells of the dense end (dot / msum with counts only) ...
struct TileCells {
    u32 *shared, *total;
    u64 *dot, *msum;
};
// ... or the rule and the records of the sparse end
struct NbRule {
    u32 min_shared, num, den, upper;  // den == 0: no Jaccard condition; upper != 0: only pairs with j > i
};
struct TileRecords {
    NbRule rule;
    u64 room;  // records that rec can hold
    uint4 *rec;
    u32 *row_count;
};

// LDS of a workgroup without counts: the value windows and cursors, and the sparse end's words, four workgroups a CU (CMP_BLOCKS_PER_CU)
// within 160 KiB; with counts (12 bytes a value) three: the statement beside k_cmp_tile_nb_w below covers k_cmp_tile_w, which has no such words
static_assert((CMP_SETS * CMP_WINDOW) * 8 + CMP_SETS * (8 + 4 + 4) + 4 + (CMP_THREADS / 64) * 4 + 8 <= 160 * 1024 / CMP_BLOCKS_PER_CU,
              "k_cmp_tile_nb: 33 308 bytes of LDS a workgroup, 40 960 available");

// the tile machine of k_cmp_tile, k_cmp_tile_w and k_cmp_tile_nb (k_cmp_tile_nb_w keeps a copy: see there).  W: counts beside the values (ac / bc NULL: an uncounted operand, every count 1).  NB: the sparse
// end -- the rule per lane and a record per kept pair -- in place of the cell store.  What an instantiation does not use (ac / bc, one of
// cells / recs, the LDS objects of the other forms) is touched under `if constexpr` only and is not in its code.
template <bool W, bool NB>
__device__ __forceinline__ void cmp_tile(const u64 *aoff, const u64 *av, const u32 *ac, u64 n_a, const u64 *boff, const u64 *bv, const u32 *bc, u64 n_b, u32 lim, u64 ntiles,
                                         u64 tiles_x, const TileCells &cells, const TileRecords &recs, u64 *fig) {
    __shared__ u64 s_a[CMP_ROWS * CMP_WINDOW];
    __shared__ u64 s_b[CMP_COLS * CMP_WINDOW];
    __shared__ u32 s_ac[CMP_ROWS * CMP_WINDOW];  // W: the count of s_a[i]
    __shared__ u32 s_bc[CMP_COLS * CMP_WINDOW];  // W: the count of s_b[i]
    __shared__ u64 s_from[CMP_SETS];             // the set's first unstaged value (index into av / bv)
    __shared__ u32 s_n[CMP_SETS];                // values copied to its window this round
    __shared__ u32 s_cnt[CMP_SETS];              // ... and how many of them lie below v_hi: the window's end
    __shared__ int s_last;
    __shared__ u32 s_wk[CMP_THREADS / 64];  // NB: kept pairs of every wavefront of the tile
    __shared__ u64 s_base;                  // NB: the tile's first record
    static_assert(!(W && NB), "both at once is k_cmp_tile_nb_w's own copy");
    const int t = threadIdx.x, r = t / CMP_COLS, c = t % CMP_COLS;
    u32 skipped = 0;
    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const u64 i0 = (tile / tiles_x) * CMP_ROWS, j0 = (tile % tiles_x) * CMP_COLS;
        if constexpr (NB) {
            if (recs.rule.upper && j0 + CMP_COLS <= i0 + 1) {  // every pair of the tile has j <= i (equal tile sides: tile column < tile row)
                ++skipped;
                continue;
            }
        }
        // threads 0 .. CMP_SETS - 1 keep a set each: rows first, then columns
        const u64 *vals = t < CMP_ROWS ? av : bv;
        u64 base = 0;
        u32 len = 0, start = 0;
        if (t < CMP_SETS) {
            const bool isa = t < CMP_ROWS;
            const u64 g = isa ? i0 + t : j0 + (t - CMP_ROWS);
            const u64 *off = isa ? aoff : boff;
            if (g < (isa ? n_a : n_b)) {
                base = off[g];
                const u64 sz = off[g + 1] - base;
                len = sz < (u64)lim ? (u32)sz : lim;
            }
        }
        const bool pair = i0 + r < n_a && j0 + c < n_b;
        u32 tot = 0, sh = 0, rounds = 0;
        u64 dt = 0, ms = 0;
        for (;;) {
            u64 cand = 0;
            bool has = false;
            if (t < CMP_SETS) {
                const u32 rem = len - start;
                has = rem > CMP_WINDOW;
                s_from[t] = base + start;
                s_n[t] = has ? CMP_WINDOW : rem;
                if (has) cand = vals[base + start + CMP_WINDOW];
            }
            __syncthreads();
            // staging: a-windows row by row (a wavefront copies 64 consecutive values), b-windows interleaved
#pragma unroll
            for (int k = 0; k < CMP_ROWS * CMP_WINDOW / CMP_THREADS; ++k) {
                const int idx = k * CMP_THREADS + t, s = idx / CMP_WINDOW, j = idx % CMP_WINDOW;
                if ((u32)j < s_n[s]) {
                    s_a[idx] = av[s_from[s] + j];
                    if constexpr (W) s_ac[idx] = ac ? ac[s_from[s] + j] : 1u;
                }
            }
#pragma unroll
            for (int k = 0; k < CMP_WINDOW / CMP_ROWS; ++k) {
                const int j = k * CMP_ROWS + r;
                if ((u32)j < s_n[CMP_ROWS + c]) {
                    s_b[k * CMP_THREADS + t] = bv[s_from[CMP_ROWS + c] + j];
                    if constexpr (W) s_bc[k * CMP_THREADS + t] = bc ? bc[s_from[CMP_ROWS + c] + j] : 1u;
                }
            }
            __syncthreads();
            if (t < 64) {  // the first wavefront: v_hi, the windows' ends, the cursors
                const bool any = __ballot(has) != 0;
                u64 vhi = has ? cand : ~0ull;  // (lanes without a candidate never undercut one; `any` says whether there is one)
                for (int d = 32; d; d >>= 1) {
                    const u64 o = __shfl_xor(vhi, d, 64);
                    vhi = o < vhi ? o : vhi;
                }
                if (t < CMP_SETS) {
                    u32 cnt = s_n[t];
                    if (any) {  // the values below v_hi
                        u32 lo = 0, hi = cnt;
                        while (lo < hi) {
                            const u32 mid = (lo + hi) >> 1;
                            const u64 v = t < CMP_ROWS ? s_a[t * CMP_WINDOW + mid] : s_b[mid * CMP_COLS + (t - CMP_ROWS)];
                            if (v < vhi) lo = mid + 1;
                            else hi = mid;
                        }
                        cnt = lo;
                    }
                    s_cnt[t] = cnt;
                    start += cnt;
                }
                if (t == 0) s_last = any ? 0 : 1;
            }
            __syncthreads();
            ++rounds;
            if (pair && tot < lim) {
                const u32 ea = s_cnt[r], eb = s_cnt[CMP_ROWS + c];
                u32 ia = 0, ib = 0;
                if (ea && eb) {
                    u64 x = s_a[r * CMP_WINDOW], y = s_b[c];
                    for (;;) {
                        ++tot;
                        const bool le = x <= y, ge = x >= y;
                        if constexpr (W) {
                            if (le && ge) {  // both hold it: its counts, from where the two values were read
                                const u32 ca = s_ac[r * CMP_WINDOW + ia], cb = s_bc[ib * CMP_COLS + c];
                                const u64 p = (u64)ca * cb;
                                ++sh;
                                dt += p;
                                dt = dt < p ? ~0ull : dt;  // saturating: a wrapped sum is below its last term
                                ms += ca < cb ? ca : cb;
                            }
                        } else {
                            sh += (le && ge) ? 1u : 0u;
                        }
                        ia += le ? 1u : 0u;
                        ib += ge ? 1u : 0u;
                        if (tot >= lim || ia >= ea || ib >= eb) break;
                        if (le) x = s_a[r * CMP_WINDOW + ia];
                        if (ge) y = s_b[ib * CMP_COLS + c];
                    }
                }
                // one window is exhausted: what the other still holds lies inside the round's range and is not in the first -- it adds to
                // the total, to no other sum
                const u32 rest = (ea - ia) + (eb - ib), left = lim - tot;
                tot += rest < left ? rest : left;
            }
            const int last = s_last;
            if (!__syncthreads_or(pair && tot < lim) || last) break;
        }
        if constexpr (NB) {
            // the epilogue: the rule per lane, the wavefronts' ballots, one reservation per tile.  A
            // wavefront holds four rows of the tile, 16 lanes each; the kept pairs are counted whether or not their records fit (the host
            // grows the room and runs once more).
            const NbRule rule = recs.rule;
            const u64 gi = i0 + r, gj = j0 + c;
            const bool keep = pair && sh >= rule.min_shared && (rule.den == 0 || (u64)sh * rule.den >= (u64)rule.num * tot) && (!rule.upper || gj > gi);
            const u64 m = __ballot(keep);
            const int lane = t & 63, w = t >> 6;
            if (lane == 0) s_wk[w] = (u32)__builtin_popcountll(m);
            __syncthreads();
            u32 before = 0, tile_kept = 0;
#pragma unroll
            for (int q = 0; q < CMP_THREADS / 64; ++q) {
                before += q < w ? s_wk[q] : 0u;
                tile_kept += s_wk[q];
            }
            if (tile_kept) {  // (the same for every thread of the workgroup)
                if (t == 0) s_base = atomicAdd((unsigned long long *)&fig[3], (unsigned long long)tile_kept);
                __syncthreads();
                const u64 slot = s_base + before + (u32)__builtin_popcountll(m & ((1ull << lane) - 1));
                if (keep && slot < recs.room) recs.rec[slot] = make_uint4((u32)gi, (u32)gj, sh, tot);
                if (c == 0) {  // the row's first lane: its 16 bits of the ballot
                    const u32 in_row = (u32)__builtin_popcountll((m >> (lane & 48)) & 0xffffull);
                    if (in_row) atomicAdd(&recs.row_count[gi], in_row);
                }
            }
        } else if (pair) {
            const u64 cell = (i0 + r) * n_b + j0 + c;
            cells.shared[cell] = sh;
            cells.total[cell] = tot;
            if constexpr (W) {
                cells.dot[cell] = dt;
                cells.msum[cell] = ms;
            }
        }
        if (t == 0) {
            atomicAdd((unsigned long long *)&fig[0], 1ull);
            atomicAdd((unsigned long long *)&fig[1], (unsigned long long)rounds);
            atomicMax((unsigned long long *)&fig[2], (unsigned long long)rounds);
        }
    }
    if constexpr (NB) {
        if (t == 0 && skipped) atomicAdd((unsigned long long *)&fig[4], (unsigned long long)skipped);
    }
}

// the three instantiations: dense (bsk_sets_compare), dense with counts (bsk_sets_compare_counted), sparse (bsk_sets_neighbors)
__global__ __launch_bounds__(CMP_THREADS) void k_cmp_tile(const u64 *aoff, const u64 *av, u64 n_a, const u64 *boff, const u64 *bv, u64 n_b, u32 lim, u64 ntiles,
                                                         u64 tiles_x, u32 *shared, u32 *total, u64 *fig) {
    cmp_tile<false, false>(aoff, av, nullptr, n_a, boff, bv, nullptr, n_b, lim, ntiles, tiles_x, TileCells{shared, total, nullptr, nullptr}, TileRecords{}, fig);
}
__global__ __launch_bounds__(CMP_THREADS) void k_cmp_tile_w(const u64 *aoff, const u64 *av, const u32 *ac, u64 n_a, const u64 *boff, const u64 *bv, const u32 *bc, u64 n_b,
                                                           u32 lim, u64 ntiles, u64 tiles_x, u32 *shared, u32 *total, u64 *dot, u64 *msum, u64 *fig) {
    cmp_tile<true, false>(aoff, av, ac, n_a, boff, bv, bc, n_b, lim, ntiles, tiles_x, TileCells{shared, total, dot, msum}, TileRecords{}, fig);
}
__global__ __launch_bounds__(CMP_THREADS) void k_cmp_tile_nb(const u64 *aoff, const u64 *av, u64 n_a, const u64 *boff, const u64 *bv, u64 n_b, u32 lim, u64 ntiles,
                                                            u64 tiles_x, NbRule rule, u64 room, uint4 *rec, u32 *row_count, u64 *fig) {
    cmp_tile<false, true>(aoff, av, nullptr, n_a, boff, bv, nullptr, n_b, lim, ntiles, tiles_x, TileCells{}, TileRecords{rule, room, rec, row_count}, fig);
}

// NOT an instantiation of the body: as cmp_tile<true, true> this kernel measured 3.3 % slower (same registers and LDS, the
// same instructions scheduled otherwise), so it keeps its own copy of the tile machine.  A change to the rounds, the staging, the cursor
// wavefront or the merge loop of cmp_tile is made here too.
// the weighted sparse tile (bsk_sets_neighbors_counted): k_cmp_tile_w's rounds and count windows, k_cmp_tile_nb's epilogue.  The rule reads
// shared and total only -- the weights are a payload -- so the kept pairs, their slots and row_count[] are those of k_cmp_tile_nb; a keeping
// lane stores its record and, at the same slot of a second array, (dot, min_sum): two 16-byte stores.
// LDS: k_cmp_tile_w's windows and cursors and the epilogue's words, three workgroups a CU (CMP_W_BLOCKS_PER_CU) within 160 KiB.
static_assert((CMP_SETS * CMP_WINDOW) * (8 + 4) + CMP_SETS * (8 + 4 + 4) + 4 + (CMP_THREADS / 64) * 4 + 8 <= 160 * 1024 / CMP_W_BLOCKS_PER_CU,
              "k_cmp_tile_nb_w: 49 692 bytes of LDS a workgroup, 54 613 available");
__global__ __launch_bounds__(CMP_THREADS) void k_cmp_tile_nb_w(const u64 *aoff, const u64 *av, const u32 *ac, u64 n_a, const u64 *boff, const u64 *bv, const u32 *bc, u64 n_b,
                                                              u32 lim, u64 ntiles, u64 tiles_x, NbRule rule, u64 room, uint4 *rec, ulonglong2 *wts, u32 *row_count,
                                                              u64 *fig) {
    __shared__ u64 s_a[CMP_ROWS * CMP_WINDOW];
    __shared__ u64 s_b[CMP_COLS * CMP_WINDOW];
    __shared__ u32 s_ac[CMP_ROWS * CMP_WINDOW];  // the count of s_a[i]
    __shared__ u32 s_bc[CMP_COLS * CMP_WINDOW];  // the count of s_b[i]
    __shared__ u64 s_from[CMP_SETS];
    __shared__ u32 s_n[CMP_SETS];
    __shared__ u32 s_cnt[CMP_SETS];
    __shared__ int s_last;
    __shared__ u32 s_wk[CMP_THREADS / 64];  // kept pairs of every wavefront of the tile
    __shared__ u64 s_base;                  // the tile's first record
    const int t = threadIdx.x, r = t / CMP_COLS, c = t % CMP_COLS;
    u32 skipped = 0;
    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const u64 i0 = (tile / tiles_x) * CMP_ROWS, j0 = (tile % tiles_x) * CMP_COLS;
        if (rule.upper && j0 + CMP_COLS <= i0 + 1) {  // every pair of the tile has j <= i
            ++skipped;
            continue;
        }
        const u64 *vals = t < CMP_ROWS ? av : bv;
        u64 base = 0;
        u32 len = 0, start = 0;
        if (t < CMP_SETS) {
            const bool isa = t < CMP_ROWS;
            const u64 g = isa ? i0 + t : j0 + (t - CMP_ROWS);
            const u64 *off = isa ? aoff : boff;
            if (g < (isa ? n_a : n_b)) {
                base = off[g];
                const u64 sz = off[g + 1] - base;
                len = sz < (u64)lim ? (u32)sz : lim;
            }
        }
        const bool pair = i0 + r < n_a && j0 + c < n_b;
        u32 tot = 0, sh = 0, rounds = 0;
        u64 dt = 0, ms = 0;
        for (;;) {
            u64 cand = 0;
            bool has = false;
            if (t < CMP_SETS) {
                const u32 rem = len - start;
                has = rem > CMP_WINDOW;
                s_from[t] = base + start;
                s_n[t] = has ? CMP_WINDOW : rem;
                if (has) cand = vals[base + start + CMP_WINDOW];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < CMP_ROWS * CMP_WINDOW / CMP_THREADS; ++k) {
                const int idx = k * CMP_THREADS + t, s = idx / CMP_WINDOW, j = idx % CMP_WINDOW;
                if ((u32)j < s_n[s]) {
                    s_a[idx] = av[s_from[s] + j];
                    s_ac[idx] = ac ? ac[s_from[s] + j] : 1u;
                }
            }
#pragma unroll
            for (int k = 0; k < CMP_WINDOW / CMP_ROWS; ++k) {
                const int j = k * CMP_ROWS + r;
                if ((u32)j < s_n[CMP_ROWS + c]) {
                    s_b[k * CMP_THREADS + t] = bv[s_from[CMP_ROWS + c] + j];
                    s_bc[k * CMP_THREADS + t] = bc ? bc[s_from[CMP_ROWS + c] + j] : 1u;
                }
            }
            __syncthreads();
            if (t < 64) {
                const bool any = __ballot(has) != 0;
                u64 vhi = has ? cand : ~0ull;
                for (int d = 32; d; d >>= 1) {
                    const u64 o = __shfl_xor(vhi, d, 64);
                    vhi = o < vhi ? o : vhi;
                }
                if (t < CMP_SETS) {
                    u32 cnt = s_n[t];
                    if (any) {
                        u32 lo = 0, hi = cnt;
                        while (lo < hi) {
                            const u32 mid = (lo + hi) >> 1;
                            const u64 v = t < CMP_ROWS ? s_a[t * CMP_WINDOW + mid] : s_b[mid * CMP_COLS + (t - CMP_ROWS)];
                            if (v < vhi) lo = mid + 1;
                            else hi = mid;
                        }
                        cnt = lo;
                    }
                    s_cnt[t] = cnt;
                    start += cnt;
                }
                if (t == 0) s_last = any ? 0 : 1;
            }
            __syncthreads();
            ++rounds;
            if (pair && tot < lim) {
                const u32 ea = s_cnt[r], eb = s_cnt[CMP_ROWS + c];
                u32 ia = 0, ib = 0;
                if (ea && eb) {
                    u64 x = s_a[r * CMP_WINDOW], y = s_b[c];
                    for (;;) {
                        ++tot;
                        const bool le = x <= y, ge = x >= y;
                        if (le && ge) {  // both hold it: its counts, from where the two values were read
                            const u32 ca = s_ac[r * CMP_WINDOW + ia], cb = s_bc[ib * CMP_COLS + c];
                            const u64 p = (u64)ca * cb;
                            ++sh;
                            dt += p;
                            dt = dt < p ? ~0ull : dt;  // saturating: a wrapped sum is below its last term
                            ms += ca < cb ? ca : cb;
                        }
                        ia += le ? 1u : 0u;
                        ib += ge ? 1u : 0u;
                        if (tot >= lim || ia >= ea || ib >= eb) break;
                        if (le) x = s_a[r * CMP_WINDOW + ia];
                        if (ge) y = s_b[ib * CMP_COLS + c];
                    }
                }
                const u32 rest = (ea - ia) + (eb - ib), left = lim - tot;
                tot += rest < left ? rest : left;
            }
            const int last = s_last;
            if (!__syncthreads_or(pair && tot < lim) || last) break;
        }
        // the epilogue of k_cmp_tile_nb: the rule per lane (the weights take no part in it), four ballots, one reservation per tile
        const u64 gi = i0 + r, gj = j0 + c;
        const bool keep = pair && sh >= rule.min_shared && (rule.den == 0 || (u64)sh * rule.den >= (u64)rule.num * tot) && (!rule.upper || gj > gi);
        const u64 m = __ballot(keep);
        const int lane = t & 63, w = t >> 6;
        if (lane == 0) s_wk[w] = (u32)__builtin_popcountll(m);
        __syncthreads();
        u32 before = 0, tile_kept = 0;
#pragma unroll
        for (int q = 0; q < CMP_THREADS / 64; ++q) {
            before += q < w ? s_wk[q] : 0u;
            tile_kept += s_wk[q];
        }
        if (tile_kept) {  // (the same for every thread of the workgroup)
            if (t == 0) s_base = atomicAdd((unsigned long long *)&fig[3], (unsigned long long)tile_kept);
            __syncthreads();
            const u64 slot = s_base + before + (u32)__builtin_popcountll(m & ((1ull << lane) - 1));
            if (keep && slot < room) {
                rec[slot] = make_uint4((u32)gi, (u32)gj, sh, tot);
                wts[slot] = make_ulonglong2(dt, ms);
            }
            if (c == 0) {  // the row's first lane: its 16 bits of the ballot
                const u32 in_row = (u32)__builtin_popcountll((m >> (lane & 48)) & 0xffffull);
                if (in_row) atomicAdd(&row_count[gi], in_row);
            }
        }
        if (t == 0) {
            atomicAdd((unsigned long long *)&fig[0], 1ull);
            atomicAdd((unsigned long long *)&fig[1], (unsigned long long)rounds);
            atomicMax((unsigned long long *)&fig[2], (unsigned long long)rounds);
        }
    }
    if (t == 0 && skipped) atomicAdd((unsigned long long *)&fig[4], (unsigned long long)skipped);
}

// the kept pairs' records to their rows: record s of row i takes a place of [off[i], off[i + 1]) -- which one depends on the order of
// arrival and does not matter -- as the key (column << 32) | s; the columns of a row are distinct, so sorting a row's keys orders its columns
__global__ __launch_bounds__(256) void k_nb_keys(const uint4 *rec, u64 n, const u64 *off, u32 *row_count, u64 *keys) {
    for (u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (u64)gridDim.x * blockDim.x) {
        const uint4 p = rec[s];
        const u32 left = atomicSub(&row_count[p.x], 1u);  // (the row's count, down to 1)
        keys[off[p.x] + left - 1] = ((u64)p.y << 32) | s;
    }
}
__global__ __launch_bounds__(256) void k_nb_place(const u64 *keys, u64 n, const uint4 *rec, u32 *tgt, u32 *sh, u32 *tot) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 k = keys[i];
        const uint4 p = rec[(u32)k];
        tgt[i] = (u32)(k >> 32);
        sh[i] = p.z;
        tot[i] = p.w;
    }
}
// ... and the weights of the weighted records, by the same keys
__global__ __launch_bounds__(256) void k_nb_place_w(const u64 *keys, u64 n, const uint4 *rec, const ulonglong2 *wts, u32 *tgt, u32 *sh, u32 *tot, u64 *dot, u64 *msum) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 k = keys[i];
        const uint4 p = rec[(u32)k];
        const ulonglong2 q = wts[(u32)k];
        tgt[i] = (u32)(k >> 32);
        sh[i] = p.z;
        tot[i] = p.w;
        dot[i] = q.x;
        msum[i] = q.y;
    }
}

// ---- bsk_sets_bottom ----
struct BtSize {  // what set r keeps
    const u64 *offs;
    u64 n;
    __device__ __forceinline__ u64 operator()(u64 r) const {
        const u64 s = offs[r + 1] - offs[r];
        return s < n ? s : n;
    }
};
template <int LANES>
__global__ __launch_bounds__(256) void k_bt_gather(const u64 *ioff, const u64 *iv, const u32 *ic, const u64 *ooff, u64 n_sets, u64 *ov, u32 *oc) {
    const u64 lane = threadIdx.x % LANES;
    for (u64 s = ((u64)blockIdx.x * 256 + threadIdx.x) / LANES; s < n_sets; s += (u64)gridDim.x * (256 / LANES)) {
        const u64 src = ioff[s], dst = ooff[s], cnt = ooff[s + 1] - dst;
        for (u64 j = lane; j < cnt; j += LANES) {
            ov[dst + j] = iv[src + j];
            if (ic) oc[dst + j] = ic[src + j];
        }
    }
}

int bottom_impl(bsk_ctx *ctx, const bsk_sets *s, u64 n, bsk_sets *res) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u64 G = s->n_sets;
    res->n_sets = G;
    res->n_values = 0;
    res->counted = false;
    res->plan[0] = 0;
    res->by_path[0] = res->by_path[1] = res->by_path[2] = 0;
    HIPCHK(ctx, grow_array(&res->offsets, &res->c_offsets, (G + 1) * 8));
    void *bq = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_BOTTOM_SCAN, (scan_parts(G) + 8) * 8, &bq));
    u64 *tot = static_cast<u64 *>(bq), *part = tot + 8;
    HIPCHK(ctx, hipMemsetAsync(tot, 0, 64, st));
    HIPCHK(ctx, scan_counts(st, BtSize{s->offsets, n}, G, part, res->offsets, tot, (u64 *)nullptr));
    HIPCHK(ctx, read_back(ctx, tot, 1));
    const u64 M = ctx->h_pinned[0];
    HIPCHK(ctx, grow_array(&res->values, &res->c_values, (M ? M : 1) * 8));
    if (s->counted) HIPCHK(ctx, sets_grow_counts(res, M ? M : 1, true));
    if (M) {
        const u32 *ic = s->counted ? s->counts : nullptr;
        const bool small = M <= G * CMP_BT_SMALL;
        const u64 per_block = small ? 256 / 8 : 256 / 64;
        const unsigned grid = grid_for(ctx, G, per_block, CMP_BT_BLOCKS_PER_CU);
        if (small) hipLaunchKernelGGL(k_bt_gather<8>, dim3(grid), dim3(256), 0, st, s->offsets, s->values, ic, res->offsets, G, res->values, res->counts);
        else hipLaunchKernelGGL(k_bt_gather<64>, dim3(grid), dim3(256), 0, st, s->offsets, s->values, ic, res->offsets, G, res->values, res->counts);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    res->n_values = M;
    res->counted = s->counted;
    return BSK_OK;
}

int compare_impl(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, u64 limit, bsk_compare *res, bool weighted) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u64 n_a = a->n_sets, n_b = b->n_sets, cells = n_a * n_b;
    res->n_a = n_a;
    res->n_b = n_b;
    res->limit = limit;
    res->figures[0] = res->figures[1] = res->figures[2] = 0;
    res->weighted = false;  // (an unweighted compare into a weighted object keeps the two arrays, like a counted bsk_sets written by an uncounted entry)
    HIPCHK(ctx, grow_array(&res->shared, &res->c_shared, (cells ? cells : 1) * 4));
    HIPCHK(ctx, grow_array(&res->total, &res->c_total, (cells ? cells : 1) * 4));
    if (weighted) {
        HIPCHK(ctx, grow_array(&res->dot, &res->c_dot, (cells ? cells : 1) * 8));
        HIPCHK(ctx, grow_array(&res->msum, &res->c_msum, (cells ? cells : 1) * 8));
    }
    if (cells == 0) {
        snprintf(res->plan, sizeof res->plan, weighted ? "bsk_sets_compare_counted: no pairs" : "bsk_sets_compare: no pairs");
        res->weighted = weighted;
        return BSK_OK;
    }
    void *bf = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_COMPARE_FIGURES, 64, &bf));
    u64 *fig = static_cast<u64 *>(bf);
    HIPCHK(ctx, hipMemsetAsync(fig, 0, 64, st));
    const u64 tiles_x = (n_b + CMP_COLS - 1) / CMP_COLS, ntiles = ((n_a + CMP_ROWS - 1) / CMP_ROWS) * tiles_x;
    // the inputs hold fewer than 2^32 values together, so no total reaches 2^32 - 1 before its union ends
    const u32 lim = limit == 0 || limit > 0xffffffffull ? 0xffffffffu : (u32)limit;
    const unsigned grid = capped_grid(ctx, ntiles, weighted ? CMP_W_BLOCKS_PER_CU : CMP_BLOCKS_PER_CU);
    if (weighted)
        hipLaunchKernelGGL(k_cmp_tile_w, dim3(grid), dim3(CMP_THREADS), 0, st, (const u64 *)a->offsets, (const u64 *)a->values, (const u32 *)(a->counted ? a->counts : nullptr), n_a,
                           (const u64 *)b->offsets, (const u64 *)b->values, (const u32 *)(b->counted ? b->counts : nullptr), n_b, lim, ntiles, tiles_x, res->shared, res->total,
                           res->dot, res->msum, fig);
    else
        hipLaunchKernelGGL(k_cmp_tile, dim3(grid), dim3(CMP_THREADS), 0, st, (const u64 *)a->offsets, (const u64 *)a->values, n_a, (const u64 *)b->offsets, (const u64 *)b->values, n_b,
                           lim, ntiles, tiles_x, res->shared, res->total, fig);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, read_back(ctx, fig, 3));
    for (int i = 0; i < 3; ++i) res->figures[i] = ctx->h_pinned[i];
    snprintf(res->plan, sizeof res->plan, "%s, %llu x %llu pairs in %llu tiles of %d x %d, windows of %d values, limit %llu",
             weighted ? "bsk_sets_compare_counted: k_cmp_tile_w" : "bsk_sets_compare: k_cmp_tile", (unsigned long long)n_a, (unsigned long long)n_b, (unsigned long long)ntiles,
             CMP_ROWS, CMP_COLS, CMP_WINDOW, (unsigned long long)limit);
    res->weighted = weighted;
    return BSK_OK;
}

// bsk_sets_neighbors: k_cmp_tile_nb (once more when the kept pairs outgrow the room), the row counts to offsets, the records to their
// rows, every row into ascending column order, the gather.  Memory follows n_a and the kept pairs, never the cells.
// `weighted` (bsk_sets_neighbors_counted): k_cmp_tile_nb_w, a second record array for (dot, min_sum), and a gather that places them too.
int neighbors_impl(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, u64 limit, const NbRule &rule, bsk_hits *res, bool reused, bool weighted) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const char *who = weighted ? "bsk_sets_neighbors_counted" : "bsk_sets_neighbors";
    const u64 n_a = a->n_sets, n_b = b->n_sets;
    res->n_queries = n_a;
    res->n_hits = 0;
    res->n_large = 0;
    res->has_total = false;
    res->has_weights = false;  // (an unweighted call into weighted hits keeps the two arrays)
    res->has_members = false;  // (neighbours carry no members)
    HIPCHK(ctx, grow_array(&res->offsets, &res->c_offsets, (n_a + 1) * 8));
    if (n_a == 0 || n_b == 0) {
        HIPCHK(ctx, hipMemsetAsync(res->offsets, 0, (n_a + 1) * 8, st));
        HIPCHK(ctx, grow_array(&res->target, &res->c_target, 4));
        HIPCHK(ctx, grow_array(&res->shared, &res->c_shared, 4));
        HIPCHK(ctx, grow_array(&res->total, &res->c_total, 4));
        if (weighted) {
            HIPCHK(ctx, grow_array(&res->dot, &res->c_dot, 8));
            HIPCHK(ctx, grow_array(&res->msum, &res->c_msum, 8));
        }
        HIPCHK(ctx, hipStreamSynchronize(st));
        res->has_total = true;
        res->has_weights = weighted;
        snprintf(res->plan, sizeof res->plan, "%s: no pairs, tiles=0 skipped=0 rounds=0 runs=0", who);
        return BSK_OK;
    }
    const u64 tiles_y = (n_a + CMP_ROWS - 1) / CMP_ROWS, tiles_x = (n_b + CMP_COLS - 1) / CMP_COLS, ntiles = tiles_y * tiles_x;  // (both below 2^28: no overflow)
    // the first room: the named constant (or the switch), or what a re-used object already holds; never more than the cells
    u64 room = ctx->opt.nb_room ? ctx->opt.nb_room : CMP_NB_FIRST_ROOM;
    if (reused) {
        u64 holds = std::min(std::min(res->c_target, res->c_shared), res->c_total) / 4;  // the smallest array, in elements
        if (weighted) holds = std::min<u64>(holds, std::min(res->c_dot, res->c_msum) / 8);
        room = std::max(room, holds);
    }
    room = std::min(room, n_b > room / n_a ? room : n_a * n_b);
    Carve cq;
    const size_t o_fig = cq.add<u64>(8), o_rows = cq.add<u32>(n_a), o_part = cq.add<u64>(scan_parts(n_a));
    void *bq = nullptr, *brec = nullptr, *bwts = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_NB_ROWS, cq.bytes, &bq));
    u64 *fig = at<u64>(bq, o_fig), *part = at<u64>(bq, o_part);  // fig: tiles run, rounds, most rounds of a tile, kept pairs, tiles skipped, (scan) hits
    u32 *row_count = at<u32>(bq, o_rows);
    const u32 lim = limit == 0 || limit > 0xffffffffull ? 0xffffffffu : (u32)limit;
    const unsigned grid = capped_grid(ctx, ntiles, weighted ? CMP_W_BLOCKS_PER_CU : CMP_BLOCKS_PER_CU);
    u64 kept = 0;
    int runs = 0;
    for (;;) {
        HIPCHK(ctx, ctx_pool(ctx, SLOT_NB_RECORDS, room * 16, &brec));
        if (weighted) HIPCHK(ctx, ctx_pool(ctx, SLOT_NB_WEIGHTS, room * 16, &bwts));
        HIPCHK(ctx, hipMemsetAsync(bq, 0, o_part, st));  // the figures and the row counts
        if (weighted)
            hipLaunchKernelGGL(k_cmp_tile_nb_w, dim3(grid), dim3(CMP_THREADS), 0, st, (const u64 *)a->offsets, (const u64 *)a->values,
                               (const u32 *)(a->counted ? a->counts : nullptr), n_a, (const u64 *)b->offsets, (const u64 *)b->values,
                               (const u32 *)(b->counted ? b->counts : nullptr), n_b, lim, ntiles, tiles_x, rule, room, static_cast<uint4 *>(brec),
                               static_cast<ulonglong2 *>(bwts), row_count, fig);
        else
            hipLaunchKernelGGL(k_cmp_tile_nb, dim3(grid), dim3(CMP_THREADS), 0, st, (const u64 *)a->offsets, (const u64 *)a->values, n_a, (const u64 *)b->offsets,
                               (const u64 *)b->values, n_b, lim, ntiles, tiles_x, rule, room, static_cast<uint4 *>(brec), row_count, fig);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, read_back(ctx, fig, 5));
        ++runs;
        kept = ctx->h_pinned[3];
        if (kept <= room) break;
        if (runs == 2) {  // (the count of a run does not depend on the room)
            ctx->err = std::string(who) + ": the kept pairs changed between two runs";
            return BSK_ERR_DEVICE;
        }
        if (kept >= (1ULL << 32)) {
            ctx->err = std::string(who) + ": 2^32 kept pairs or more (raise the thresholds or split the sets)";
            return BSK_ERR_UNSUPPORTED;
        }
        room = kept;
    }
    const u64 tiles_run = ctx->h_pinned[0], rounds = ctx->h_pinned[1], skipped = ctx->h_pinned[4];
    const uint4 *rec = static_cast<const uint4 *>(brec);
    HIPCHK(ctx, scan_counts(st, KeepOf{row_count}, n_a, part, res->offsets, fig + 5, (u64 *)nullptr));
    HIPCHK(ctx, grow_array(&res->target, &res->c_target, (kept ? kept : 1) * 4));
    HIPCHK(ctx, grow_array(&res->shared, &res->c_shared, (kept ? kept : 1) * 4));
    HIPCHK(ctx, grow_array(&res->total, &res->c_total, (kept ? kept : 1) * 4));
    if (weighted) {
        HIPCHK(ctx, grow_array(&res->dot, &res->c_dot, (kept ? kept : 1) * 8));
        HIPCHK(ctx, grow_array(&res->msum, &res->c_msum, (kept ? kept : 1) * 8));
    }
    if (kept) {
        size_t tb = 0;
        HIPCHK(ctx, sets_sort_segments_u64(nullptr, tb, nullptr, nullptr, kept, n_a, res->offsets, st));
        Carve cs;
        const size_t o_in = cs.add<u64>(kept), o_out = cs.add<u64>(kept), o_tmp = cs.add<char>(tb ? tb : 8);
        void *bs = nullptr;
        HIPCHK(ctx, ctx_pool(ctx, SLOT_NB_SORT, cs.bytes, &bs));
        u64 *kin = at<u64>(bs, o_in), *kout = at<u64>(bs, o_out);
        hipLaunchKernelGGL(k_nb_keys, dim3(grid_for(ctx, kept, 256, 16)), dim3(256), 0, st, rec, kept, (const u64 *)res->offsets, row_count, kin);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, sets_sort_segments_u64(at<char>(bs, o_tmp), tb, kin, kout, kept, n_a, res->offsets, st));
        if (weighted)
            hipLaunchKernelGGL(k_nb_place_w, dim3(grid_for(ctx, kept, 256, 16)), dim3(256), 0, st, (const u64 *)kout, kept, rec, static_cast<const ulonglong2 *>(bwts),
                               res->target, res->shared, res->total, res->dot, res->msum);
        else
            hipLaunchKernelGGL(k_nb_place, dim3(grid_for(ctx, kept, 256, 16)), dim3(256), 0, st, (const u64 *)kout, kept, rec, res->target, res->shared, res->total);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    res->n_hits = kept;
    res->has_total = true;
    res->has_weights = weighted;
    snprintf(res->plan, sizeof res->plan, "%s: %s, %llu x %llu pairs, limit %llu, tiles=%llu skipped=%llu rounds=%llu runs=%d", who, weighted ? "k_cmp_tile_nb_w" : "k_cmp_tile_nb",
             (unsigned long long)n_a, (unsigned long long)n_b, (unsigned long long)limit, (unsigned long long)tiles_run, (unsigned long long)skipped, (unsigned long long)rounds, runs);
    return BSK_OK;
}

}  // namespace

namespace {
int neighbors_entry(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, uint64_t limit, const bsk_neighbor_params *np, bsk_hits **hits, bool weighted);
}  // namespace

extern "C" int bsk_sets_neighbors(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, uint64_t limit, const bsk_neighbor_params *np, bsk_hits **hits) {
    return neighbors_entry(ctx, a, b, limit, np, hits, false);
}

// bsk_sets_neighbors with the counts: the same checks in the same order, the same rule, and (dot, min_sum) beside every kept pair
extern "C" int bsk_sets_neighbors_counted(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, uint64_t limit, const bsk_neighbor_params *np, bsk_hits **hits) {
    return neighbors_entry(ctx, a, b, limit, np, hits, true);
}

namespace {
// the checks and the *hits rules both entries share; `weighted`: bsk_sets_neighbors_counted
int neighbors_entry(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, uint64_t limit, const bsk_neighbor_params *np, bsk_hits **hits, bool weighted) {
    if (!ctx || !a || !b || !hits) return fail_arg(ctx, weighted ? "bsk_sets_neighbors_counted: null argument" : "bsk_sets_neighbors: null argument");
    NbRule rule{1, 0, 0, 0};
    if (np) {
        if (np->flags & ~(uint32_t)BSK_NEIGHBORS_UPPER) return fail_arg(ctx, weighted ? "bsk_sets_neighbors_counted: unknown flag" : "bsk_sets_neighbors: unknown flag");
        if (np->jaccard_den != 0 && np->jaccard_num > np->jaccard_den)
            return fail_arg(ctx, weighted ? "bsk_sets_neighbors_counted: jaccard_num > jaccard_den" : "bsk_sets_neighbors: jaccard_num > jaccard_den");
        rule = NbRule{np->min_shared ? np->min_shared : 1u, np->jaccard_num, np->jaccard_den, np->flags & BSK_NEIGHBORS_UPPER};
    }
    if (a->ctx != ctx || b->ctx != ctx || (*hits && (*hits)->ctx != ctx))
        return fail_arg(ctx, weighted ? "bsk_sets_neighbors_counted: the sets or the hits belong to another context" : "bsk_sets_neighbors: the sets or the hits belong to another context");
    return take_over(ctx, hits, bsk_hits_release, [&](bsk_hits *res, bool reused) -> int {
        // the limits after the slot is taken, as in bsk_sets_compare: a re-used object is released (a == b holds its values once)
        const u64 held = a == b ? a->n_values : a->n_values + b->n_values;
        if (a->n_values >= (1ULL << 32) || b->n_values >= (1ULL << 32) || held >= (1ULL << 32)) {
            ctx->err = weighted ? "bsk_sets_neighbors_counted: 2^32 values or more (split the sets)" : "bsk_sets_neighbors: 2^32 values or more (split the sets)";
            return BSK_ERR_UNSUPPORTED;
        }
        if (a->n_sets >= (1ULL << 32) || b->n_sets >= (1ULL << 32)) {  // targets are u32, and so are a record's row and the sort's segments
            ctx->err = weighted ? "bsk_sets_neighbors_counted: 2^32 sets or more (split the sets)" : "bsk_sets_neighbors: 2^32 sets or more (split the sets)";
            return BSK_ERR_UNSUPPORTED;
        }
        return neighbors_impl(ctx, a, b, limit, rule, res, reused, weighted);
    });
}
}  // namespace

extern "C" int bsk_hits_weights_device(const bsk_hits *h, const uint64_t **dot, const uint64_t **min_sum) {
    if (!h) return BSK_ERR_ARG;
    if (dot) *dot = h->has_weights ? (const uint64_t *)h->dot : nullptr;
    if (min_sum) *min_sum = h->has_weights ? (const uint64_t *)h->msum : nullptr;
    return BSK_OK;
}

extern "C" int bsk_hits_fetch_weights(bsk_ctx *ctx, const bsk_hits *h, uint64_t first, uint64_t count, uint64_t *dot, uint64_t *min_sum, uint64_t hit_cap) {
    if (!ctx || !h) return fail_arg(ctx, "bsk_hits_fetch_weights: null argument");
    if (h->ctx != ctx) return fail_arg(ctx, "bsk_hits_fetch_weights: the hits belong to another context");
    if (!h->has_weights) return fail_arg(ctx, "bsk_hits_fetch_weights: the hits carry no weights (bsk_sets_neighbors_counted makes such)");
    if (first > h->n_queries || count > h->n_queries - first) return fail_arg(ctx, "bsk_hits_fetch_weights: range outside the hits");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, h->offsets + first, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned + 1, h->offsets + first + count, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const u64 o0 = ctx->h_pinned[0], nh = ctx->h_pinned[1] - o0;
    if (nh > hit_cap) return fail_arg(ctx, "bsk_hits_fetch_weights: hit_cap too small");
    if (nh && dot) HIPCHK(ctx, hipMemcpyAsync(dot, h->dot + o0, nh * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (nh && min_sum) HIPCHK(ctx, hipMemcpyAsync(min_sum, h->msum + o0, nh * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BSK_OK;
}

extern "C" int bsk_hits_totals_device(const bsk_hits *h, const uint32_t **total) {
    if (!h) return BSK_ERR_ARG;
    if (total) *total = h->has_total ? (const uint32_t *)h->total : nullptr;
    return BSK_OK;
}

extern "C" int bsk_hits_fetch_totals(bsk_ctx *ctx, const bsk_hits *h, uint64_t first, uint64_t count, uint32_t *total, uint64_t hit_cap) {
    if (!ctx || !h || !total) return fail_arg(ctx, "bsk_hits_fetch_totals: null argument");
    if (h->ctx != ctx) return fail_arg(ctx, "bsk_hits_fetch_totals: the hits belong to another context");
    if (!h->has_total) return fail_arg(ctx, "bsk_hits_fetch_totals: the hits carry no totals (bsk_sets_neighbors makes such)");
    if (first > h->n_queries || count > h->n_queries - first) return fail_arg(ctx, "bsk_hits_fetch_totals: range outside the hits");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, h->offsets + first, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned + 1, h->offsets + first + count, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const u64 o0 = ctx->h_pinned[0], nh = ctx->h_pinned[1] - o0;
    if (nh > hit_cap) return fail_arg(ctx, "bsk_hits_fetch_totals: hit_cap too small");
    if (nh) HIPCHK(ctx, hipMemcpyAsync(total, h->total + o0, nh * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BSK_OK;
}

extern "C" void bsk_compare_release(bsk_compare *c) {
    if (!c) return;
    if (c->ctx) (void)hipSetDevice(c->ctx->device);
    (void)hipFree(c->shared);
    (void)hipFree(c->total);
    (void)hipFree(c->dot);
    (void)hipFree(c->msum);
    delete c;
}

extern "C" int bsk_sets_bottom(bsk_ctx *ctx, const bsk_sets *s, uint64_t n, bsk_sets **out) {
    if (!ctx || !s || !out) return fail_arg(ctx, "bsk_sets_bottom: null argument");
    if (s->ctx != ctx || (*out && (*out)->ctx != ctx)) return fail_arg(ctx, "bsk_sets_bottom: the sets belong to another context");
    if (*out == s) return fail_arg(ctx, "bsk_sets_bottom: *out is the input");
    if (n == 0) return fail_arg(ctx, "bsk_sets_bottom: n == 0");
    return take_over(ctx, out, bsk_sets_release, [&](bsk_sets *res, bool) { return bottom_impl(ctx, s, n, res); });
}

namespace {
// the checks and the *cmp rules both compares share; `weighted`: bsk_sets_compare_counted
int compare_entry(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, uint64_t limit, bsk_compare **cmp, bool weighted) {
    if (!ctx || !a || !b || !cmp) return fail_arg(ctx, weighted ? "bsk_sets_compare_counted: null argument" : "bsk_sets_compare: null argument");
    if (a->ctx != ctx || b->ctx != ctx || (*cmp && (*cmp)->ctx != ctx))
        return fail_arg(ctx, weighted ? "bsk_sets_compare_counted: the sets or the result belong to another context" : "bsk_sets_compare: the sets or the result belong to another context");
    return take_over(ctx, cmp, bsk_compare_release, [&](bsk_compare *res, bool) -> int {
        // both limits after the slot is taken: a re-used object is released (a == b holds its values once)
        const u64 held = a == b ? a->n_values : a->n_values + b->n_values;
        const bool many_values = a->n_values >= (1ULL << 32) || b->n_values >= (1ULL << 32) || held >= (1ULL << 32);
        const bool many_cells = a->n_sets && b->n_sets > (1ULL << 31) / a->n_sets;
        if (many_values || many_cells) {
            if (weighted) ctx->err = many_values ? "bsk_sets_compare_counted: 2^32 values or more (split the sets)" : "bsk_sets_compare_counted: more than 2^31 cells (split the sets)";
            else ctx->err = many_values ? "bsk_sets_compare: 2^32 values or more (split the sets)" : "bsk_sets_compare: more than 2^31 cells (split the sets)";
            return BSK_ERR_UNSUPPORTED;
        }
        return compare_impl(ctx, a, b, limit, res, weighted);
    });
}
}  // namespace

extern "C" int bsk_sets_compare(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, uint64_t limit, bsk_compare **cmp) { return compare_entry(ctx, a, b, limit, cmp, false); }

extern "C" int bsk_sets_compare_counted(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, uint64_t limit, bsk_compare **cmp) { return compare_entry(ctx, a, b, limit, cmp, true); }

extern "C" int bsk_compare_info(const bsk_compare *c, uint64_t *n_a, uint64_t *n_b, uint64_t *limit) {
    if (!c) return BSK_ERR_ARG;
    if (n_a) *n_a = c->n_a;
    if (n_b) *n_b = c->n_b;
    if (limit) *limit = c->limit;
    return BSK_OK;
}

extern "C" int bsk_compare_plan(const bsk_compare *c, const char **plan, uint64_t figures[3]) {
    if (!c) return BSK_ERR_ARG;
    if (plan) *plan = c->plan;
    if (figures)
        for (int i = 0; i < 3; ++i) figures[i] = c->figures[i];
    return BSK_OK;
}

extern "C" int bsk_compare_fetch(bsk_ctx *ctx, const bsk_compare *c, uint64_t first_row, uint64_t n_rows, uint32_t *shared, uint32_t *total, uint64_t cell_cap) {
    if (!ctx || !c) return fail_arg(ctx, "bsk_compare_fetch: null argument");
    if (c->ctx != ctx) return fail_arg(ctx, "bsk_compare_fetch: the result belongs to another context");
    if (first_row > c->n_a || n_rows > c->n_a - first_row) return fail_arg(ctx, "bsk_compare_fetch: rows outside the matrix");
    const u64 cells = n_rows * c->n_b;  // (at most 2^31)
    if (cells > cell_cap) return fail_arg(ctx, "bsk_compare_fetch: cell_cap too small");
    if (cells == 0 || (!shared && !total)) return BSK_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (shared) HIPCHK(ctx, hipMemcpyAsync(shared, c->shared + first_row * c->n_b, cells * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (total) HIPCHK(ctx, hipMemcpyAsync(total, c->total + first_row * c->n_b, cells * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BSK_OK;
}

extern "C" int bsk_compare_device(const bsk_compare *c, const uint32_t **shared, const uint32_t **total) {
    if (!c) return BSK_ERR_ARG;
    if (shared) *shared = c->shared;
    if (total) *total = c->total;
    return BSK_OK;
}

extern "C" int bsk_compare_weights_device(const bsk_compare *c, const uint64_t **dot, const uint64_t **min_sum) {
    if (!c) return BSK_ERR_ARG;
    if (dot) *dot = c->weighted ? (const uint64_t *)c->dot : nullptr;
    if (min_sum) *min_sum = c->weighted ? (const uint64_t *)c->msum : nullptr;
    return BSK_OK;
}

extern "C" int bsk_compare_fetch_weights(bsk_ctx *ctx, const bsk_compare *c, uint64_t first_row, uint64_t n_rows, uint64_t *dot, uint64_t *min_sum, uint64_t cell_cap) {
    if (!ctx || !c) return fail_arg(ctx, "bsk_compare_fetch_weights: null argument");
    if (c->ctx != ctx) return fail_arg(ctx, "bsk_compare_fetch_weights: the result belongs to another context");
    if (!c->weighted) return fail_arg(ctx, "bsk_compare_fetch_weights: the result is not weighted (bsk_sets_compare_counted makes one)");
    if (first_row > c->n_a || n_rows > c->n_a - first_row) return fail_arg(ctx, "bsk_compare_fetch_weights: rows outside the matrix");
    const u64 cells = n_rows * c->n_b;  // (at most 2^31)
    if (cells > cell_cap) return fail_arg(ctx, "bsk_compare_fetch_weights: cell_cap too small");
    if (cells == 0 || (!dot && !min_sum)) return BSK_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (dot) HIPCHK(ctx, hipMemcpyAsync(dot, c->dot + first_row * c->n_b, cells * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (min_sum) HIPCHK(ctx, hipMemcpyAsync(min_sum, c->msum + first_row * c->n_b, cells * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BSK_OK;
}
