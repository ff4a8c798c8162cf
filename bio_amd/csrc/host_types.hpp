// host_types.hpp -- host-side objects behind the opaque handles of include/biosketch.h, shared by the translation units
// of libbiosketch.so (biosketch.hip: batches, dispatch; sets.hip: sorted unique hash sets).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <new>
#include <string>
#include <vector>

#include "biosketch.h"
#include "device_common.hpp"

// ------------------------------------------------------------------------------------
// Developer switches (DESIGN.md "Switches"): read from the environment ONCE, when the context is created, or again on
// bsk_ctx_reload_options (the test suite flips them inside one process) -- never on the bsk_sketch path.
struct BskOpts {
    u32 pk_tail = 1, pk_small = 3;  // k_minimizer_pk: the last pk_tail x (grid x 8) units of a launch of whole tickets go out as tickets of pk_small units (BSK_PK_TAIL, 0: none; BSK_PK_SMALL, 3..8)
    bool force_generic = false, no_mixed = false, no_dense = false, no_pk = false, no_ring = false, no_pkd = false, no_side_early = false, pk_no_uniform = false, no_side_dense = false, ring = false, no_bin = false, no_bin_early = false, compact = false, no_spare = false, no_tiles = false, no_tile_cache = false, no_tile_defer = false, tile_dense = false, no_group_gather = false, timing = false,
         no_fused_translate = false, sets_no_small = false;
    int syn_margin = 2;
    u32 test_overflow = 0;   // BSK_TEST_OVERFLOW (tests): pretend an overflow flag once per call -- 1: in a timed re-run (BSK_RESIZE), 2: a class plan's part while sizing, 4: ... in a timed re-run (BSK_REPLAN_CLASS)
    bool no_syn_long = false;
    u32 pf_density = 0;      // BSK_PF_DENSITY (tests): the expected selections per read up to which k_syncmer_pf / _pfl are planned (0: 86 % of what a unit's emit list holds per read -- 1 024 / 1 792 tuples per 64 reads; beyond the list the unit's last reads go to the exact machine)
    bool no_syn_pf = false;  // BSK_NO_SYN_PF: syncmers on k_syncmer_pk / _pkl also where the fused-emit kernel (k_syncmer_pf, round 6) is planned
    bool syn_sel = false;    // BSK_SYN_SEL (make EXPERIMENTS=1): the two-pass syncmer plan, measured and not planned (kernels_syncmer_sel.hpp)
    u32 nb_room = 0;         // BSK_NB_ROOM (tests): records bsk_sets_neighbors' first run has room for (0: CMP_NB_FIRST_ROOM, compare.hip) -- a case of a few tiles then reaches the second run
    u32 grid_cap = 0;        // BSK_GRID_CAP (tests): at most this many workgroups for every grid capped_grid sizes, on top of its own cap per CU (0: that cap alone) -- shapes of a few hundred sets then run every grid-stride loop's later trips
    u32 unit_grid = 0;       // BSK_UNIT_GRID (tests): at most this many workgroups for every grid unit_grid sizes -- the planned sketch kernels' persistent waves and the unit passes beside them (0: their own size) -- a batch of 83 units then gives every wave several tickets
    bool no_class = false;   // BSK_NO_CLASS: one plan per batch, keyed on the longest read (rounds 1-4)
    u32 class_min = 16384;   // BSK_CLASS_MIN: batches below this many reads keep one plan
    bool class_view = false;   // BSK_CLASS_VIEW: class plans always cut on the device (k_class_cut + a view of the batch), also where the host's list would do
    bool class_force = false;  // BSK_CLASS_FORCE: cut wherever the planner's choice changes, whatever the cost model says (tests: small batches)
    u32 wpr = 0, seg = 0, dense_min = 21 /* PlannerTable::dense_min */, ring_max = 0, ring_sel10 = 0 /* dev: ring_rows' selections per window x (w + 1), in tenths (0: PlannerTable::slab_sel_num) */, bin_min = 1024, waves_per_cu = 0, tile_min = 0, tile_pos = 0;  // tile_min 0: the kind's default
    void load();  // biosketch.hip
};

// The slots of the context's grow-only pool (bsk_ctx::tmp, taken through ctx_pool below).  A buffer lives from its first use to the end of
// the context; an entry that shares a slot with another says so here.  A new feature adds its own numbers before POOL_SLOTS (none is free).
enum PoolSlot {
    // 0-9 serve two users, each under its own names: a tiled call (tiles.hip) ...
    SLOT_TILE_START = 0, SLOT_TILE_DESC = 1, SLOT_TILE_ADESC = 2, SLOT_TILE_SEQ = 3, SLOT_TILE_SHIFT = 4, SLOT_TILE_KEEP = 5, SLOT_TILE_FLAGS = 6, SLOT_TILE_SEQ_FLAGS = 7,
    SLOT_TILE_SEQ_BAD = 8, SLOT_TILE_EXCL = 9,
    // ... and sets_build (sets.hip); SLOT_SETS_TMP is the sort's temporary storage, then the parts of the scan behind it
    SLOT_SETS_OFFS = 0, SLOT_SETS_PART = 1, SLOT_SETS_VALUES = 2, SLOT_SETS_UCOUNT = 3, SLOT_SETS_SORTED = 5, SLOT_SETS_HEAD = 6, SLOT_SETS_KEEP = 7, SLOT_SETS_POS = 8,
    SLOT_SETS_TMP = 9,
    // the containment search and bsk_hits_top, which runs when the search's temporaries are dead (search.hip)
    SLOT_SEARCH_QUERY = 10, SLOT_SEARCH_RANGES = 11, SLOT_SEARCH_STAGE = 15, SLOT_SEARCH_LARGE = 30, SLOT_SEARCH_SORT_TMP = 31,
    // bsk_result_fetch (biosketch.hip) AND bsk_result_fetch_narrow (sets.hip): the packed offsets, hashes and positions of one fetch
    SLOT_FETCH_OFFS = 12, SLOT_FETCH_HASH = 13, SLOT_FETCH_POS = 14,
    // bsk_result_compact (sets.hip): the arrays it hands to its caller
    SLOT_COMPACT_OFFS = 16,
    SLOT_SCAN_PART = 17,  // bsk_result_compact AND bsk_result_fetch_narrow: the parts of their offset scans (scratch, dead when either returns)
    SLOT_COMPACT_HASH = 18, SLOT_COMPACT_POS = 19,
    SLOT_NARROW_OFFS = 20,  // bsk_sets_fetch_narrow AND hits_fetch_narrow: u32 offsets between two synchronisations of the stream
    // class plans (classes.hip): the parts' lists of reads, the bulk's view, the parts' descriptors -- bsk_ctx::cls_owner says whose
    SLOT_CLASS_LISTS = 21, SLOT_CLASS_VIEW = 22, SLOT_CLASS_DESC = 23,
    // two-pass syncmers (launch.hip, make EXPERIMENTS=1)
    SLOT_SEL_MASK = 24, SLOT_SEL_CNT = 25, SLOT_SEL_UTOT = 26, SLOT_SEL_UBASE = 27,
    // the ASCII side launch's own reference words and status bytes (launch.hip)
    SLOT_SIDE_REFS = 28, SLOT_SIDE_STATUS = 29,
    // set operations (setops.hip): bsk_sets_op's pairs and tiles; bsk_sets_reduce's groups, sorted values, flags and sort storage
    SLOT_OP_PAIRS = 32, SLOT_OP_TILES = 33, SLOT_REDUCE_GROUPS = 34, SLOT_REDUCE_SORTED = 35, SLOT_REDUCE_VALUES = 36, SLOT_REDUCE_SORT_TMP = 37,
    // counted sets: sets_build's run lengths (sets.hip); the filter's flags; positions or count sums, and the scan behind them; the totals (counts.hip)
    SLOT_COUNT_RUNS = 40, SLOT_COUNT_KEEP = 41, SLOT_COUNT_POS = 42, SLOT_COUNT_SCAN = 43, SLOT_COUNT_OUT = 44,
    // all-pairs comparison: its figures; bottom-n: its scan (compare.hip)
    SLOT_COMPARE_FIGURES = 45, SLOT_BOTTOM_SCAN = 46,
    // sparse all-pairs comparison (compare.hip): figures, row counts and scan parts; the kept pairs' records; the sort's keys and storage
    SLOT_NB_ROWS = 38, SLOT_NB_RECORDS = 39, SLOT_NB_SORT = 47,
    // clusters of hits (cluster.hip): figures and per-node arrays; the hits' rows and the edges in rank space; the sorts' keys and storage
    SLOT_CLUSTER_NODES = 48, SLOT_CLUSTER_EDGES = 49, SLOT_CLUSTER_SORT = 50,
    // weighted sparse all-pairs comparison (compare.hip): the kept pairs' (dot, min_sum), slot for slot beside SLOT_NB_RECORDS
    SLOT_NB_WEIGHTS = 51,
    // window sets (windows.hip): the per-sequence window counts, lengths and offsets; the windows' spans, which sets_build reads as its source
    SLOT_WIN_SEQS = 52, SLOT_WIN_SPANS = 53,
    // folded hits (fold.hip): the target-to-group map; the group offsets, heads, runs and their scans
    SLOT_FOLD_MAP = 54, SLOT_FOLD_WORK = 55,
    // weighted containment search (search.hip): the payload pass's chunk offsets, scan parts and figures; the saturation bits of its hits
    SLOT_SW_QUERY = 56, SLOT_SW_FLAGS = 57,
    // hits selected by a measure (select.hip): figures, flags and scans; the norms of the call; the global sort path's hit indices
    SLOT_SELECT_WORK = 58, SLOT_SELECT_NORMS = 59, SLOT_SELECT_INDEX = 60,
    // hits by target (transpose.hip): the transpose's figure, sort keys and sort storage; the tally's figure
    SLOT_TRANSPOSE_WORK = 61, SLOT_TALLY_WORK = 62,
    // merged hits (merge.hip): the check's figures, the table of the parts, the summed offsets and the parts' places; the sort path's keys,
    // placed payloads, heads, scan and sort storage; the copies of parts that live on another device
    SLOT_MERGE_WORK = 63, SLOT_MERGE_SORT = 64, SLOT_MERGE_PEER = 65,
    POOL_SLOTS = 66
};

struct bsk_ctx {
    BskOpts opt;
    int device = 0;
    int cus = 0;
    mutable u64 grid_stats[2] = {};  // capped_grid: the launches it sized, and those whose cap left fewer workgroups than the work asked for (bsk_ctx_grid_stats)
    mutable u64 unit_grid_stats[2] = {};  // unit_grid: the grids it sized, and those BSK_UNIT_GRID left fewer workgroups than they asked for (bsk_ctx_unit_grid_stats)
    hipStream_t stream = nullptr;
    std::string err;
    // per-launch synchronisation scratch
    u32 *d_ticket = nullptr;    // [32]: 0..7 a launch's tickets and overflow flags, 8..15 class cuts' cursors, 16 the overflow flags of a class plan's PARTS (their own launches on the side context reset 0..7 one after another: k_fold_flags)
    u64 *d_total = nullptr;     // [1]
    u64 *d_lookback = nullptr;  // [lookback_cap]
    size_t lookback_cap = 0;
    u64 *d_ring_h = nullptr;  // runtime-w ring scratch
    u32 *d_ring_p = nullptr;
    size_t ring_cap = 0;  // entries
    static constexpr unsigned PINNED_WORDS = 8;
    u64 *h_pinned = nullptr;  // [PINNED_WORDS] pinned host words for small read-backs (read_back below)
    u8 *d_lut = nullptr;      // codon tables of `lut_table` (kernels_translate.hpp layout)
    int lut_table = 0;
    // grow-only temporaries of the entries (hipMalloc / hipFree of a tiled call's ten buffers cost more than its kernels)
    void *tmp[POOL_SLOTS] = {};  // one buffer per PoolSlot, taken through ctx_pool
    size_t tmp_cap[POOL_SLOTS] = {};
    u64 *h_refs = nullptr;   // pinned staging of bsk_result_fetch (refs down, offsets up), grow-only
    size_t h_refs_cap = 0;
    struct bsk_result *tile_res = nullptr;  // tile-level result of the previous tiled call, reused
    // Result arrays a released result leaves behind (biosketch.hip: spare_give / spare_take).  hipFree + hipMalloc of the arrays of a bench-size
    // result (10^8 reads: 32 GB) cost 1.2-3 s a call -- a hundred kernel times; a caller that releases every result and sketches the next
    // batch gets the last ones back instead.  Bounded (SPARE_SLOTS buffers, 40 % of the device memory), flushed when any allocation of the
    // library runs out of memory (host_internal.hpp: hipMalloc retries once after the flush) and with the context.
    static constexpr int SPARE_SLOTS = 8;
    struct Spare {
        void *p = nullptr;
        size_t bytes = 0;
    } spare[SPARE_SLOTS];
    size_t spare_bytes = 0, spare_limit = 0;
    // the one collective of the path (comm.cpp): an RCCL communicator over the GPUs that share a job
    void *comm = nullptr;  // ncclComm_t
    int comm_rank = 0, comm_world = 0;
    u64 *d_comm = nullptr;  // [(world + 1) * BSK_MAX_COUNTERS] device staging of bsk_gather_counts
    // class plans: the parts (the classes besides the bulk) run on a SIDE context -- a stream and scratch of their own -- so that their
    // small, latency-bound launches overlap with the bulk's kernel instead of queueing in front of it; two events order the two streams
    bsk_ctx *side = nullptr;              // created on first use, destroyed with this context
    hipEvent_t ev_side_done = nullptr, ev_adopted = nullptr, ev_mix0 = nullptr, ev_mix1 = nullptr, ev_tiled = nullptr;
    bool adopted_recorded = false;
    struct ClassSet *cls = nullptr;       // the class plan a run_planned / launch in progress belongs to (biosketch.hip: run_classed)
    bool no_side_fast = false;            // run_planned: a staged side kernel's region overflowed, plan the general one
    struct bsk_result *cls_owner = nullptr;  // the result whose class plan the pooled lists / views (SLOT_CLASS_*) currently describe
    u64 sel_need = 0;           // two-pass syncmers: the dense region a call that is being sized again needs (run_planned)
    bool no_syn_pk = false;     // set while a call falls back from k_syncmer_pk / k_minimizer_pk (the list of reads for the exact machine filled up)
    bool no_prot_fast = false;
    bool defer = false;         // run_planned: plan, size from the plan's own bounds, launch ONCE and read nothing back (sketch_tiled's path without host round trips: the caller looks at the flags behind its own last synchronisation)
    bool tile_sync = false;     // sketch_tiled: the round-trip path (tile count, sizing run and totals read on the host) -- set while a call falls back after the deferred path's flags showed an overflow
    bool tile_async = false;    // sketch_tiled on a class plan's side context: not even the last synchronisation -- totals stay on the device, the flags in d_ticket[24] (launch_parts folds them into the parent's)
    bool tile_was_async = false;  // ... what the last sketch_tiled on this context did
    bool in_resize = false;     // a timed call that outgrew its sized regions is being sized again (once per call: run_planned_resizing)
    int cls_round = 0;          // run_classed: which sizing round of the class plan is running (tests: BSK_TEST_OVERFLOW fires in round 0 only)
    bool part_grow = false;     // ... and a class plan's parts get twice their previous overflow regions (run_classed)
    bool no_dense = false;      // same for the dense-minimizer kernel (per-read slabs)  // set while a call falls back from the per-sequence-slab protein kernel
};

// Exact histogram of a batch's sequence lengths, built on the host where the batch is created (the lengths pass through the host there
// anyway): buckets of 16 bases below 1024, quarter octaves above.  What the per-length-class plans of biosketch.hip ("class plans") are
// cut from: which lengths occur, how many reads and bases each class holds -- without a device pass or a read-back.
struct LenHist {
    static constexpr int NB = 160;
    u64 cnt[NB] = {}, bases[NB] = {};
    u32 hi[NB] = {};  // the longest sequence of the bucket
    u32 lo[NB];       // ... and the shortest (valid where cnt != 0)
    LenHist() {
        for (int i = 0; i < NB; ++i) lo[i] = 0xffffffffu;
    }
    static int bucket(u64 L) {
        if (L < 1024) return (int)(L >> 4);
        const int lg = 63 - __builtin_clzll(L);  // >= 10
        return 64 + 4 * (lg - 10) + (int)((L >> (lg - 2)) & 3);
    }
    void add(u64 L) {
        const int i = bucket(L);
        cnt[i]++;
        bases[i] += L;
        if ((u32)L > hi[i]) hi[i] = (u32)L;
        if ((u32)L < lo[i]) lo[i] = (u32)L;
    }
};

struct bsk_batch {
    bsk_ctx *ctx = nullptr;
    int alphabet = BSK_ALPHA_DNA;
    int pairs = BSK_ALPHA_DNA;  // nucleotide batches: the alphabet whose PairLetter the two-strand k-mer mode applies (BSK_ALPHA_DNA = DNAredundant, 2..5)
    u64 n = 0, n_bases = 0, n_words = 0, n_nonacgt = 0;
    u32 maxlen = 0;
    u32 side_maxlen = 0;   // class views: the longest read of the WHOLE batch (the ASCII side launch covers every flagged read, whatever its class); 0: maxlen
    u32 uniform_len = 0;  // != 0: every read has this length (synthetic batches)
    u32 word_stride = 0;  // != 0: ... the batch is DNA and read r starts at word r * word_stride (= words per read): k_minimizer_pk needs no descriptors
    u32 *words = nullptr;
    u64 *desc = nullptr;   // NULL when a sequence has 2^24 bases or more: fw + llen then locate the sequences (tiled runs only)
    u64 *fw = nullptr;     // [n] first word
    u64 *llen = nullptr;   // [n] bases
    u64 *adesc = nullptr;  // tile batches over ASCII: (first_byte << 24) | n_bases per tile
    bool alias = false;    // words / ascii belong to another batch (tile batches)
    bool borrowed = false; // a VIEW of another batch (class plans): nothing but desc / bdesc / bflags / adesc is its own
    LenHist *hist = nullptr;  // DNA batches of varying length created from host data; NULL: unknown (synthetic, tiles, translated)
    // ... and, when at most a twentieth of the sequences lie outside the histogram's fullest bucket, those sequences: (index << 32) | bases,
    // ascending.  A class plan whose bulk holds that bucket then needs NO device pass to cut the batch: the other classes' lists are picked
    // from here on the host and the bulk's kernel masks by length itself (KArgs::cls_*).
    std::vector<u64> *odd = nullptr;
    u64 *d_odd = nullptr;  // the same list on the device (lists of 65 536 and more: class plans split them there)
    int modal_bucket = -1;
    u32 *wbits = nullptr;  // one bit per packed word: the word holds a non-ACGT letter (batches that may be tiled)
    u32 *subset = nullptr; // reads with a non-ACGT letter, ascending (side launch of the ASCII kernels); nsub = n_nonacgt
    u64 nsub = 0;
    u8 *rflags = nullptr;
    // length-binned view of desc / rflags (ensure_binned, planner.hip): built on the first sketch call that plans it, kept with the batch
    mutable u64 *bdesc = nullptr;
    mutable u8 *bflags = nullptr;
    mutable u32 bin_gran = 0, bin_lo = 0;  // bases per length class (above bin_lo) the view was built with (0: not built)
    mutable bool bin_early = false;        // the view was built with the batch (bin_with_batch, biosketch.hip): classes finer than any plan's, no pass per plan
    mutable size_t c_bdesc = 0, c_bflags = 0;
    u8 *ascii = nullptr;  // DNA: kept only when some read has a non-ACGT byte; protein: always
    u64 *aoff = nullptr;
    u64 device_bytes = 0;
    // capacities (bytes) of the device buffers, and the ASCII buffers parked while a batch is pure ACGT: a streaming caller
    // re-fills one batch object per stream (bsk_batch_refill_ascii) instead of allocating per chunk -- hipFree synchronises the
    // whole device and would serialise the streams
    size_t c_words = 0, c_desc = 0, c_rflags = 0, c_ascii = 0, c_aoff = 0;
    u8 *spare_ascii = nullptr;
    u64 *spare_aoff = nullptr;
};

struct ClassSet;  // biosketch.hip: the parts of a class plan (sub-batches, their results, the lists of their reads)
struct bsk_result {
    bsk_ctx *ctx = nullptr;
    u64 n = 0, cap = 0, n_tuples = 0;
    u64 alloc_cap = 0;  // tuples hash[] / pos[] were allocated for: cap + tail_cap
    u64 tail_cap = 0;   // class plans: tuples behind `cap` that hold the adopted parts' slabs
    bool arrays_borrowed = false;  // hash / pos point into another result's tail (a part of a class plan)
    ClassSet *classes = nullptr;   // class plan of the last sizing call (owned)
    u64 n_cap = 0;  // reads the refs / status arrays were allocated for
    u64 ovf_cap = 0;  // slab kernels: tuples reserved (inside cap) for units that outgrow their slab
    u64 main_cap = 0; // tuples [0, main_cap) belong to the main launch, [main_cap, cap) to the side launch (mixed batches)
    int kind = 0, has_pos = 0;
    u64 *refs = nullptr;  // per read: (first_tuple << 24) | n_tuples ; NULL for wide results
    u64 *wfirst = nullptr, *wcount = nullptr;  // wide results (tiled long sequences): first tuple and tuple count per sequence
    u8 *status = nullptr;
    u64 *hash = nullptr;
    u32 *pos = nullptr;
    char plan[320] = "";   // what ran: kernel name of the last launch into this result (bsk_result_plan)
    int plan_grid = 0, plan_per_cu = 0;
    // The plan the arrays were SIZED for (run_planned, launch.hip): bsk_sketch_timed on an existing result repeats exactly this plan --
    // a fresh plan could want more rows per unit than `cap` holds (k_minimizer_ring after a fall-back to 32-row slabs) and write past it.
    bool plan_valid = false;
    bool unit_rows = false;  // the last launch wrote unit rows (BSK_REF_ROWS: k_minimizer_ring): what the group gathers of sets.hip dispatch on
    u64 plan_n = 0, plan_bases = 0;
    u32 plan_maxlen = 0;
    int plan_circ = 0;
    bsk_params plan_params = {};
    alignas(8) unsigned char plan_blob[192] = {};
};

static inline int fail_hip(bsk_ctx *ctx, hipError_t e, const char *what) {
    if (ctx) {
        char buf[512];
        snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
        ctx->err = buf;
    }
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? BSK_ERR_NOMEM : BSK_ERR_DEVICE;
}
static inline int fail_arg(bsk_ctx *ctx, const char *what) {
    if (ctx) ctx->err = what;
    return BSK_ERR_ARG;
}
#define HIPCHK(ctx, call)                                        \
    do {                                                         \
        hipError_t e__ = (call);                                 \
        if (e__ != hipSuccess) return fail_hip(ctx, e__, #call); \
    } while (0)

// The one place a capped grid is sized: every launch of the sets side and the small passes around a sketch call (the two grid_for, the
// tile grids of compare.hip, bsk_hits_top's wave budget) -- the grids of the planned sketch kernels themselves do not come here and keep
// ctx->cus.  grid_cap_blocks: the most workgroups such a launch gets, `per_cu` per CU and, with BSK_GRID_CAP, no more than that.  capped_grid: `want` workgroups under that
// cap, at least one; the kernels behind it cover the rest in a grid-stride loop and none of them waits for another workgroup.
static inline u64 grid_cap_blocks(const bsk_ctx *ctx, u64 per_cu) {
    const u64 own = (u64)ctx->cus * per_cu;
    return ctx->opt.grid_cap ? std::min<u64>(ctx->opt.grid_cap, own) : own;
}
static inline unsigned capped_grid(const bsk_ctx *ctx, u64 want, u64 per_cu) {
    const u64 g = std::max<u64>(1, std::min<u64>(want, grid_cap_blocks(ctx, per_cu)));
    ++ctx->grid_stats[0];
    if (g < want) ++ctx->grid_stats[1];
    return (unsigned)g;
}
// The grids capped_grid leaves alone -- the persistent waves of a planned sketch kernel (pl.grid, pl.side_grid, the tile unit kernels through
// them) and the unit passes k_tile_count, k_bin_desc, k_class_cut, k_two_strand: `want` workgroups as the caller sized them, or, with
// BSK_UNIT_GRID=N (tests), at most N.  Never more than `want`; unset, `want` itself.  Counters of its own (bsk_ctx_unit_grid_stats): capped_grid's are
// held to exact figures.  NOT for a launch whose kernel takes its units from eight ticket heads and looks back over them (k_translate,
// k_compact_flags, k_tile_stitch, k_minimizer_pft: device_common.hpp, "tickets from eight heads"): head x hands out the units x, x + 8, ...
// and a wave starts on its own XCD's head, so with fewer waves than XCDs a wave can wait for a unit nobody has taken.  The kernels behind
// this helper take tickets from ONE word (next_ticket) and walk a ticket's units upward: a unit only waits for units that run or are done.
static inline unsigned unit_grid(const bsk_ctx *ctx, u64 want) {
    const u64 g = ctx->opt.unit_grid ? std::max<u64>(1, std::min<u64>(want, ctx->opt.unit_grid)) : want;
    ++ctx->unit_grid_stats[0];
    if (g < want) ++ctx->unit_grid_stats[1];
    return (unsigned)g;
}
int grid_for(bsk_ctx *ctx, u64 items, int block) __attribute__((visibility("hidden")));  // biosketch.hip: workgroups of `block` items, at most 16 per CU
bool spare_flush_all() __attribute__((visibility("hidden")));  // biosketch.hip
// Every device allocation of the library's host code (this header is in all of its translation units): when the device is out of memory, what the contexts keep in reserve (released
// results' arrays) goes back first, then the allocation is tried once more.
static inline hipError_t bsk_malloc_retry(void **p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory && spare_flush_all()) {
        (void)hipGetLastError();
        e = hipMalloc(p, bytes);
    }
    return e;
}
#define hipMalloc(ptr, bytes) bsk_malloc_retry((void **)(ptr), (bytes))

// The library's one grow-only allocator (below the macro: it flushes and retries like every other allocation).  A buffer is kept while it
// holds `bytes` and exists -- so a request of no bytes still yields a pointer -- and is otherwise freed BEFORE its successor is allocated
// (the peak stays one buffer), with a quarter and 256 bytes of slack so that a slowly growing caller settles.  hipMalloc / hipFree
// synchronise the whole device and cost more than the kernels of a small call: in steady state neither runs.
// An object's own array: *cap is what *p holds, in bytes.  slack == false: exactly `bytes` (an object made for one call).  On failure the
// array is gone (*p NULL, *cap 0).  Out of line: the library has some ninety call sites and none of them is hot.
template <class T>
static inline __attribute__((noinline)) hipError_t grow_array(T **p, size_t *cap, size_t bytes, bool slack = true) {
    if (*cap >= bytes && *p) return hipSuccess;
    (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const size_t want = slack ? bytes + bytes / 4 + 256 : bytes;
    const hipError_t e = hipMalloc(p, want);
    if (e == hipSuccess) *cap = want;
    return e;
}
// Slot `slot` of the context's pool, at least `bytes` big.
template <class T>
static inline hipError_t ctx_pool(bsk_ctx *ctx, PoolSlot slot, size_t bytes, T **out) {
    const hipError_t e = grow_array(&ctx->tmp[slot], &ctx->tmp_cap[slot], bytes);
    *out = static_cast<T *>(ctx->tmp[slot]);
    return e;
}

// A few device totals to the host: `n_words` u64 from `dev` to ctx->h_pinned[at ..] on the context's stream, then the synchronisation.  The
// caller reads ctx->h_pinned[at .. at + n_words) when this returns hipSuccess.
static inline hipError_t read_back(bsk_ctx *ctx, const u64 *dev, unsigned n_words, unsigned at = 0) {
    if (at + n_words > bsk_ctx::PINNED_WORDS) return hipErrorInvalidValue;
    const hipError_t e = hipMemcpyAsync(ctx->h_pinned + at, dev, n_words * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(ctx->stream);
}

// The in/out object slot of an entry (bsk_sets **out, bsk_hits **hits, bsk_compare **cmp): NULL, or an earlier result to re-use.  The
// object is taken over for the call -- the slot is NULL while `run(res, reused)` works on it -- released when run fails, and stored back
// when it returns BSK_OK.  What an entry checks BEFORE it calls this leaves the slot as it was; what it checks inside `run` releases a
// re-used object (include/biosketch.h "The result slot" says which entry does which).
template <class T, class F>
static inline int take_over(bsk_ctx *ctx, T **slot, void (*release)(T *), F run) {
    T *res = *slot;
    *slot = nullptr;
    const bool reused = res != nullptr;
    if (!res) res = new (std::nothrow) T();
    if (!res) return BSK_ERR_NOMEM;
    res->ctx = ctx;
    const int rc = run(res, reused);
    if (rc != BSK_OK) {
        release(res);
        return rc;
    }
    *slot = res;
    return BSK_OK;
}
