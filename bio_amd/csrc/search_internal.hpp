// search_internal.hpp -- what search.hip shares with pipeline.cpp (the hits sink) and compare.hip (bsk_sets_neighbors fills a bsk_hits).
// Nothing here crosses the C ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#include "biosketch.h"
#include "device_common.hpp"

struct bsk_hits {
    bsk_ctx *ctx = nullptr;
    u64 n_queries = 0, n_hits = 0, n_large = 0;
    u64 *offsets = nullptr;  // [n_queries + 1]
    u32 *target = nullptr, *shared = nullptr;
    size_t c_offsets = 0, c_target = 0, c_shared = 0;  // bytes allocated (grow-only when the object is re-used)
    char plan[256] = "";
    // hits with totals (compare.hip: bsk_sets_neighbors): total[i] = the values walked for hit i.  `has_total` says whether the array is
    // valid: every entry that writes hits into this object without totals clears it and keeps the array (grow-only, like the others).
    u32 *total = nullptr;  // [n_hits]
    size_t c_total = 0;
    bool has_total = false;
    // hits with weights (compare.hip: bsk_sets_neighbors_counted; search.hip: bsk_index_search_counted): dot[i] and msum[i] of hit i, as the
    // cells of bsk_sets_compare_counted.
    // `has_weights` follows the rule of `has_total`: whoever clears that clears this, and the arrays stay.
    u64 *dot = nullptr, *msum = nullptr;  // [n_hits]
    size_t c_dot = 0, c_msum = 0;
    bool has_weights = false;
    // folded hits (fold.hip: bsk_hits_fold): members[i] = how many targets of hit i's group the row hit.  `has_members` follows the rule of
    // `has_total` too: whoever clears that clears this, and the array stays.
    u32 *members = nullptr;  // [n_hits]
    size_t c_members = 0;
    bool has_members = false;
};

// clusters of a hits graph (cluster.hip: bsk_hits_cluster)
struct bsk_clusters {
    bsk_ctx *ctx = nullptr;
    u64 n = 0, n_clusters = 0, largest = 0, rounds = 0, edges = 0;
    u32 *label = nullptr;    // [n]
    u32 *rep = nullptr;      // [n_clusters] ascending
    u64 *offsets = nullptr;  // [n_clusters + 1]
    u32 *members = nullptr;  // [n] ascending inside a cluster
    size_t c_label = 0, c_rep = 0, c_offsets = 0, c_members = 0;  // bytes allocated (grow-only when the object is re-used)
    char plan[128] = "";
};

// All hits of h to the host in the narrow form of a pipeline chunk: u32 offsets[n_queries + 1] (narrowed on the device, as
// bsk_sets_fetch_narrow narrows a set's), target[] and shared[], copied on the context's stream -- 4 bytes per query + 8 per hit over
// the link.  BSK_ERR_UNSUPPORTED when h holds 2^32 hits or more (the caller takes bsk_hits_fetch).
int hits_fetch_narrow(bsk_ctx *ctx, const bsk_hits *h, uint32_t *offsets, uint32_t *target, uint32_t *shared, uint64_t hit_cap)
    __attribute__((visibility("hidden")));
