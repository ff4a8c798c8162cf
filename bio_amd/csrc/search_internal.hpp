// search_internal.hpp -- what search.hip shares with pipeline.cpp (the hits sink).  Nothing here crosses the C ABI.
#pragma once
#include <cstdint>

#include "biosketch.h"

// All hits of h to the host in the narrow form of a pipeline chunk: u32 offsets[n_queries + 1] (narrowed on the device, as
// bsk_sets_fetch_narrow narrows a set's), target[] and shared[], copied on the context's stream -- 4 bytes per query + 8 per hit over
// the link.  BSK_ERR_UNSUPPORTED when h holds 2^32 hits or more (the caller takes bsk_hits_fetch).
int hits_fetch_narrow(bsk_ctx *ctx, const bsk_hits *h, uint32_t *offsets, uint32_t *target, uint32_t *shared, uint64_t hit_cap)
    __attribute__((visibility("hidden")));
