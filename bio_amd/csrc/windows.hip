// windows.hip -- window sets (include/biosketch.h "window sets and folded hits"): one set per window of a sequence's positions, the form
// in which kmcp indexes a reference (one k-mer set per chunk), made where the tuples already are.
//
// A sequence's tuples are stored in position order (include/biosketch.h, bsk_sketch: "in position order" -- unit rows with stride 64,
// the tails of class plans and the stitched tuples of a tiled call alike), so window w of a sequence -- the tuples with
// w*S <= p < w*S + W -- is a contiguous span (first tuple, count, stride) of them.  That is what a reference word or a wfirst / wcount
// pair already describes, so the windows become the span source of sets_build_spans (sets.hip) and everything behind the spans -- the
// small-set kernel, the segmented sort, the FracMinHash filter, the run lengths -- is the code bsk_result_sets runs.  Spans of
// overlapping windows overlap; nothing in that path minds.
//
//   k_win_count   a lane per sequence: the last tuple's position P -> nwin (and, in count mode, the sequence's own W)
//   scan_counts   over nwin -> seq_offsets[n + 1] and the number of windows
//   k_win_spans   a lane per window, neighbouring lanes neighbouring windows (their searches walk the same lines of the L2): the
//                 sequence by a search in seq_offsets, the span by two lower-bound searches over the sequence's strided pos[] -- or by
//                 arithmetic for the kinds with implicit positions.  Packed results keep packed words (the row stride survives in bit
//                 63), wide results the wide pair.
// Integers only, bounded loops, no kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "biosketch.h"
#include "host_types.hpp"
#include "sets_internal.hpp"

#define WIN_BLOCK 256

namespace {

struct WinRule {
    u32 window, step, count;  // count != 0: W per sequence, S = W
};

// first tuple, count and stride of sequence r
__device__ __forceinline__ void win_seq(const u64 *refs, const u64 *wfirst, const u64 *wcount, u64 r, u64 &first, u64 &cnt, u64 &stride) {
    if (refs) {
        first = BSK_REF_FIRST(refs[r]);
        cnt = BSK_REF_COUNT(refs[r]);
        stride = BSK_REF_STRIDE(refs[r]);
    } else {
        first = wfirst[r];
        cnt = wcount[r];
        stride = 1;
    }
}

__global__ __launch_bounds__(WIN_BLOCK) void k_win_count(const u32 *pos, const u64 *refs, const u64 *wfirst, const u64 *wcount, u64 n, WinRule rule, u64 *nwin, u32 *wlen) {
    for (u64 r = (u64)blockIdx.x * WIN_BLOCK + threadIdx.x; r < n; r += (u64)gridDim.x * WIN_BLOCK) {
        u64 first, c, stride;
        win_seq(refs, wfirst, wcount, r, first, c, stride);
        u64 nw = 0, W = rule.window;
        if (c) {
            const u64 P = pos ? (u64)(pos[first + (c - 1) * stride] & BSK_POS_MASK) : c - 1;
            if (rule.count) W = (P + rule.count) / rule.count;  // ceil((P + 1) / count), which is >= 1
            const u64 S = rule.count ? W : (rule.step ? rule.step : rule.window);
            nw = (P < W ? 0 : (P - W) / S + 1) + 1;
        }
        nwin[r] = nw;
        wlen[r] = (u32)W;  // (P < 2^31, so W fits)
    }
}

// the first tuple t in [0, c) of the sequence whose position is >= key (c when there is none); 64 halvings cover any count
__device__ __forceinline__ u64 win_lower(const u32 *pos, u64 first, u64 stride, u64 c, u64 key) {
    u64 lo = 0, hi = c;
    for (int it = 0; it < 64 && lo < hi; ++it) {
        const u64 mid = (lo + hi) >> 1;
        if ((u64)(pos[first + mid * stride] & BSK_POS_MASK) < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(WIN_BLOCK) void k_win_spans(const u32 *pos, const u64 *refs, const u64 *wfirst, const u64 *wcount, u64 n, WinRule rule, const u64 *seq_off,
                                                          const u32 *wlen, u64 nw, u64 *orefs, u64 *ofirst, u64 *ocount) {
    for (u64 i = (u64)blockIdx.x * WIN_BLOCK + threadIdx.x; i < nw; i += (u64)gridDim.x * WIN_BLOCK) {
        // the sequence of window i: the last r with seq_off[r] <= i (seq_off[0] = 0 <= i < seq_off[n]; sequences without windows are passed over)
        u64 lo = 0, hi = n;
        for (int it = 0; it < 64 && hi - lo > 1; ++it) {
            const u64 mid = (lo + hi) >> 1;
            if (seq_off[mid] <= i) lo = mid;
            else hi = mid;
        }
        const u64 r = lo, w = i - seq_off[r];
        u64 first, c, stride;
        win_seq(refs, wfirst, wcount, r, first, c, stride);
        const u64 W = rule.count ? wlen[r] : rule.window, S = rule.count ? W : (rule.step ? rule.step : rule.window);
        const u64 p0 = w * S, p1 = p0 + W;  // (w < 2^32, S and W < 2^31: no overflow)
        const u64 a = pos ? win_lower(pos, first, stride, c, p0) : (p0 < c ? p0 : c);
        const u64 b = pos ? win_lower(pos, first, stride, c, p1) : (p1 < c ? p1 : c);
        if (orefs) {
            orefs[i] = ((first + a * stride) << 24) | (b - a) | (stride > 1 ? BSK_REF_ROWS : 0);
        } else {
            ofirst[i] = first + a;
            ocount[i] = b - a;
        }
    }
}

int windows_impl(bsk_ctx *ctx, const bsk_result *r, const WinRule &rule, int scale, bool counted, uint64_t *seq_offsets, bsk_sets *res, bool reused) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u64 n = r->n;
    // per sequence: nwin, W, seq_offsets and the scan's parts; two totals
    Carve cs;
    const size_t o_tot = cs.add<u64>(2), o_nwin = cs.add<u64>(n), o_off = cs.add<u64>(n + 1), o_part = cs.add<u64>(scan_parts(n)), o_wlen = cs.add<u32>(n);
    void *bs = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_WIN_SEQS, cs.bytes, &bs));
    u64 *tot = at<u64>(bs, o_tot), *nwin = at<u64>(bs, o_nwin), *seq_off = at<u64>(bs, o_off), *part = at<u64>(bs, o_part);
    u32 *wlen = at<u32>(bs, o_wlen);
    HIPCHK(ctx, hipMemsetAsync(tot, 0, 16, st));
    if (n) {
        hipLaunchKernelGGL(k_win_count, dim3(grid_for(ctx, n, WIN_BLOCK, 16)), dim3(WIN_BLOCK), 0, st, (const u32 *)r->pos, (const u64 *)r->refs, (const u64 *)r->wfirst,
                           (const u64 *)r->wcount, n, rule, nwin, wlen);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, scan_counts(st, ArrayOf{nwin}, n, part, seq_off, tot, (u64 *)nullptr));
    HIPCHK(ctx, read_back(ctx, tot, 1));
    const u64 NW = ctx->h_pinned[0];
    if (NW >= (1ULL << 32)) {
        ctx->err = "bsk_result_sets_windows: 2^32 windows or more in one call (split the batch or widen the window)";
        return BSK_ERR_UNSUPPORTED;
    }
    if (seq_offsets) HIPCHK(ctx, hipMemcpyAsync(seq_offsets, seq_off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    // the windows' spans, in the result's own form
    const bool packed = r->refs != nullptr;
    Carve cw;
    const size_t o_a = cw.add<u64>(NW), o_b = cw.add<u64>(packed ? 0 : NW);
    void *bw = nullptr;
    HIPCHK(ctx, ctx_pool(ctx, SLOT_WIN_SPANS, cw.bytes, &bw));
    u64 *sa = at<u64>(bw, o_a), *sb = at<u64>(bw, o_b);
    if (NW) {
        hipLaunchKernelGGL(k_win_spans, dim3(grid_for(ctx, NW, WIN_BLOCK, 16)), dim3(WIN_BLOCK), 0, st, (const u32 *)r->pos, (const u64 *)r->refs, (const u64 *)r->wfirst,
                           (const u64 *)r->wcount, n, rule, (const u64 *)seq_off, (const u32 *)wlen, NW, packed ? sa : nullptr, packed ? nullptr : sa, packed ? nullptr : sb);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(st));  // (seq_offsets is the caller's from here; sets_build_spans re-uses the stream)
    const SpanSrc src{r->hash, packed ? sa : nullptr, packed ? nullptr : sa, packed ? nullptr : sb, NW, "bsk_result_sets_windows"};
    return sets_build_spans(ctx, src, BSK_SETS_PER_SEQUENCE, scale, counted, res, reused);
}

}  // namespace

extern "C" int bsk_result_sets_windows(bsk_ctx *ctx, const bsk_result *r, const bsk_window_params *wp, int scale, bsk_sets **sets, uint64_t *seq_offsets) {
    if (!ctx || !r || !wp || !sets) return fail_arg(ctx, "bsk_result_sets_windows: null argument");
    if ((wp->window != 0) == (wp->count != 0)) return fail_arg(ctx, "bsk_result_sets_windows: exactly one of window and count must be set");
    if (wp->step > wp->window) return fail_arg(ctx, wp->count ? "bsk_result_sets_windows: step set in count mode" : "bsk_result_sets_windows: step > window");
    if (wp->window >= (1u << 31)) return fail_arg(ctx, "bsk_result_sets_windows: window >= 2^31");
    if (wp->flags & ~(uint32_t)BSK_WINDOWS_COUNTED) return fail_arg(ctx, "bsk_result_sets_windows: unknown flag");
    if (scale < 0) return fail_arg(ctx, "bsk_result_sets_windows: bad scale");
    if (r->ctx != ctx || (*sets && (*sets)->ctx != ctx)) return fail_arg(ctx, "bsk_result_sets_windows: the result or the sets belong to another context");
    const WinRule rule{wp->window, wp->step, wp->count};
    const bool counted = (wp->flags & BSK_WINDOWS_COUNTED) != 0;
    return take_over(ctx, sets, bsk_sets_release, [&](bsk_sets *res, bool reused) { return windows_impl(ctx, r, rule, scale, counted, seq_offsets, res, reused); });
}
