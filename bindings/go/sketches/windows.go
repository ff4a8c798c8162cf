//go:build biosketch

package sketches

/*
#cgo LDFLAGS: -lbiosketch
#include <stdlib.h>
#include "biosketch.h"
*/
import "C"

import (
	"errors"
	"runtime"
	"unsafe"
)

// ---- window sets and folded hits: genome chunks as search targets ---------------------------------------------------------
//
// chunks, starts, _ := res.WindowSets(WindowParams{Count: 10}, 1, nil) makes one set per chunk of every genome (kmcp's
// --split-number); an index of them is searched with the reads' sets, and hits.Fold(starts, FoldParams{FracNum: 8, FracDen: 10}, nil)
// sums the hits per genome and keeps the genomes of which the read set hit at least 80 % of the chunks.  Nothing leaves the device
// but the offsets.

// WindowParams is bsk_window_params: Window positions per window whose starts are Step apart (0: no overlap), or Count windows per
// sequence, sized per sequence.  Counted: every value with its run length inside the window.
type WindowParams struct {
	Window, Step, Count uint32
	Counted             bool
}

// WindowSets makes one set per window of every sequence's positions (bsk_result_sets_windows).  seqOffsets[i] is the set of
// window 0 of sequence i, seqOffsets[n] the number of sets: the group offsets (*Sets).Reduce and (*Hits).Fold take.  into: nil, or a
// Sets of this engine whose device arrays are kept and only grow.
func (r *DeviceResult) WindowSets(p WindowParams, scale int, into *Sets) (sets *Sets, seqOffsets []uint64, err error) {
	if into == nil {
		into = &Sets{eng: r.eng}
		runtime.SetFinalizer(into, func(s *Sets) { C.bsk_sets_release(s.h) })
	}
	var n C.uint64_t
	C.bsk_result_info(r.h, &n, nil, nil)
	seqOffsets = make([]uint64, uint64(n)+1)
	wp := C.bsk_window_params{window: C.uint32_t(p.Window), step: C.uint32_t(p.Step), count: C.uint32_t(p.Count)}
	if p.Counted {
		wp.flags = C.BSK_WINDOWS_COUNTED
	}
	rc := C.bsk_result_sets_windows(r.eng.ctx, r.h, &wp, C.int(scale), &into.h, (*C.uint64_t)(unsafe.Pointer(&seqOffsets[0])))
	runtime.KeepAlive(r)
	return into, seqOffsets, r.eng.err(rc)
}

// FoldParams is bsk_fold_params: keep a group only if at least MinMembers of its targets were hit (0 is taken as 1) and, with
// FracDen != 0, members * FracDen >= FracNum * the group's size.
type FoldParams struct {
	MinMembers, FracNum, FracDen uint32
}

// Fold sums the hits by target group (bsk_hits_fold): group g is targets groupOffsets[g] .. groupOffsets[g+1]-1.  The result has
// the rows of h, one hit per group with a hit target that passes p: its target is g, its shared count the saturating sum, and
// Members / FetchMembers tell how many of the group's targets the row hit.  The rows of h must list their targets strictly
// ascending (not the output of Top).  reuse: nil, or any Hits of this engine but h.
func (h *Hits) Fold(groupOffsets []uint64, p FoldParams, reuse *Hits) (*Hits, error) {
	if len(groupOffsets) == 0 {
		return nil, errors.New("Fold: groupOffsets must have n+1 entries")
	}
	if reuse == nil {
		reuse = &Hits{eng: h.eng}
		runtime.SetFinalizer(reuse, func(r *Hits) { C.bsk_hits_release(r.h) })
	}
	fp := C.bsk_fold_params{min_members: C.uint32_t(p.MinMembers), frac_num: C.uint32_t(p.FracNum), frac_den: C.uint32_t(p.FracDen)}
	rc := C.bsk_hits_fold(h.eng.ctx, h.h, (*C.uint64_t)(unsafe.Pointer(&groupOffsets[0])), C.uint64_t(len(groupOffsets)-1), &fp, &reuse.h)
	runtime.KeepAlive(h)
	runtime.KeepAlive(groupOffsets)
	return reuse, h.eng.err(rc)
}

// Members is the device array members[hits] of folded hits, nil for hits without members (bsk_hits_members_device).
func (h *Hits) Members() unsafe.Pointer {
	var m *C.uint32_t
	C.bsk_hits_members_device(h.h, &m)
	runtime.KeepAlive(h)
	return unsafe.Pointer(m)
}

// FetchMembers copies the members of every hit to the host (bsk_hits_fetch_members); hits without members are an error.
func (h *Hits) FetchMembers() ([]uint32, error) {
	nq, nh := h.Info()
	members := make([]uint32, nh+1)
	rc := C.bsk_hits_fetch_members(h.eng.ctx, h.h, 0, C.uint64_t(nq), (*C.uint32_t)(unsafe.Pointer(&members[0])), C.uint64_t(nh+1))
	runtime.KeepAlive(h)
	return members[:nh], h.eng.err(rc)
}
