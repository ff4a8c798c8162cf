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

// ---- merged hits: a database split over many indexes -------------------------------------------------------------------------------
//
// Shards by target: search every shard's index, then all, _ := MergeHits(e, parts, base, false, nil) with base[p] the targets before
// shard p -- a row of the result is the union of the parts' rows.  Shards by value (every shard holds all targets and a range of the
// hash space): search every shard with MinShared 1, MergeHits(e, parts, nil, true, nil) adds a pair's integers up, then
// Filter(Measure{Kind: MeasureShared}, m, 1, nil) applies the threshold to the sums.

// MergeHits makes one Hits out of the hits of several searches of the same queries (bsk_hits_merge): row q holds every hit of row q of
// every part with base[p] added to its target (base nil: all 0), strictly ascending, with every payload all parts carry.  A pair that
// occurs twice is an error unless add is set; then its fields are summed, saturating.  The parts may belong to other engines, on this
// device or another; at most 64 parts.  into: nil, or any Hits of e that is not one of the parts.
func MergeHits(e *Engine, parts []*Hits, base []uint64, add bool, into *Hits) (*Hits, error) {
	if len(parts) == 0 || (base != nil && len(base) != len(parts)) {
		return into, errors.New("sketches: MergeHits needs at least one part and one base per part")
	}
	if into == nil {
		into = &Hits{eng: e}
		runtime.SetFinalizer(into, func(r *Hits) { C.bsk_hits_release(r.h) })
	}
	hs := make([]*C.bsk_hits, len(parts)) // (C pointers: the slice holds no Go pointer)
	for i, p := range parts {
		if p != nil {
			hs[i] = p.h
		}
	}
	var bp *C.uint64_t
	if base != nil {
		bp = (*C.uint64_t)(unsafe.Pointer(&base[0]))
	}
	flags := C.uint32_t(0)
	if add {
		flags = C.uint32_t(C.BSK_MERGE_ADD)
	}
	rc := C.bsk_hits_merge(e.ctx, (**C.bsk_hits)(unsafe.Pointer(&hs[0])), bp, C.uint32_t(len(parts)), flags, &into.h)
	runtime.KeepAlive(parts)
	runtime.KeepAlive(base)
	return into, e.err(rc)
}
