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

// ---- counted sets: values with their abundance, on the device -----------------------------------------------------------
//
// A counted Sets carries counts[i] for values[i]: how often the value occurred in its scope.  k-mer counting is CountedSets
// over the whole batch, error removal FilterCounts(2, ...), a sample's weighted containment in every genome
// sample.OpCounted(genomes, CountKeep, nil) followed by Totals.  Every other method treats a counted Sets as its values.

// CountOp names the operation of (*Sets).OpCounted.
type CountOp int

const (
	CountAdd  CountOp = C.BSK_COUNTOP_ADD  // the union's values, counts added (saturating at 2^32-1)
	CountKeep CountOp = C.BSK_COUNTOP_KEEP // a's values that b holds, with a's counts
	CountDrop CountOp = C.BSK_COUNTOP_DROP // a's values that b does not hold, with a's counts
)

// CountedSets reduces the result to per-record (or whole-batch) sets with counts into s (nil the first time):
// bsk_result_sets_counted -- the device arrays of s are kept and only grow.
func (r *DeviceResult) CountedSets(s *Sets, wholeBatch bool, scale int) (*Sets, error) {
	if s == nil {
		s = &Sets{eng: r.eng}
		runtime.SetFinalizer(s, func(s *Sets) { C.bsk_sets_release(s.h) })
	}
	scope := C.int(C.BSK_SETS_PER_SEQUENCE)
	if wholeBatch {
		scope = C.int(C.BSK_SETS_WHOLE_BATCH)
	}
	rc := C.bsk_result_sets_counted(r.eng.ctx, r.h, scope, C.int(scale), &s.h)
	runtime.KeepAlive(r)
	return s, r.eng.err(rc)
}

// Counted reports whether s carries counts, and where they are on the device (bsk_sets_counts_device; nil for plain sets).
func (s *Sets) Counted() (bool, unsafe.Pointer) {
	var c *C.uint32_t
	C.bsk_sets_counts_device(s.h, &c)
	runtime.KeepAlive(s)
	return c != nil, unsafe.Pointer(c)
}

// Counts copies the counts of all sets to the host, parallel to the values Fetch returns (bsk_sets_fetch_counts).
func (s *Sets) Counts() ([]uint32, error) {
	var nSets, nValues C.uint64_t
	C.bsk_sets_info(s.h, &nSets, &nValues)
	counts := make([]uint32, uint64(nValues)+1)
	rc := C.bsk_sets_fetch_counts(s.eng.ctx, s.h, 0, nSets, (*C.uint32_t)(unsafe.Pointer(&counts[0])), nValues+1)
	runtime.KeepAlive(s)
	return counts[:nValues], s.eng.err(rc)
}

// OpCounted combines the sets pair by pair as Op does, counts included; besides Op's pairings an a of exactly one set is
// combined with every set of b (bsk_sets_op_counted).  Sets without counts count 1 for every value.  into as in Op.
func (a *Sets) OpCounted(b *Sets, op CountOp, into *Sets) (*Sets, error) {
	if into == nil {
		into = &Sets{eng: a.eng}
		runtime.SetFinalizer(into, func(s *Sets) { C.bsk_sets_release(s.h) })
	}
	rc := C.bsk_sets_op_counted(a.eng.ctx, a.h, b.h, C.int(op), &into.h)
	runtime.KeepAlive(a)
	runtime.KeepAlive(b)
	return into, a.eng.err(rc)
}

// FilterCounts keeps the values with minCount <= count <= maxCount, and their counts (bsk_sets_filter_counts).  into as in Op.
func (s *Sets) FilterCounts(minCount, maxCount uint32, into *Sets) (*Sets, error) {
	if into == nil {
		into = &Sets{eng: s.eng}
		runtime.SetFinalizer(into, func(r *Sets) { C.bsk_sets_release(r.h) })
	}
	rc := C.bsk_sets_filter_counts(s.eng.ctx, s.h, C.uint32_t(minCount), C.uint32_t(maxCount), &into.h)
	runtime.KeepAlive(s)
	return into, s.eng.err(rc)
}

// Totals returns, per set, the sum of its counts (bsk_sets_totals); for sets without counts, their sizes.
func (s *Sets) Totals() ([]uint64, error) {
	var nSets, nValues C.uint64_t
	C.bsk_sets_info(s.h, &nSets, &nValues)
	totals := make([]uint64, uint64(nSets)+1)
	rc := C.bsk_sets_totals(s.eng.ctx, s.h, 0, nSets, (*C.uint64_t)(unsafe.Pointer(&totals[0])))
	runtime.KeepAlive(s)
	return totals[:nSets], s.eng.err(rc)
}

// SumSq returns, per set, the sum of its squared counts, saturating at 2^64-1 (bsk_sets_sumsq): the squared norm that
// (*Compare).Cosine divides by; for sets without counts, their sizes.
func (s *Sets) SumSq() ([]uint64, error) {
	var nSets, nValues C.uint64_t
	C.bsk_sets_info(s.h, &nSets, &nValues)
	sumsq := make([]uint64, uint64(nSets)+1)
	rc := C.bsk_sets_sumsq(s.eng.ctx, s.h, 0, nSets, (*C.uint64_t)(unsafe.Pointer(&sumsq[0])))
	runtime.KeepAlive(s)
	return sumsq[:nSets], s.eng.err(rc)
}

// SetsFromHostCounted loads sets with their counts from the host (bsk_sets_from_host_counted): SetsFromHost's rules, and no
// count may be 0.
func (e *Engine) SetsFromHostCounted(offsets []uint64, values []uint64, counts []uint32) (*Sets, error) {
	if len(offsets) == 0 || offsets[len(offsets)-1] != uint64(len(values)) || len(counts) != len(values) {
		return nil, errors.New("SetsFromHostCounted: offsets must have n+1 entries and end at len(values) == len(counts)")
	}
	var vp *C.uint64_t
	var cp *C.uint32_t
	if len(values) > 0 {
		vp = (*C.uint64_t)(unsafe.Pointer(&values[0]))
		cp = (*C.uint32_t)(unsafe.Pointer(&counts[0]))
	}
	s := &Sets{eng: e}
	rc := C.bsk_sets_from_host_counted(e.ctx, (*C.uint64_t)(unsafe.Pointer(&offsets[0])), C.uint64_t(len(offsets)-1), vp, cp, &s.h)
	runtime.KeepAlive(offsets)
	runtime.KeepAlive(values)
	runtime.KeepAlive(counts)
	if err := e.err(rc); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(s, func(s *Sets) { C.bsk_sets_release(s.h) })
	return s, nil
}
