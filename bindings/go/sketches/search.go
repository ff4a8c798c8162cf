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

// ---- containment search: what kmcp does with the sets -------------------------------------------------------------------
//
// Target sets (genomes, per sequence) -> BuildIndex; query sets (reads) -> Search: for every query, the targets that share
// enough values with it, and how many.  Everything stays on the device; only the hits cross the link.

// SetsFromHost uploads sets built elsewhere (e.g. a reference collection read from disk): offsets[n+1] with offsets[0] = 0 and
// offsets[n] = len(values), values strictly ascending inside every set (bsk_sets_from_host).
func (e *Engine) SetsFromHost(offsets []uint64, values []uint64) (*Sets, error) {
	if len(offsets) == 0 || offsets[len(offsets)-1] != uint64(len(values)) {
		return nil, errors.New("SetsFromHost: offsets must have n+1 entries and end at len(values)")
	}
	var vp *C.uint64_t
	if len(values) > 0 {
		vp = (*C.uint64_t)(unsafe.Pointer(&values[0]))
	}
	s := &Sets{eng: e}
	rc := C.bsk_sets_from_host(e.ctx, (*C.uint64_t)(unsafe.Pointer(&offsets[0])), C.uint64_t(len(offsets)-1), vp, &s.h)
	runtime.KeepAlive(offsets)
	runtime.KeepAlive(values)
	if err := e.err(rc); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(s, func(s *Sets) { C.bsk_sets_release(s.h) })
	return s, nil
}

// Index is a device-resident inverted index of target sets (bsk_index): value -> ascending target ids.
type Index struct {
	eng *Engine
	h   *C.bsk_index
}

// IndexInfo is what bsk_index_info reports.
type IndexInfo struct {
	Targets, Postings, Distinct, MaxBucket, DeviceBytes uint64
}

// BuildIndex indexes the sets as search targets (bsk_index_build); s may be released afterwards.
func (s *Sets) BuildIndex() (*Index, error) {
	ix := &Index{eng: s.eng}
	rc := C.bsk_index_build(s.eng.ctx, s.h, &ix.h)
	runtime.KeepAlive(s)
	if err := s.eng.err(rc); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(ix, func(ix *Index) { C.bsk_index_release(ix.h) })
	return ix, nil
}

// Info of the index (bsk_index_info).
func (ix *Index) Info() IndexInfo {
	var t, p, d, m, b C.uint64_t
	C.bsk_index_info(ix.h, &t, &p, &d, &m, &b)
	runtime.KeepAlive(ix)
	return IndexInfo{uint64(t), uint64(p), uint64(d), uint64(m), uint64(b)}
}

// SearchParams: a (query, target) pair sharing s values is listed iff s >= max(MinShared, 1), s >= MinQueryCov*|q| and
// s >= MinTargetCov*|t|.
type SearchParams struct {
	MinShared    uint32
	MinQueryCov  float64
	MinTargetCov float64
}

// Hits of one search (bsk_hits): CSR by query, target ids ascending inside a query.
type Hits struct {
	eng *Engine
	h   *C.bsk_hits
}

// Search lists the targets every query set shares enough values with (bsk_index_search).  into: nil, or the Hits of an earlier
// search on this engine, whose device arrays are kept and only grow.
func (ix *Index) Search(q *Sets, p SearchParams, into *Hits) (*Hits, error) {
	if into == nil {
		into = &Hits{eng: ix.eng}
		runtime.SetFinalizer(into, func(h *Hits) { C.bsk_hits_release(h.h) })
	}
	sp := C.bsk_search_params{min_shared: C.uint32_t(p.MinShared), min_query_cov: C.double(p.MinQueryCov), min_target_cov: C.double(p.MinTargetCov)}
	rc := C.bsk_index_search(ix.eng.ctx, ix.h, q.h, &sp, &into.h)
	runtime.KeepAlive(ix)
	runtime.KeepAlive(q)
	return into, ix.eng.err(rc)
}

// BuildIndexCounted indexes the sets with their counts (bsk_index_build_counted): BuildIndex plus, per posting, the target's count
// of the value, and per target the squared norm and the total of its counts.  Sets without counts give an index without counts.
func (s *Sets) BuildIndexCounted() (*Index, error) {
	ix := &Index{eng: s.eng}
	rc := C.bsk_index_build_counted(s.eng.ctx, s.h, &ix.h)
	runtime.KeepAlive(s)
	if err := s.eng.err(rc); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(ix, func(ix *Index) { C.bsk_index_release(ix.h) })
	return ix, nil
}

// Counted reports whether the index keeps counts (bsk_index_counted).
func (ix *Index) Counted() bool {
	var k C.int
	C.bsk_index_counted(ix.h, &k)
	runtime.KeepAlive(ix)
	return k != 0
}

// Norms of targets [first, first+count): the sum of the squared counts (saturating at 2^64-1) and the sum of the counts
// (bsk_index_fetch_norms); an index without counts reports the targets' sizes for both.
func (ix *Index) Norms(first, count uint64) (sumsq, totals []uint64, err error) {
	sumsq = make([]uint64, count+1)
	totals = make([]uint64, count+1)
	rc := C.bsk_index_fetch_norms(ix.eng.ctx, ix.h, C.uint64_t(first), C.uint64_t(count), (*C.uint64_t)(unsafe.Pointer(&sumsq[0])),
		(*C.uint64_t)(unsafe.Pointer(&totals[0])))
	runtime.KeepAlive(ix)
	return sumsq[:count], totals[:count], ix.eng.err(rc)
}

// SearchCounted is Search with the counts (bsk_index_search_counted): the same hits, bit for bit -- the thresholds read the
// shared count only -- and per hit the dot product and the sum of minima of the two count vectors over the shared values
// ((*Hits).Weights, FetchWeights).  Queries or an index without counts count 1 for every value.  into: nil, or any Hits of this engine.
func (ix *Index) SearchCounted(q *Sets, p SearchParams, into *Hits) (*Hits, error) {
	if into == nil {
		into = &Hits{eng: ix.eng}
		runtime.SetFinalizer(into, func(h *Hits) { C.bsk_hits_release(h.h) })
	}
	sp := C.bsk_search_params{min_shared: C.uint32_t(p.MinShared), min_query_cov: C.double(p.MinQueryCov), min_target_cov: C.double(p.MinTargetCov)}
	rc := C.bsk_index_search_counted(ix.eng.ctx, ix.h, q.h, &sp, &into.h)
	runtime.KeepAlive(ix)
	runtime.KeepAlive(q)
	return into, ix.eng.err(rc)
}

// Info: queries and hits (bsk_hits_info).
func (h *Hits) Info() (queries, hits uint64) {
	var nq, nh C.uint64_t
	C.bsk_hits_info(h.h, &nq, &nh)
	runtime.KeepAlive(h)
	return uint64(nq), uint64(nh)
}

// Plan: what the search ran, and how many queries took the large-query path (bsk_hits_plan).
func (h *Hits) Plan() (string, uint64) {
	var p *C.char
	var n C.uint64_t
	C.bsk_hits_plan(h.h, &p, &n)
	s := C.GoString(p)
	runtime.KeepAlive(h)
	return s, uint64(n)
}

// Fetch copies the hits of queries [first, first+count) to the host (bsk_hits_fetch): offsets rebased to 0.
func (h *Hits) Fetch(first, count uint64) (offsets []uint64, target []uint32, shared []uint32, err error) {
	offsets = make([]uint64, count+1)
	rc := C.bsk_hits_fetch(h.eng.ctx, h.h, C.uint64_t(first), C.uint64_t(count), (*C.uint64_t)(unsafe.Pointer(&offsets[0])), nil, nil, 0)
	if err = h.eng.err(rc); err != nil {
		return nil, nil, nil, err
	}
	n := offsets[count]
	target = make([]uint32, n+1)
	shared = make([]uint32, n+1)
	rc = C.bsk_hits_fetch(h.eng.ctx, h.h, C.uint64_t(first), C.uint64_t(count), (*C.uint64_t)(unsafe.Pointer(&offsets[0])),
		(*C.uint32_t)(unsafe.Pointer(&target[0])), (*C.uint32_t)(unsafe.Pointer(&shared[0])), C.uint64_t(n+1))
	runtime.KeepAlive(h)
	return offsets, target[:n], shared[:n], h.eng.err(rc)
}

// DevicePointers of the hits: offsets[n_queries+1] (u64), target[] and shared[] (u32) (bsk_hits_device).
func (h *Hits) DevicePointers() (offsets, target, shared unsafe.Pointer) {
	var o *C.uint64_t
	var t, s *C.uint32_t
	C.bsk_hits_device(h.h, &o, &t, &s)
	runtime.KeepAlive(h)
	return unsafe.Pointer(o), unsafe.Pointer(t), unsafe.Pointer(s)
}

// Attach returns a handle on the index for another engine (bsk_index_attach): on the same device the device arrays are shared
// (reference counted), on another device they are copied there once.  The handle is searched like any Index; the handles of an
// index may be released in any order, but not while a search on that same handle runs.
func (ix *Index) Attach(e *Engine) (*Index, error) {
	h := &Index{eng: e}
	rc := C.bsk_index_attach(e.ctx, ix.h, &h.h)
	runtime.KeepAlive(ix)
	if err := e.err(rc); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(h, func(h *Index) { C.bsk_index_release(h.h) })
	return h, nil
}

// Top keeps every query's min(n, hits) best hits: largest shared count first, ties by ascending target id (bsk_hits_top).
// into: nil, or the Hits of an earlier Top on this engine, whose device arrays are kept and only grow.
func (h *Hits) Top(n uint32, into *Hits) (*Hits, error) {
	if into == nil {
		into = &Hits{eng: h.eng}
		runtime.SetFinalizer(into, func(t *Hits) { C.bsk_hits_release(t.h) })
	}
	rc := C.bsk_hits_top(h.eng.ctx, h.h, C.uint32_t(n), &into.h)
	runtime.KeepAlive(h)
	return into, h.eng.err(rc)
}
