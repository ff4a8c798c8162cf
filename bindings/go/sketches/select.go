//go:build biosketch

package sketches

/*
#cgo LDFLAGS: -lbiosketch
#include <stdlib.h>
#include "biosketch.h"
*/
import "C"

import (
	"runtime"
	"unsafe"
)

// ---- hits selected by a measure: an exact filter, a top-n that keeps the payloads --------------------------------------------------
//
// near, _ := hits.Filter(Measure{Kind: MeasureCosine, QNorm: sumsqA, TNorm: sumsqB}, 9, 10, nil) keeps the neighbours of cosine >= 9/10
// with their totals, weights and members; near.Cluster(...) then clusters by that weighted measure, and
// folded.TopBy(Measure{Kind: MeasureMembers}, 1, nil) is every read's best genome with the chunks it hit.  Nothing leaves the device.

// The kinds of a Measure (BSK_MEASURE_*): every one an exact fraction N/D of the hit's integers and the two norms.
const (
	MeasureShared          = uint32(C.BSK_MEASURE_SHARED)
	MeasureMembers         = uint32(C.BSK_MEASURE_MEMBERS)
	MeasureDot             = uint32(C.BSK_MEASURE_DOT)
	MeasureMinSum          = uint32(C.BSK_MEASURE_MIN_SUM)
	MeasureQueryCov        = uint32(C.BSK_MEASURE_QUERY_COV)
	MeasureTargetCov       = uint32(C.BSK_MEASURE_TARGET_COV)
	MeasureJaccard         = uint32(C.BSK_MEASURE_JACCARD)
	MeasureCosine          = uint32(C.BSK_MEASURE_COSINE)
	MeasureWeightedJaccard = uint32(C.BSK_MEASURE_WEIGHTED_JACCARD)
	MeasureBCSimilarity    = uint32(C.BSK_MEASURE_BC_SIMILARITY)
	MeasureQueryMass       = uint32(C.BSK_MEASURE_QUERY_MASS)
)

// Measure is bsk_measure: the kind and the norms it reads -- QNorm one u64 per query, TNorm one per target (the sets' sizes, sumsq or
// totals, as the kind asks); nil where the kind needs none.  The slices are read during the call only.
type Measure struct {
	Kind         uint32
	QNorm, TNorm []uint64
}

// c is the C form of m; the norms are pinned for the call (a struct handed to C may only point at pinned Go memory)
func (m Measure) c(pin *runtime.Pinner) C.bsk_measure {
	cm := C.bsk_measure{kind: C.uint32_t(m.Kind), n_qnorm: C.uint64_t(len(m.QNorm)), n_tnorm: C.uint64_t(len(m.TNorm))}
	if len(m.QNorm) != 0 {
		pin.Pin(&m.QNorm[0])
		cm.qnorm = (*C.uint64_t)(unsafe.Pointer(&m.QNorm[0]))
	}
	if len(m.TNorm) != 0 {
		pin.Pin(&m.TNorm[0])
		cm.tnorm = (*C.uint64_t)(unsafe.Pointer(&m.TNorm[0]))
	}
	return cm
}

func (h *Hits) selected(reuse *Hits) *Hits {
	if reuse == nil {
		reuse = &Hits{eng: h.eng}
		runtime.SetFinalizer(reuse, func(r *Hits) { C.bsk_hits_release(r.h) })
	}
	return reuse
}

// Filter keeps the hits whose measure is at least minNum / minDen, compared in integers (bsk_hits_filter; for MeasureCosine the bound
// is on the cosine itself).  Rows keep their order and every payload -- totals, weights, members -- stays with its hit.  reuse: nil,
// or any Hits of this engine but h.
func (h *Hits) Filter(m Measure, minNum, minDen uint64, reuse *Hits) (*Hits, error) {
	reuse = h.selected(reuse)
	var pin runtime.Pinner
	defer pin.Unpin()
	cm := m.c(&pin)
	fp := C.bsk_filter_params{min_num: C.uint64_t(minNum), min_den: C.uint64_t(minDen)}
	rc := C.bsk_hits_filter(h.eng.ctx, h.h, &cm, &fp, &reuse.h)
	runtime.KeepAlive(h)
	runtime.KeepAlive(m)
	return reuse, h.eng.err(rc)
}

// TopBy keeps every query's min(n, hits) hits of largest measure, best first, ties by ascending target, with every payload
// (bsk_hits_top_by); with MeasureShared the hits are those of Top, which drops the payloads.  reuse: nil, or any Hits of this engine but h.
func (h *Hits) TopBy(m Measure, n uint32, reuse *Hits) (*Hits, error) {
	reuse = h.selected(reuse)
	var pin runtime.Pinner
	defer pin.Unpin()
	cm := m.c(&pin)
	rc := C.bsk_hits_top_by(h.eng.ctx, h.h, &cm, C.uint32_t(n), &reuse.h)
	runtime.KeepAlive(h)
	runtime.KeepAlive(m)
	return reuse, h.eng.err(rc)
}
