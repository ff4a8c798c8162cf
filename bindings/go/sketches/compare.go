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
	"math"
	"runtime"
	"unsafe"
)

// ---- MinHash on the device: bottom-n sets and the dense all-pairs comparison ---------------------------------------------
//
// s.Bottom(1000, nil) is the Mash / sourmash num= sketch of every set; a.Compare(b, 1000, nil) walks, for every pair, the first
// 1000 distinct values of the union and counts those both sets hold: Shared / Total is the Mash estimator of the Jaccard.
// A limit of 0 walks the whole union: the exact Jaccard.

// Bottom cuts every set to its min(n, size) smallest values, counts included for counted sets (bsk_sets_bottom).  into as in Op.
func (s *Sets) Bottom(n uint64, into *Sets) (*Sets, error) {
	if into == nil {
		into = &Sets{eng: s.eng}
		runtime.SetFinalizer(into, func(r *Sets) { C.bsk_sets_release(r.h) })
	}
	rc := C.bsk_sets_bottom(s.eng.ctx, s.h, C.uint64_t(n), &into.h)
	runtime.KeepAlive(s)
	return into, s.eng.err(rc)
}

// Compare is the result of (*Sets).Compare: two dense row-major matrices on the device, Shared and Total.
type Compare struct {
	eng *Engine
	h   *C.bsk_compare
}

// Compare compares every set of a with every set of b (nil: of a itself) into `into` (nil the first time; the device arrays of an
// earlier Compare are kept and only grow): bsk_sets_compare.
func (a *Sets) Compare(b *Sets, limit uint64, into *Compare) (*Compare, error) {
	if b == nil {
		b = a
	}
	if into == nil {
		into = &Compare{eng: a.eng}
		runtime.SetFinalizer(into, func(m *Compare) { C.bsk_compare_release(m.h) })
	}
	rc := C.bsk_sets_compare(a.eng.ctx, a.h, b.h, C.uint64_t(limit), &into.h)
	runtime.KeepAlive(a)
	runtime.KeepAlive(b)
	return into, a.eng.err(rc)
}

// Info returns the matrix's rows and columns and the limit it was computed with (bsk_compare_info).
func (m *Compare) Info() (nA, nB, limit uint64) {
	var a, b, l C.uint64_t
	C.bsk_compare_info(m.h, &a, &b, &l)
	runtime.KeepAlive(m)
	return uint64(a), uint64(b), uint64(l)
}

// Plan describes what ran, and returns the tiles run, the rounds summed over them and the most rounds of one tile (bsk_compare_plan).
func (m *Compare) Plan() (string, [3]uint64) {
	var p *C.char
	var f [3]C.uint64_t
	C.bsk_compare_plan(m.h, &p, &f[0])
	runtime.KeepAlive(m)
	return C.GoString(p), [3]uint64{uint64(f[0]), uint64(f[1]), uint64(f[2])}
}

// Fetch copies rows firstRow .. firstRow+nRows-1 of both matrices to the host, nRows * nB cells each (bsk_compare_fetch).
func (m *Compare) Fetch(firstRow, nRows uint64) (shared, total []uint32, err error) {
	_, nB, _ := m.Info()
	cells := nRows * nB
	shared = make([]uint32, cells+1)
	total = make([]uint32, cells+1)
	rc := C.bsk_compare_fetch(m.eng.ctx, m.h, C.uint64_t(firstRow), C.uint64_t(nRows), (*C.uint32_t)(unsafe.Pointer(&shared[0])),
		(*C.uint32_t)(unsafe.Pointer(&total[0])), C.uint64_t(cells))
	runtime.KeepAlive(m)
	return shared[:cells], total[:cells], m.eng.err(rc)
}

// Device returns the device addresses of the two matrices (bsk_compare_device).
func (m *Compare) Device() (shared, total unsafe.Pointer) {
	var s, t *C.uint32_t
	C.bsk_compare_device(m.h, &s, &t)
	runtime.KeepAlive(m)
	return unsafe.Pointer(s), unsafe.Pointer(t)
}

// Close releases the device arrays now instead of at finalisation.
func (m *Compare) Close() {
	C.bsk_compare_release(m.h)
	m.h = nil
}

// Jaccard returns Shared / Total of every cell, row-major, 0 where Total is 0.
func (m *Compare) Jaccard() ([]float64, error) {
	nA, _, _ := m.Info()
	shared, total, err := m.Fetch(0, nA)
	if err != nil {
		return nil, err
	}
	j := make([]float64, len(shared))
	for i := range j {
		if total[i] != 0 {
			j[i] = float64(shared[i]) / float64(total[i])
		}
	}
	return j, nil
}

// MashDistance returns, with j the Jaccard of a cell, 1 where j is 0 and max(0, -ln(2j / (1 + j)) / k) elsewhere.
func (m *Compare) MashDistance(k int) ([]float64, error) {
	j, err := m.Jaccard()
	if err != nil {
		return nil, err
	}
	for i, x := range j {
		if x == 0 {
			j[i] = 1
		} else {
			j[i] = math.Max(0, -math.Log(2*x/(1+x))/float64(k))
		}
	}
	return j, nil
}

// ---- sparse all-pairs comparison: the neighbours above a threshold, no matrix --------------------------------------------
//
// a.Neighbors(nil, 1000, NeighborParams{JaccardNum: 9, JaccardDen: 10, Upper: true}, nil) walks every pair as Compare does and
// lists, per set of a, the sets that pass the thresholds: a Hits with Totals, at any number of cells.  h.Top(5, nil) then gives the
// five nearest neighbours of every set.

// NeighborParams is bsk_neighbor_params: a pair is listed iff shared >= max(MinShared, 1), and, with JaccardDen != 0,
// shared * JaccardDen >= JaccardNum * total (exact), and, with Upper, j > i.
type NeighborParams struct {
	MinShared              uint32
	JaccardNum, JaccardDen uint32
	Upper                  bool
}

// Neighbors compares every set of a with every set of b (nil: of a itself) and keeps the pairs p admits (bsk_sets_neighbors).
// reuse: nil, or any Hits of this engine, whose device arrays are kept and only grow.
func (a *Sets) Neighbors(b *Sets, limit uint64, p NeighborParams, reuse *Hits) (*Hits, error) {
	if b == nil {
		b = a
	}
	if reuse == nil {
		reuse = &Hits{eng: a.eng}
		runtime.SetFinalizer(reuse, func(h *Hits) { C.bsk_hits_release(h.h) })
	}
	np := C.bsk_neighbor_params{min_shared: C.uint32_t(p.MinShared), jaccard_num: C.uint32_t(p.JaccardNum), jaccard_den: C.uint32_t(p.JaccardDen)}
	if p.Upper {
		np.flags = C.BSK_NEIGHBORS_UPPER
	}
	rc := C.bsk_sets_neighbors(a.eng.ctx, a.h, b.h, C.uint64_t(limit), &np, &reuse.h)
	runtime.KeepAlive(a)
	runtime.KeepAlive(b)
	return reuse, a.eng.err(rc)
}

// Totals returns the device address of total[], nil for hits without totals: a search, Top (bsk_hits_totals_device).
func (h *Hits) Totals() unsafe.Pointer {
	var t *C.uint32_t
	C.bsk_hits_totals_device(h.h, &t)
	runtime.KeepAlive(h)
	return unsafe.Pointer(t)
}

// FetchTotals copies the totals of the hits of rows [first, first+count) to the host (bsk_hits_fetch_totals); hits without
// totals are an error.
func (h *Hits) FetchTotals(first, count uint64) ([]uint32, error) {
	offsets, _, _, err := h.Fetch(first, count)
	if err != nil {
		return nil, err
	}
	n := offsets[count]
	total := make([]uint32, n+1)
	rc := C.bsk_hits_fetch_totals(h.eng.ctx, h.h, C.uint64_t(first), C.uint64_t(count), (*C.uint32_t)(unsafe.Pointer(&total[0])), C.uint64_t(n+1))
	runtime.KeepAlive(h)
	return total[:n], h.eng.err(rc)
}

// NeighborsCounted is Neighbors with the counts (bsk_sets_neighbors_counted): the same pairs, offsets, targets, shared and totals,
// and per kept pair Dot and MinSum as CompareCounted defines them (Weights, FetchWeights).  The thresholds of p read shared and
// total only.  Sets without counts count 1.  reuse: nil, or any Hits of this engine.
func (a *Sets) NeighborsCounted(b *Sets, limit uint64, p NeighborParams, reuse *Hits) (*Hits, error) {
	if b == nil {
		b = a
	}
	if reuse == nil {
		reuse = &Hits{eng: a.eng}
		runtime.SetFinalizer(reuse, func(h *Hits) { C.bsk_hits_release(h.h) })
	}
	np := C.bsk_neighbor_params{min_shared: C.uint32_t(p.MinShared), jaccard_num: C.uint32_t(p.JaccardNum), jaccard_den: C.uint32_t(p.JaccardDen)}
	if p.Upper {
		np.flags = C.BSK_NEIGHBORS_UPPER
	}
	rc := C.bsk_sets_neighbors_counted(a.eng.ctx, a.h, b.h, C.uint64_t(limit), &np, &reuse.h)
	runtime.KeepAlive(a)
	runtime.KeepAlive(b)
	return reuse, a.eng.err(rc)
}

// Weights returns the device addresses of dot[] and min_sum[], both nil for hits without weights: anything but NeighborsCounted
// (bsk_hits_weights_device).
func (h *Hits) Weights() (dot, minSum unsafe.Pointer) {
	var d, m *C.uint64_t
	C.bsk_hits_weights_device(h.h, &d, &m)
	runtime.KeepAlive(h)
	return unsafe.Pointer(d), unsafe.Pointer(m)
}

// FetchWeights copies dot and min_sum of the hits of rows [first, first+count) to the host (bsk_hits_fetch_weights); hits without
// weights are an error.
func (h *Hits) FetchWeights(first, count uint64) (dot, minSum []uint64, err error) {
	offsets, _, _, err := h.Fetch(first, count)
	if err != nil {
		return nil, nil, err
	}
	n := offsets[count]
	dot, minSum = make([]uint64, n+1), make([]uint64, n+1)
	rc := C.bsk_hits_fetch_weights(h.eng.ctx, h.h, C.uint64_t(first), C.uint64_t(count), (*C.uint64_t)(unsafe.Pointer(&dot[0])),
		(*C.uint64_t)(unsafe.Pointer(&minSum[0])), C.uint64_t(n+1))
	runtime.KeepAlive(h)
	return dot[:n], minSum[:n], h.eng.err(rc)
}

// ---- abundance-weighted comparison of counted sets ------------------------------------------------------------------------
//
// a.CompareCounted(b, 0, nil) walks every pair as Compare does and keeps, over the walked values both sets hold, Dot = the sum of
// the products of the two counts (saturating at 2^64-1) and MinSum = the sum of their minima.  Sets without counts count 1.

// CompareCounted is Compare with the counts (bsk_sets_compare_counted); into may be the result of either kind of compare.
func (a *Sets) CompareCounted(b *Sets, limit uint64, into *Compare) (*Compare, error) {
	if b == nil {
		b = a
	}
	if into == nil {
		into = &Compare{eng: a.eng}
		runtime.SetFinalizer(into, func(m *Compare) { C.bsk_compare_release(m.h) })
	}
	rc := C.bsk_sets_compare_counted(a.eng.ctx, a.h, b.h, C.uint64_t(limit), &into.h)
	runtime.KeepAlive(a)
	runtime.KeepAlive(b)
	return into, a.eng.err(rc)
}

// Weights returns the device addresses of Dot and MinSum, both nil for an unweighted result (bsk_compare_weights_device).
func (m *Compare) Weights() (dot, minSum unsafe.Pointer) {
	var d, s *C.uint64_t
	C.bsk_compare_weights_device(m.h, &d, &s)
	runtime.KeepAlive(m)
	return unsafe.Pointer(d), unsafe.Pointer(s)
}

// FetchWeights copies rows firstRow .. firstRow+nRows-1 of Dot and MinSum to the host (bsk_compare_fetch_weights); an
// unweighted result is an error.
func (m *Compare) FetchWeights(firstRow, nRows uint64) (dot, minSum []uint64, err error) {
	_, nB, _ := m.Info()
	cells := nRows * nB
	dot = make([]uint64, cells+1)
	minSum = make([]uint64, cells+1)
	rc := C.bsk_compare_fetch_weights(m.eng.ctx, m.h, C.uint64_t(firstRow), C.uint64_t(nRows), (*C.uint64_t)(unsafe.Pointer(&dot[0])),
		(*C.uint64_t)(unsafe.Pointer(&minSum[0])), C.uint64_t(cells))
	runtime.KeepAlive(m)
	return dot[:cells], minSum[:cells], m.eng.err(rc)
}

// Cosine returns Dot / (sqrt(sumSqA[i]) * sqrt(sumSqB[j])) of every cell, row-major, with the operands' (*Sets).SumSq: 0 where a
// norm is 0, NaN where Dot or either norm is saturated.  Whole sets only: a limit other than 0 is an error.
func (m *Compare) Cosine(sumSqA, sumSqB []uint64) ([]float64, error) {
	nA, nB, limit := m.Info()
	if limit != 0 {
		return nil, errors.New("Cosine: defined on whole sets, CompareCounted with limit 0")
	}
	if uint64(len(sumSqA)) != nA || uint64(len(sumSqB)) != nB {
		return nil, errors.New("Cosine: one squared norm per set of either operand")
	}
	dot, _, err := m.FetchWeights(0, nA)
	if err != nil {
		return nil, err
	}
	cos := make([]float64, len(dot))
	for i := uint64(0); i < nA; i++ {
		for j := uint64(0); j < nB; j++ {
			d, qa, qb := dot[i*nB+j], sumSqA[i], sumSqB[j]
			switch {
			case d == math.MaxUint64 || qa == math.MaxUint64 || qb == math.MaxUint64:
				cos[i*nB+j] = math.NaN()
			case qa != 0 && qb != 0:
				cos[i*nB+j] = float64(d) / (math.Sqrt(float64(qa)) * math.Sqrt(float64(qb)))
			}
		}
	}
	return cos, nil
}
