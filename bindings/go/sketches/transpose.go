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

// ---- hits by target: the transpose with its payloads, the per-target tally ---------------------------------------------------------
//
// byGenome, _ := hits.Transpose(nGenomes, nil) lists per genome the reads that hit it, every payload with its hit;
// byGenome.TopBy(Measure{Kind: MeasureShared}, 1, nil) is every genome's best read.  table, _ := hits.Tally(nGenomes, true, table)
// adds a batch's hits per genome -- all, those of reads that hit nothing else, and the shared values -- into one table on the device.

// Transpose writes the hits whose rows are the nTargets targets (bsk_hits_transpose): row t lists the queries that hit t, ascending,
// with shared and every payload of the hit.  Targets nobody hit are empty rows.  reuse: nil, or any Hits of this engine but h.
func (h *Hits) Transpose(nTargets uint64, reuse *Hits) (*Hits, error) {
	reuse = h.selected(reuse)
	rc := C.bsk_hits_transpose(h.eng.ctx, h.h, C.uint64_t(nTargets), &reuse.h)
	runtime.KeepAlive(h)
	return reuse, h.eng.err(rc)
}

// Tally is bsk_tally: per target the hits that name it, those among them that are the only hit of their row, and the sum of their
// shared values -- three u64 arrays on the device.
type Tally struct {
	eng *Engine
	t   *C.bsk_tally
}

// Tally fills the per-target table of the hits (bsk_hits_tally).  into: nil, or the Tally of an earlier call on this engine, which is
// overwritten -- or, with add, added to: it must then be a table of the same nTargets, and its Info adds up too.
func (h *Hits) Tally(nTargets uint64, add bool, into *Tally) (*Tally, error) {
	if into == nil {
		into = &Tally{eng: h.eng}
		runtime.SetFinalizer(into, func(r *Tally) { C.bsk_tally_release(r.t) })
	}
	flags := C.uint32_t(0)
	if add {
		flags = C.uint32_t(C.BSK_TALLY_ADD)
	}
	rc := C.bsk_hits_tally(h.eng.ctx, h.h, C.uint64_t(nTargets), flags, &into.t)
	runtime.KeepAlive(h)
	return into, h.eng.err(rc)
}

// Info reports the targets of the table and the queries, hits and calls it holds (bsk_tally_info).
func (t *Tally) Info() (nTargets, queries, hits, calls uint64) {
	var n, q, hh, k C.uint64_t
	C.bsk_tally_info(t.t, &n, &q, &hh, &k)
	runtime.KeepAlive(t)
	return uint64(n), uint64(q), uint64(hh), uint64(k)
}

// Plan says what the last call ran (bsk_tally_plan): counters in LDS or adds to the table, with targets= and hits=.
func (t *Tally) Plan() string {
	var p *C.char
	C.bsk_tally_plan(t.t, &p)
	runtime.KeepAlive(t)
	if p == nil {
		return ""
	}
	return C.GoString(p)
}

// Fetch copies targets first .. first+count-1 of the table to the host (bsk_tally_fetch).
func (t *Tally) Fetch(first, count uint64) (rows, unique, shared []uint64, err error) {
	rows, unique, shared = make([]uint64, count+1), make([]uint64, count+1), make([]uint64, count+1)
	rc := C.bsk_tally_fetch(t.eng.ctx, t.t, C.uint64_t(first), C.uint64_t(count), (*C.uint64_t)(unsafe.Pointer(&rows[0])),
		(*C.uint64_t)(unsafe.Pointer(&unique[0])), (*C.uint64_t)(unsafe.Pointer(&shared[0])))
	runtime.KeepAlive(t)
	return rows[:count], unique[:count], shared[:count], t.eng.err(rc)
}

// Device returns the device addresses of the three arrays, nTargets u64 each (bsk_tally_device); they live as long as the Tally.
func (t *Tally) Device() (rows, unique, shared unsafe.Pointer) {
	var r, u, s *C.uint64_t
	C.bsk_tally_device(t.t, &r, &u, &s)
	return unsafe.Pointer(r), unsafe.Pointer(u), unsafe.Pointer(s)
}

// Release frees the table now instead of at garbage collection.
func (t *Tally) Release() {
	C.bsk_tally_release(t.t)
	t.t = nil
}
