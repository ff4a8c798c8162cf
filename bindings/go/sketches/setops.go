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

// ---- set algebra on device-resident sets: what unikmer's union / inter / diff do on disk --------------------------------
//
// A genome of many contigs is the union of its contigs' sets (Reduce), a read pair the union of its mates' (Reduce in groups
// of two), a masked read its set minus the host's (Op with a one-set operand).  The results are ordinary Sets: BuildIndex,
// Search and the fetches work on them.

// SetOp names the operation of (*Sets).Op.
type SetOp int

const (
	SetUnion     SetOp = C.BSK_SETOP_UNION
	SetIntersect SetOp = C.BSK_SETOP_INTERSECT
	SetDiff      SetOp = C.BSK_SETOP_DIFF // a \ b
	SetSymDiff   SetOp = C.BSK_SETOP_SYMDIFF
)

// MembersAll as Reduce's minMembers: the values every member of a group holds.
const MembersAll uint32 = C.BSK_MEMBERS_ALL

// Op combines the sets pair by pair: set i of the result is a[i] op b[i]; a b of exactly one set is combined with every set of
// a (bsk_sets_op).  into: nil, or the Sets of an earlier Op / Reduce on this engine, whose device arrays are kept and only grow;
// it must be neither a nor b.
func (a *Sets) Op(b *Sets, op SetOp, into *Sets) (*Sets, error) {
	if into == nil {
		into = &Sets{eng: a.eng}
		runtime.SetFinalizer(into, func(s *Sets) { C.bsk_sets_release(s.h) })
	}
	rc := C.bsk_sets_op(a.eng.ctx, a.h, b.h, C.int(op), &into.h)
	runtime.KeepAlive(a)
	runtime.KeepAlive(b)
	return into, a.eng.err(rc)
}

// Reduce turns runs of consecutive sets into one set each: group g is sets groupOffsets[g] .. groupOffsets[g+1]-1, and its set
// holds the values at least minMembers of them hold -- 1: the union, MembersAll: the intersection (bsk_sets_reduce).
// groupOffsets starts at 0, never decreases and ends at the number of sets.  into as in Op.
func (s *Sets) Reduce(groupOffsets []uint64, minMembers uint32, into *Sets) (*Sets, error) {
	if len(groupOffsets) == 0 {
		return nil, errors.New("Reduce: groupOffsets must have n+1 entries")
	}
	if into == nil {
		into = &Sets{eng: s.eng}
		runtime.SetFinalizer(into, func(r *Sets) { C.bsk_sets_release(r.h) })
	}
	rc := C.bsk_sets_reduce(s.eng.ctx, s.h, (*C.uint64_t)(unsafe.Pointer(&groupOffsets[0])), C.uint64_t(len(groupOffsets)-1), C.uint32_t(minMembers), &into.h)
	runtime.KeepAlive(s)
	runtime.KeepAlive(groupOffsets)
	return into, s.eng.err(rc)
}

// Plan: what made these sets, and how many pairs of the last Op into them took the group, wave and tiled path (bsk_sets_plan);
// sets of any other origin report an empty string and zeros.
func (s *Sets) Plan() (string, [3]uint64) {
	var p *C.char
	var n [3]C.uint64_t
	C.bsk_sets_plan(s.h, &p, &n[0])
	plan := C.GoString(p)
	runtime.KeepAlive(s)
	return plan, [3]uint64{uint64(n[0]), uint64(n[1]), uint64(n[2])}
}
