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

// ---- clusters of a neighbour graph: connected components and greedy representatives --------------------------------------
//
// h, _ := a.Neighbors(nil, 0, NeighborParams{JaccardNum: 1, JaccardDen: 2, Upper: true}, nil) leaves the pairs above the
// threshold on the device; h.Cluster(ClusterParams{Method: ClusterGreedy}, sizes, nil) turns them into clusters with one
// representative each.  Only the labels cross the link.

// ClusterMethod selects how bsk_hits_cluster groups the nodes.
type ClusterMethod uint32

const (
	ClusterComponents ClusterMethod = C.BSK_CLUSTER_COMPONENTS // connected components; the member of best rank represents
	ClusterGreedy     ClusterMethod = C.BSK_CLUSTER_GREEDY     // by ascending rank: join the best representative neighbour, or become one
)

// ClusterParams is bsk_cluster_params.
type ClusterParams struct {
	Method ClusterMethod
}

// Clusters is the result of (*Hits).Cluster: label[n], rep[clusters] ascending, offsets[clusters+1] and members[n] on the device.
type Clusters struct {
	eng *Engine
	h   *C.bsk_clusters
}

// ClustersInfo is what bsk_clusters_info reports.
type ClustersInfo struct {
	Items, Clusters, Largest uint64
}

// Cluster reads the hits as an undirected graph over their queries and clusters it (bsk_hits_cluster).  score: one value per
// query, higher is better, ties to the smaller index; nil: index order.  reuse: nil, or the Clusters of an earlier call on this
// engine, whose device arrays are kept and only grow.
func (h *Hits) Cluster(p ClusterParams, score []uint64, reuse *Clusters) (*Clusters, error) {
	if score != nil {
		if n, _ := h.Info(); uint64(len(score)) != n {
			return nil, errors.New("Cluster: score must hold one value per query")
		}
	}
	if reuse == nil {
		reuse = &Clusters{eng: h.eng}
		runtime.SetFinalizer(reuse, func(r *Clusters) { C.bsk_clusters_release(r.h) })
	}
	cp := C.bsk_cluster_params{method: C.uint32_t(p.Method)}
	var sp *C.uint64_t
	if len(score) > 0 {
		sp = (*C.uint64_t)(unsafe.Pointer(&score[0]))
	}
	rc := C.bsk_hits_cluster(h.eng.ctx, h.h, &cp, sp, &reuse.h)
	runtime.KeepAlive(h)
	runtime.KeepAlive(score)
	return reuse, h.eng.err(rc)
}

// Info: nodes, clusters and the size of the largest cluster (bsk_clusters_info).
func (r *Clusters) Info() ClustersInfo {
	var n, k, l C.uint64_t
	C.bsk_clusters_info(r.h, &n, &k, &l)
	runtime.KeepAlive(r)
	return ClustersInfo{uint64(n), uint64(k), uint64(l)}
}

// Plan: what ran, the rounds the host drove and the hits off the diagonal (bsk_clusters_plan).
func (r *Clusters) Plan() (plan string, rounds, edges uint64) {
	var p *C.char
	var f [2]C.uint64_t
	C.bsk_clusters_plan(r.h, &p, &f[0])
	runtime.KeepAlive(r)
	return C.GoString(p), uint64(f[0]), uint64(f[1])
}

// Fetch copies the clusters to the host (bsk_clusters_fetch): the cluster of every node, the representatives ascending, and the
// members of cluster k in members[offsets[k]:offsets[k+1]], ascending.
func (r *Clusters) Fetch() (label, rep []uint32, offsets []uint64, members []uint32, err error) {
	inf := r.Info()
	label, rep = make([]uint32, inf.Items+1), make([]uint32, inf.Clusters+1)
	offsets, members = make([]uint64, inf.Clusters+1), make([]uint32, inf.Items+1)
	rc := C.bsk_clusters_fetch(r.eng.ctx, r.h, (*C.uint32_t)(unsafe.Pointer(&label[0])), (*C.uint32_t)(unsafe.Pointer(&rep[0])),
		(*C.uint64_t)(unsafe.Pointer(&offsets[0])), (*C.uint32_t)(unsafe.Pointer(&members[0])))
	runtime.KeepAlive(r)
	return label[:inf.Items], rep[:inf.Clusters], offsets, members[:inf.Items], r.eng.err(rc)
}

// DevicePointers of the clusters: label[n], rep[clusters] (u32), offsets[clusters+1] (u64), members[n] (u32) (bsk_clusters_device).
func (r *Clusters) DevicePointers() (label, rep, offsets, members unsafe.Pointer) {
	var l, p, m *C.uint32_t
	var o *C.uint64_t
	C.bsk_clusters_device(r.h, &l, &p, &o, &m)
	runtime.KeepAlive(r)
	return unsafe.Pointer(l), unsafe.Pointer(p), unsafe.Pointer(o), unsafe.Pointer(m)
}

// Release frees the device arrays now instead of at garbage collection (bsk_clusters_release).
func (r *Clusters) Release() {
	C.bsk_clusters_release(r.h)
	r.h = nil
}

// HitsFromHost uploads hits made elsewhere (ANI, alignments) as CSR: offsets[n+1] from 0, targets strictly ascending inside a row,
// shared[], and total[] or nil for hits without totals (bsk_hits_from_host).  reuse: nil, or any Hits of this engine.
func (e *Engine) HitsFromHost(offsets []uint64, target, shared, total []uint32, reuse *Hits) (*Hits, error) {
	if len(offsets) == 0 || offsets[len(offsets)-1] != uint64(len(target)) || len(shared) != len(target) || (total != nil && len(total) != len(target)) {
		return nil, errors.New("HitsFromHost: offsets must have n+1 entries and end at len(target) == len(shared)")
	}
	if reuse == nil {
		reuse = &Hits{eng: e}
		runtime.SetFinalizer(reuse, func(h *Hits) { C.bsk_hits_release(h.h) })
	}
	var tp, sp, op *C.uint32_t
	if len(target) > 0 {
		tp, sp = (*C.uint32_t)(unsafe.Pointer(&target[0])), (*C.uint32_t)(unsafe.Pointer(&shared[0]))
		if total != nil {
			op = (*C.uint32_t)(unsafe.Pointer(&total[0]))
		}
	}
	rc := C.bsk_hits_from_host(e.ctx, (*C.uint64_t)(unsafe.Pointer(&offsets[0])), C.uint64_t(len(offsets)-1), tp, sp, op, &reuse.h)
	runtime.KeepAlive(offsets)
	runtime.KeepAlive(target)
	runtime.KeepAlive(shared)
	runtime.KeepAlive(total)
	return reuse, e.err(rc)
}
