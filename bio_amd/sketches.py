"""Host-side mirror of the reference ``sketches`` package over the C ABI.

Same names, argument order and error behaviour as shenwei356/bio ``sketches``
(file:line relative to the reference root):

    NewHashIterator(s, k, canonical, circular)      iterator.go:615   -> Iterator.NextHash()   :658
    NewKmerIterator(s, k, canonical, circular)      iterator.go:668   -> Iterator.NextKmer()   :708
    NewSimHashIterator(s, k, m, scale, canon, circ) iterator.go:113   -> Iterator.NextSimHash():191
    NewMinimizerSketch(S, k, w, circular)           sketch.go:85      -> Sketch.NextMinimizer():205
    NewSyncmerSketch(S, k, s, circular)             sketch.go:142     -> Sketch.NextSyncmer()  :312
    NewProteinIterator(s, k, codonTable, frame)     iterator-protein.go:46 -> ProteinIterator.Next() :76
    NewProteinMinimizerSketch(S, k, table, frame, w) sketch-protein.go:62  -> ProteinMinimizerSketch.Next() :106
    Index() on all four types                       iterator.go:776, sketch.go:488, ...

Constructors return ``(obj, err)`` Go-style; ``err`` is one of the sentinel
objects below (compare with ``is``).  The device works on batches: the fast path
is ``Engine.batch(...)`` + ``Engine.run(...)`` whose ``BatchResult.iterator(i)``
hands out the same cursor types; the single-sequence constructors run a batch of
one on the GPU so that code written against the reference keeps working.

Everything computes on the MI355X through libbiosketch.so -- there is no Python
or CPU implementation here.
"""
from __future__ import annotations

import ctypes as C
import fractions
import math
import os
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L


# ---- sentinel errors (iterator.go:34-53, sketch.go:32-42) ------------------------------------
class SketchError(Exception):
    def __init__(self, code: int, msg: str):
        super().__init__(msg)
        self.code = code


ErrInvalidK = SketchError(L.ERR_INVALID_K, "sketches: invalid k-mer size")
ErrEmptySeq = SketchError(L.ERR_EMPTY_SEQ, "sketches: empty sequence")
ErrShortSeq = SketchError(L.ERR_SHORT_SEQ, "sketches: sequence too short")
ErrIllegalBase = SketchError(L.ERR_ILLEGAL_BASE, "sketches: illegal base")
ErrKTooLarge = SketchError(L.ERR_K_TOO_LARGE, "sketches: k-mer size is too large")
ErrInvalidM = SketchError(L.ERR_INVALID_M, "sketches: invalid m-mer size, should be in range of [4, k]")
ErrInvalidScale = SketchError(L.ERR_INVALID_SCALE, "sketches: invalid scale, should be in range of [1, k-m+1]")
ErrInvalidS = SketchError(L.ERR_INVALID_S, "kmers: invalid s-mer size")
ErrInvalidW = SketchError(L.ERR_INVALID_W, "kmers: invalid minimimzer window")
ErrBufNil = SketchError(L.ERR_BUF_NIL, "kmers: buffer slice is nil")
ErrBufNotEmpty = SketchError(L.ERR_BUF_NOT_EMPTY, "kmers: buffer has elements")
_SENTINELS = {e.code: e for e in (ErrInvalidK, ErrEmptySeq, ErrShortSeq, ErrIllegalBase, ErrKTooLarge, ErrInvalidM,
                                  ErrInvalidScale, ErrInvalidS, ErrInvalidW, ErrBufNil, ErrBufNotEmpty)}


class DeviceError(RuntimeError):
    """Non-sentinel failure of the engine (device, memory, unsupported)."""


# ---- seq.Seq stand-in (seq/seq.go:29-34): only Alphabet identity and the byte slice cross the boundary
class Alphabet:
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return self.name


DNA = Alphabet("DNA")
DNAredundant = Alphabet("DNAredundant")
RNA = Alphabet("RNA")
RNAredundant = Alphabet("RNAredundant")
Protein = Alphabet("Protein")
Unlimit = Alphabet("Unlimit")


def _alpha_code(a: Alphabet) -> int:
    """bsk_alphabet of a Seq's Alphabet: the nucleotide alphabets differ only in the letters RevComInplace pairs (iterator.go:719)."""
    return {DNA: L.ALPHA_DNA_PLAIN, RNA: L.ALPHA_RNA, RNAredundant: L.ALPHA_RNA_REDUNDANT, Unlimit: L.ALPHA_UNLIMIT,
            Protein: L.ALPHA_PROTEIN}.get(a, L.ALPHA_DNA)


class Seq:
    def __init__(self, alphabet: Alphabet, seq):
        self.Alphabet = alphabet
        self.Seq = seq.encode() if isinstance(seq, str) else bytes(seq)


def NewSeq(alphabet: Alphabet, seq) -> Tuple[Seq, None]:
    return Seq(alphabet, seq), None


# ---- engine ---------------------------------------------------------------------------------------
class _Owner:
    """Owns one library handle: close() hands it to the library's release function once, and so does garbage collection."""

    _release = ""  # the release function's name
    _slot = "h"    # the attribute that holds the handle

    def close(self):
        h = getattr(self, self._slot, None)  # (None as well when the constructor failed before it had a handle)
        if h:
            getattr((getattr(self, "eng", None) or self).lib, self._release)(h)
            setattr(self, self._slot, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _take_over(eng: "Engine", into, call):
    """call(byref(slot)) with the handle of `into` -- None, or any owner with an .h to re-use -- in the slot -> the slot's handle.
    into.h follows the slot before the return code raises: kept where the library refuses the call before it takes the object
    over, None where it released it (include/biosketch.h, "The result slot")."""
    h = into.h if into is not None and into.h else C.c_void_p()
    rc = call(C.byref(h))
    if into is not None:
        into.h = h if h.value else None
        if isinstance(into, Sets) and (rc == L.OK or not h.value):  # written or released: not what a result bound to it has seen
            into._gen += 1
    eng._chk(rc)
    return h


def _same_sets(sets, gens, what: str):
    """the norms of a weighted result are those of its operands as the call saw them: fetched lazily, so only while the operands are unwritten"""
    if any(x._gen != g for x, g in zip(sets, gens)):
        raise ValueError(what + ": the operand sets were written or closed since the call; ask a formula before that (its norms are then kept)")


def _chk_pipeline(lib, what: str, rc: int):
    if rc != L.OK:
        raise _SENTINELS.get(rc) or DeviceError(f"{what}: {lib.bsk_err_name(rc).decode()}")


class Batch(_Owner):
    _release = "bsk_batch_destroy"

    def __init__(self, eng: "Engine", handle):
        self.eng, self.h = eng, handle

    def info(self):
        v = [C.c_uint64() for _ in range(4)]
        self.eng._chk(self.eng.lib.bsk_batch_info(self.h, *[C.byref(x) for x in v]))
        return dict(n_reads=v[0].value, n_bases=v[1].value, device_bytes=v[2].value, n_non_acgt_reads=v[3].value)

    def fetch_ascii(self, first: int, count: int) -> Tuple[np.ndarray, np.ndarray]:
        inf = self.info()
        cap = inf["n_bases"] if count == inf["n_reads"] else None
        offs = np.zeros(count + 1, np.uint64)
        if cap is None:  # two-step: sizes first via a generous bound
            cap = inf["n_bases"]
        buf = np.zeros(max(int(cap), 1), np.uint8)
        self.eng._chk(self.eng.lib.bsk_batch_fetch_ascii(self.eng.ctx, self.h, first, count, buf.ctypes.data, buf.size,
                                                         offs.ctypes.data))
        return buf[: int(offs[-1])].copy(), offs

    def translate(self, codon_table: int = 1, frame: int = 1) -> "Batch":
        """(*seq.Seq).Translate(table, frame, false, false, true, false) of every sequence (seq/seq.go:685) -> protein batch."""
        h = C.c_void_p()
        self.eng._chk(self.eng.lib.bsk_batch_translate(self.eng.ctx, self.h, codon_table, frame, C.byref(h)))
        return Batch(self.eng, h)

    def _refill(self, call):
        """call(byref(slot)) with this batch's handle in the slot; the object follows the slot (NULL after a refused call)"""
        h = self.h if self.h else C.c_void_p()
        self.eng._opts()
        rc = call(C.byref(h))
        self.h = h if h.value else None
        self.eng._chk(rc)
        return self

    def refill(self, data: np.ndarray, offsets: np.ndarray, alphabet: int = L.ALPHA_DNA) -> "Batch":
        """bsk_batch_refill_ascii: Engine.batch_from_arrays into THIS object -- its device buffers are kept and only grow, the old contents are gone"""
        data = np.ascontiguousarray(data, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        return self._refill(lambda slot: self.eng.lib.bsk_batch_refill_ascii(self.eng.ctx, slot, data.ctypes.data, offsets.ctypes.data, len(offsets) - 1, alphabet))

    def refill_packed(self, words: np.ndarray, desc: np.ndarray) -> "Batch":
        """bsk_batch_refill_packed: Engine.batch_from_packed into THIS object"""
        words = np.ascontiguousarray(words, np.uint32)
        desc = np.ascontiguousarray(desc, np.uint64)
        return self._refill(lambda slot: self.eng.lib.bsk_batch_refill_packed(self.eng.ctx, slot, words.ctypes.data, len(words), desc.ctypes.data, len(desc)))


class BatchResult(_Owner):
    """Device-resident CSR result of one bsk_sketch call."""

    _release = "bsk_result_release"

    def __init__(self, eng: "Engine", handle, params: L.Params):
        self.eng, self.h, self.params = eng, handle, params
        self._host = None

    def info(self):
        n, t, hp = C.c_uint64(), C.c_uint64(), C.c_int()
        self.eng._chk(self.eng.lib.bsk_result_info(self.h, C.byref(n), C.byref(t), C.byref(hp)))
        return dict(n_reads=n.value, n_tuples=t.value, has_pos=bool(hp.value))

    def plan(self):
        """What ran: the kernel the planner launched for this result, its grid and wavefronts per CU (bsk_result_plan)."""
        name, grid, per_cu = C.c_char_p(), C.c_int(), C.c_int()
        self.eng._chk(self.eng.lib.bsk_result_plan(self.h, C.byref(name), C.byref(grid), C.byref(per_cu)))
        return dict(kernel=(name.value or b"").decode(), grid=grid.value, waves_per_cu=per_cu.value)

    def class_plan(self):
        """bsk_result_class_plan -> (classes besides the bulk, device ms of the passes that cut the batch)"""
        n, ms = C.c_int(), C.c_float()
        self.eng._chk(self.eng.lib.bsk_result_class_plan(self.h, C.byref(n), C.byref(ms)))
        return n.value, float(ms.value)

    def fetch(self, first: int = 0, count: Optional[int] = None):
        """-> (offsets[count+1] rebased, status[count], hash[T], pos[T] or None)"""
        inf = self.info()
        if count is None:
            count = inf["n_reads"] - first
        offs = np.zeros(count + 1, np.uint64)
        status = np.zeros(max(count, 1), np.uint8)
        self.eng._chk(self.eng.lib.bsk_result_fetch(self.eng.ctx, self.h, first, count, offs.ctypes.data,
                                                    status.ctypes.data, None, None, 0))
        T = int(offs[-1])
        hash_ = np.zeros(max(T, 1), np.uint64)
        pos = np.zeros(max(T, 1), np.uint32) if inf["has_pos"] else None
        self.eng._chk(self.eng.lib.bsk_result_fetch(self.eng.ctx, self.h, first, count, offs.ctypes.data,
                                                    status.ctypes.data, hash_.ctypes.data,
                                                    pos.ctypes.data if pos is not None else None, max(T, 1)))
        return offs, status[:count], hash_[:T], (pos[:T] if pos is not None else None)

    def fetch_status(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """bsk_result_fetch_status -> status[count]: the BSK_ST_* bytes of reads [first, first + count) alone"""
        if count is None:
            count = self.info()["n_reads"] - first
        status = np.zeros(max(count, 1), np.uint8)
        self.eng._chk(self.eng.lib.bsk_result_fetch_status(self.eng.ctx, self.h, first, count, status.ctypes.data))
        return status[:count]

    def device(self):
        """The result's own arrays ON THE DEVICE, valid until close() or the next run into this object (bsk_result_device, and
        bsk_result_device_wide for a result over tiles) -> dict(wide, refs, status, hash, pos, first, count): raw pointers, None where the
        layout has no such array -- refs for a wide result, first / count for the others, pos for the kinds with implicit positions."""
        refs, status, hash_, pos, first, count = (C.c_void_p() for _ in range(6))
        self.eng._chk(self.eng.lib.bsk_result_device(self.h, C.byref(refs), C.byref(status), C.byref(hash_), C.byref(pos)))
        self.eng._chk(self.eng.lib.bsk_result_device_wide(self.h, C.byref(first), C.byref(count)))
        return dict(wide=not refs.value, refs=refs.value, status=status.value, hash=hash_.value, pos=pos.value, first=first.value, count=count.value)

    def fetch_narrow(self, first: int = 0, count: Optional[int] = None):
        """bsk_result_fetch_narrow -> (offsets[count+1] u32, status[count], hash[T], pos[T] u16 (bit 15 = strand) or None)"""
        inf = self.info()
        if count is None:
            count = inf["n_reads"] - first
        offs = np.zeros(count + 1, np.uint32)
        status = np.zeros(max(count, 1), np.uint8)
        cap = max(int(inf["n_tuples"]), 1)
        hash_ = np.zeros(cap, np.uint64)
        pos = np.zeros(cap, np.uint16) if inf["has_pos"] else None
        nt = C.c_uint64()
        self.eng._chk(self.eng.lib.bsk_result_fetch_narrow(self.eng.ctx, self.h, first, count, offs.ctypes.data, status.ctypes.data, hash_.ctypes.data,
                                                           pos.ctypes.data if pos is not None else None, cap, C.byref(nt)))
        T = int(nt.value)
        return offs, status[:count], hash_[:T], (pos[:T] if pos is not None else None)

    def sets(self, whole_batch: bool = False, scale: int = 1):
        """Sorted distinct hash values per sequence (or of the whole batch), optionally FracMinHash-filtered
        (bsk_result_sets) -> (offsets[n_sets+1], values)."""
        h = C.c_void_p()
        self.eng._opts()
        self.eng._chk(self.eng.lib.bsk_result_sets(self.eng.ctx, self.h, L.SETS_WHOLE_BATCH if whole_batch else L.SETS_PER_SEQUENCE, scale,
                                                   C.byref(h)))
        try:
            ns, nv = C.c_uint64(), C.c_uint64()
            self.eng._chk(self.eng.lib.bsk_sets_info(h, C.byref(ns), C.byref(nv)))
            offs = np.zeros(ns.value + 1, np.uint64)
            vals = np.zeros(max(nv.value, 1), np.uint64)
            self.eng._chk(self.eng.lib.bsk_sets_fetch(self.eng.ctx, h, 0, ns.value, offs.ctypes.data, vals.ctypes.data, vals.size))
            return offs, vals[: nv.value]
        finally:
            self.eng.lib.bsk_sets_release(h)

    def device_sets(self, whole_batch: bool = False, scale: int = 1) -> "Sets":
        """The same sets as sets(), left ON THE DEVICE (bsk_result_sets) -> Sets: index them or search them without a round trip."""
        h = C.c_void_p()
        self.eng._opts()
        self.eng._chk(self.eng.lib.bsk_result_sets(self.eng.ctx, self.h, L.SETS_WHOLE_BATCH if whole_batch else L.SETS_PER_SEQUENCE, scale,
                                                   C.byref(h)))
        return Sets(self.eng, h)

    def counted_sets(self, whole_batch: bool = False, scale: int = 1, into: Optional["Sets"] = None) -> "Sets":
        """device_sets() with every value's abundance (bsk_result_sets_counted): counts[i] = how many tuples of the set's scope hold
        values[i].  into: a Sets of this engine to re-use (its device arrays are kept and only grow)."""
        self.eng._opts()
        scope = L.SETS_WHOLE_BATCH if whole_batch else L.SETS_PER_SEQUENCE
        h = _take_over(self.eng, into, lambda out: self.eng.lib.bsk_result_sets_counted(self.eng.ctx, self.h, scope, scale, out))
        if into is not None:
            into.group_offsets = None
        return into if into is not None else Sets(self.eng, h)

    def window_sets(self, window: int = 0, step: int = 0, count: int = 0, scale: int = 1, counted: bool = False, into: Optional["Sets"] = None) -> "Sets":
        """One set per window of every sequence's positions, left on the device (bsk_result_sets_windows): windows of `window` positions
        whose starts are `step` apart (0: no overlap), or -- count != 0 -- `count` windows per sequence, sized per sequence (kmcp's
        --split-number).  The windows of a sequence follow from its tuples, not from its length.  counted: every value with its run
        length inside the window.  into: a Sets of this engine to re-use.  The returned Sets carries .group_offsets, the host array
        [n_reads + 1] with window w of sequence i at set group_offsets[i] + w: the offsets that Sets.reduce and Hits.fold take."""
        self.eng._opts()
        wp = L.WindowParams(window, step, count, L.WINDOWS_COUNTED if counted else 0)
        go = np.zeros(self.info()["n_reads"] + 1, np.uint64)
        h = _take_over(self.eng, into, lambda out: self.eng.lib.bsk_result_sets_windows(self.eng.ctx, self.h, C.byref(wp), scale, out, go.ctypes.data))
        res = into if into is not None else Sets(self.eng, h)
        res.group_offsets = go
        return res

    def compact(self):
        """bsk_result_compact: dense CSR copy left ON THE DEVICE -> (offsets_ptr, hash_ptr, pos_ptr or None, n_tuples); the arrays belong
        to the engine's context until its next compact()."""
        po, ph, pp = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nt = C.c_uint64()
        self.eng._chk(self.eng.lib.bsk_result_compact(self.eng.ctx, self.h, C.byref(po), C.byref(ph), C.byref(pp), C.byref(nt)))
        return po.value, ph.value, pp.value, int(nt.value)

    def digest(self):
        ck, nt = C.c_uint64(), C.c_uint64()
        sc = (C.c_uint64 * 4)()
        self.eng._chk(self.eng.lib.bsk_result_digest(self.eng.ctx, self.h, C.byref(ck), C.byref(nt), sc))
        return dict(checksum=ck.value, n_tuples=nt.value, short=sc[0], illegal=sc[1], first_window_tie=sc[2],
                    has_non_acgt=sc[3])

    def _cache(self):
        if self._host is None:
            self._host = self.fetch()
        return self._host

    def read(self, i: int):
        """(status, hash[], pos[] or None) of read i -- what the reference iterator over read i yields."""
        offs, status, h, p = self._cache()
        a, b = int(offs[i]), int(offs[i + 1])
        return int(status[i]), h[a:b], (p[a:b] if p is not None else None)


class Sets(_Owner):
    """Device-resident sorted distinct value sets (bsk_sets): offsets[n_sets+1] and values[] stay on the device until close()."""

    _release = "bsk_sets_release"
    group_offsets = None  # BatchResult.window_sets: the sets' windows by sequence (host, [n_reads + 1]); None on sets from any other call
    _gen = 0  # the write generation: one more after every call that took this object over as its `into`, and after close()

    def __init__(self, eng: "Engine", handle):
        self.eng, self.h = eng, handle

    def close(self):
        self._gen += 1
        _Owner.close(self)

    def info(self):
        ns, nv = C.c_uint64(), C.c_uint64()
        self.eng._chk(self.eng.lib.bsk_sets_info(self.h, C.byref(ns), C.byref(nv)))
        return dict(n_sets=ns.value, n_values=nv.value)

    def offsets(self) -> np.ndarray:
        """offsets[n_sets+1] to the host (the sets' sizes are its differences)"""
        ns = self.info()["n_sets"]
        offs = np.zeros(ns + 1, np.uint64)
        self.eng._chk(self.eng.lib.bsk_sets_fetch(self.eng.ctx, self.h, 0, ns, offs.ctypes.data, None, 0))
        return offs

    def fetch(self):
        """bsk_sets_fetch -> (offsets[n_sets+1], values)"""
        inf = self.info()
        offs = np.zeros(inf["n_sets"] + 1, np.uint64)
        vals = np.zeros(max(inf["n_values"], 1), np.uint64)
        self.eng._chk(self.eng.lib.bsk_sets_fetch(self.eng.ctx, self.h, 0, inf["n_sets"], offs.ctypes.data, vals.ctypes.data, vals.size))
        return offs, vals[: inf["n_values"]]

    def device(self):
        """bsk_sets_device -> (offsets_ptr, values_ptr)"""
        po, pv = C.c_void_p(), C.c_void_p()
        self.eng._chk(self.eng.lib.bsk_sets_device(self.h, C.byref(po), C.byref(pv)))
        return po.value, pv.value

    def index(self) -> "Index":
        """Inverted index of these sets as search targets (bsk_index_build); the sets may be closed afterwards."""
        h = C.c_void_p()
        self.eng._chk(self.eng.lib.bsk_index_build(self.eng.ctx, self.h, C.byref(h)))
        return Index(self.eng, h, np.diff(self.offsets()))

    def index_counted(self) -> "Index":
        """index() with the sets' counts (bsk_index_build_counted): per posting the target's count of the value, per target the norms
        (Index.norms()); search it with Index.search_counted.  Sets without counts give an index without counts."""
        h = C.c_void_p()
        self.eng._chk(self.eng.lib.bsk_index_build_counted(self.eng.ctx, self.h, C.byref(h)))
        return Index(self.eng, h, np.diff(self.offsets()))

    # -- set algebra (bsk_sets_op / bsk_sets_reduce): the result is a Sets of the same engine, left on the device
    def _into(self, into: Optional["Sets"], call) -> "Sets":
        h = _take_over(self.eng, into, call)
        if into is not None:
            into.group_offsets = None  # (after the call: a refused call leaves the object, and its windows, as they were)
        return into if into is not None else Sets(self.eng, h)

    def op(self, other: "Sets", op: int, into: Optional["Sets"] = None) -> "Sets":
        """Set i of the result is self[i] op other[i]; an `other` of exactly one set is combined with every set of self (bsk_sets_op).
        into: the Sets of an earlier operation on this engine, whose device arrays are kept and only grow."""
        return self._into(into, lambda out: self.eng.lib.bsk_sets_op(self.eng.ctx, self.h, other.h, op, out))

    def union(self, other: "Sets", into: Optional["Sets"] = None) -> "Sets":
        return self.op(other, L.SETOP_UNION, into)

    def intersect(self, other: "Sets", into: Optional["Sets"] = None) -> "Sets":
        return self.op(other, L.SETOP_INTERSECT, into)

    def difference(self, other: "Sets", into: Optional["Sets"] = None) -> "Sets":
        """self[i] minus other[i]"""
        return self.op(other, L.SETOP_DIFF, into)

    def symmetric_difference(self, other: "Sets", into: Optional["Sets"] = None) -> "Sets":
        return self.op(other, L.SETOP_SYMDIFF, into)

    def reduce(self, group_offsets, min_members: int = 1, into: Optional["Sets"] = None) -> "Sets":
        """One set per run of consecutive sets (group g: sets group_offsets[g] .. group_offsets[g + 1] - 1): the values at least
        min_members of the run's sets hold -- 1: their union, L.MEMBERS_ALL: their intersection (bsk_sets_reduce)."""
        go = np.ascontiguousarray(group_offsets, np.uint64)
        if go.ndim != 1 or go.size == 0:
            raise ValueError("group_offsets: a one-dimensional array of n_groups + 1 entries")
        return self._into(into, lambda out: self.eng.lib.bsk_sets_reduce(self.eng.ctx, self.h, go.ctypes.data, go.size - 1, min_members, out))

    # -- counted sets (bsk_sets_*count*): values with their abundance
    @property
    def counted(self) -> bool:
        """whether the sets carry counts (bsk_sets_counts_device gives an array)"""
        p = C.c_void_p()
        self.eng._chk(self.eng.lib.bsk_sets_counts_device(self.h, C.byref(p)))
        return bool(p.value)

    def fetch_counts(self) -> np.ndarray:
        """bsk_sets_fetch_counts -> counts[n_values] (u32), parallel to fetch()'s values"""
        inf = self.info()
        c = np.zeros(max(inf["n_values"], 1), np.uint32)
        self.eng._chk(self.eng.lib.bsk_sets_fetch_counts(self.eng.ctx, self.h, 0, inf["n_sets"], c.ctypes.data, c.size))
        return c[: inf["n_values"]]

    def op_counted(self, other: "Sets", op: int, into: Optional["Sets"] = None) -> "Sets":
        """bsk_sets_op_counted: L.COUNTOP_ADD / KEEP / DROP; pairing as op(), and a self of one set is combined with every set of other"""
        return self._into(into, lambda out: self.eng.lib.bsk_sets_op_counted(self.eng.ctx, self.h, other.h, op, out))

    def add(self, other: "Sets", into: Optional["Sets"] = None) -> "Sets":
        """the union's values, counts added (saturating at 2^32 - 1)"""
        return self.op_counted(other, L.COUNTOP_ADD, into)

    def keep(self, other: "Sets", into: Optional["Sets"] = None) -> "Sets":
        """self's values that other holds, with self's counts"""
        return self.op_counted(other, L.COUNTOP_KEEP, into)

    def drop(self, other: "Sets", into: Optional["Sets"] = None) -> "Sets":
        """self's values that other does not hold, with self's counts"""
        return self.op_counted(other, L.COUNTOP_DROP, into)

    def filter_counts(self, min_count: int = 1, max_count: Optional[int] = None, into: Optional["Sets"] = None) -> "Sets":
        """the values with min_count <= count <= max_count (None: no upper bound) and their counts (bsk_sets_filter_counts)"""
        hi = 0xFFFFFFFF if max_count is None else max_count
        return self._into(into, lambda out: self.eng.lib.bsk_sets_filter_counts(self.eng.ctx, self.h, min_count, hi, out))

    def totals(self) -> np.ndarray:
        """per set the sum of its counts, u64 (bsk_sets_totals); the sets' sizes for sets without counts"""
        ns = self.info()["n_sets"]
        t = np.zeros(max(ns, 1), np.uint64)
        self.eng._chk(self.eng.lib.bsk_sets_totals(self.eng.ctx, self.h, 0, ns, t.ctypes.data))
        return t[:ns]

    def sumsq(self) -> np.ndarray:
        """per set the sum of its squared counts, u64, saturating at 2^64 - 1 (bsk_sets_sumsq): the squared norm of the abundance
        vector; the sets' sizes for sets without counts"""
        ns = self.info()["n_sets"]
        t = np.zeros(max(ns, 1), np.uint64)
        self.eng._chk(self.eng.lib.bsk_sets_sumsq(self.eng.ctx, self.h, 0, ns, t.ctypes.data))
        return t[:ns]

    # -- MinHash (bsk_sets_bottom / bsk_sets_compare)
    def bottom(self, n: int, into: Optional["Sets"] = None) -> "Sets":
        """Every set cut to its min(n, size) smallest values, counts included when the sets are counted (bsk_sets_bottom): the
        fixed-size MinHash sketch.  into as in op()."""
        return self._into(into, lambda out: self.eng.lib.bsk_sets_bottom(self.eng.ctx, self.h, n, out))

    def compare(self, other: Optional["Sets"] = None, limit: int = 0, reuse: Optional["Compare"] = None) -> "Compare":
        """Every set of self against every set of other (None: of self): per pair the first `limit` distinct values of the union
        (0: all of them) and how many of those both sets hold (bsk_sets_compare).  limit 0 gives the exact Jaccard, limit n the
        Mash estimator of bottom-n sketches.  reuse: the Compare of an earlier call on this engine, whose device arrays are kept."""
        other = self if other is None else other
        h = _take_over(self.eng, reuse, lambda out: self.eng.lib.bsk_sets_compare(self.eng.ctx, self.h, other.h, limit, out))
        res = reuse if reuse is not None else Compare(self.eng)
        res._bind(h, np.diff(self.offsets()))
        return res

    def compare_counted(self, other: Optional["Sets"] = None, limit: int = 0, reuse: Optional["Compare"] = None) -> "Compare":
        """compare() with the counts (bsk_sets_compare_counted): shared and total as compare() gives them, and over the walked values
        both sets hold dot = the sum of the products of the two counts (u64, saturating) and min_sum = the sum of their minima.
        Sets without counts count 1 for every value.  The Compare keeps both operands for its norms (cosine() and its kin)."""
        other = self if other is None else other
        h = _take_over(self.eng, reuse, lambda out: self.eng.lib.bsk_sets_compare_counted(self.eng.ctx, self.h, other.h, limit, out))
        res = reuse if reuse is not None else Compare(self.eng)
        res._bind(h, np.diff(self.offsets()), (self, other))
        return res

    def neighbors(self, other: Optional["Sets"] = None, limit: int = 0, min_shared: int = 1, min_jaccard=None, upper: bool = False,
                  reuse: Optional["Hits"] = None) -> "Hits":
        """compare() without the matrix (bsk_sets_neighbors): per set of self the sets of other (None: of self) that share at least
        max(min_shared, 1) of the walked values and, with min_jaccard, have shared / total >= it -- a (num, den) pair of integers,
        compared exactly, or a float x in 0..1 taken as (ceil(x * 2^30), 2^30).  upper: only pairs with j > i (self against itself:
        every unordered pair once, the lower triangle never computed).  -> Hits with .total; any number of cells.  reuse: any Hits
        of this engine, whose device arrays are kept."""
        return self._neighbors(other, limit, min_shared, min_jaccard, upper, reuse, False)

    def neighbors_counted(self, other: Optional["Sets"] = None, limit: int = 0, min_shared: int = 1, min_jaccard=None, upper: bool = False,
                          reuse: Optional["Hits"] = None) -> "Hits":
        """neighbors() with the counts (bsk_sets_neighbors_counted): the same pairs, offsets, targets, shared and totals -- the
        thresholds read shared and total only -- and per kept pair .dot and .min_sum as compare_counted() defines them.  Sets without
        counts count 1 for every value.  The Hits keep both operands for their norms (cosine() and its kin)."""
        return self._neighbors(other, limit, min_shared, min_jaccard, upper, reuse, True)

    def _neighbors(self, other, limit, min_shared, min_jaccard, upper, reuse, counted):
        other = self if other is None else other
        num, den = 0, 0
        if min_jaccard is not None:
            if isinstance(min_jaccard, tuple):
                num, den = int(min_jaccard[0]), int(min_jaccard[1])
            else:
                x = float(min_jaccard)
                if not 0.0 <= x <= 1.0:
                    raise ValueError("min_jaccard outside 0..1")
                num, den = int(math.ceil(x * (1 << 30))), 1 << 30
        np_ = L.NeighborParams(min_shared, L.NEIGHBORS_UPPER if upper else 0, num, den)
        entry = self.eng.lib.bsk_sets_neighbors_counted if counted else self.eng.lib.bsk_sets_neighbors
        h = _take_over(self.eng, reuse, lambda out: entry(self.eng.ctx, self.h, other.h, limit, C.byref(np_), out))
        res = reuse if reuse is not None else Hits(self.eng)
        res._bind(h, np.diff(self.offsets()), np.diff(other.offsets()), (self, other, limit) if counted else None)
        return res

    def plan(self):
        """What made these sets (bsk_sets_plan): a description and the pairs of the last op() that took the group, wave and tiled
        path; sets of any other origin report an empty string and zeros."""
        p, n = C.c_char_p(), (C.c_uint64 * 3)()
        self.eng._chk(self.eng.lib.bsk_sets_plan(self.h, C.byref(p), n))
        return dict(plan=(p.value or b"").decode(), n_by_path=[int(n[0]), int(n[1]), int(n[2])])


class Compare(_Owner):
    """Dense all-pairs comparison (bsk_compare): shared[n_a, n_b] and total[n_a, n_b] (u32), fetched on first use; after
    Sets.compare_counted also dot[n_a, n_b] and min_sum[n_a, n_b] (u64)."""

    _release = "bsk_compare_release"
    _whost = _norms = _operands = _gens = None  # the weighted side: (dot, min_sum); (sumsq_a, sumsq_b, totals_a, totals_b); the two Sets; their generations at bind time

    def __init__(self, eng: "Engine"):
        self.eng, self.h = eng, None
        self._host = None

    def _bind(self, h, a_sizes: np.ndarray, operands=None):
        self.h, self._host = h, None
        self.a_sizes = a_sizes.astype(np.uint64)
        self._whost, self._norms, self._operands = None, None, operands
        self._gens = None if operands is None else tuple(x._gen for x in operands)

    def info(self):
        na, nb, lim = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.eng._chk(self.eng.lib.bsk_compare_info(self.h, C.byref(na), C.byref(nb), C.byref(lim)))
        return dict(n_a=na.value, n_b=nb.value, limit=lim.value)

    def plan(self):
        """What the comparison ran (bsk_compare_plan): a description, the tiles run, the rounds summed over them, the most of one tile."""
        p, n = C.c_char_p(), (C.c_uint64 * 3)()
        self.eng._chk(self.eng.lib.bsk_compare_plan(self.h, C.byref(p), n))
        return dict(plan=(p.value or b"").decode(), tiles=int(n[0]), rounds=int(n[1]), max_rounds=int(n[2]))

    def device(self):
        """bsk_compare_device -> (shared_ptr, total_ptr)"""
        ps, pt = C.c_void_p(), C.c_void_p()
        self.eng._chk(self.eng.lib.bsk_compare_device(self.h, C.byref(ps), C.byref(pt)))
        return ps.value, pt.value

    def fetch(self, first_row: int = 0, n_rows: Optional[int] = None):
        """bsk_compare_fetch -> (shared[n_rows, n_b], total[n_rows, n_b])"""
        inf = self.info()
        if n_rows is None:
            n_rows = inf["n_a"] - first_row
        cells = max(n_rows, 0) * inf["n_b"]
        sh, tt = np.zeros(max(cells, 1), np.uint32), np.zeros(max(cells, 1), np.uint32)
        self.eng._chk(self.eng.lib.bsk_compare_fetch(self.eng.ctx, self.h, first_row, n_rows, sh.ctypes.data, tt.ctypes.data, cells))
        return sh[:cells].reshape(n_rows, inf["n_b"]), tt[:cells].reshape(n_rows, inf["n_b"])

    def _cache(self):
        if self._host is None:
            self._host = self.fetch()
        return self._host

    @property
    def shared(self) -> np.ndarray:
        return self._cache()[0]

    @property
    def total(self) -> np.ndarray:
        return self._cache()[1]

    def jaccard(self) -> np.ndarray:
        """shared / total as float64, 0.0 where total == 0"""
        s, t = self.shared.astype(np.float64), self.total.astype(np.float64)
        return np.divide(s, t, out=np.zeros_like(s), where=t != 0)

    def containment(self) -> np.ndarray:
        """shared / |a[i]| (0.0 for an empty a[i]); whole sets only: limit == 0"""
        if self.info()["limit"] != 0:
            raise ValueError("containment is defined on whole sets: compare with limit=0")
        s = self.shared.astype(np.float64)
        q = np.broadcast_to(self.a_sizes.astype(np.float64)[:, None], s.shape)
        return np.divide(s, q, out=np.zeros_like(s), where=q != 0)

    def mash_distance(self, k: int) -> np.ndarray:
        """1.0 where the Jaccard j is 0, elsewhere max(0, -ln(2j / (1 + j)) / k)"""
        j = self.jaccard()
        d = np.ones_like(j)
        nz = j > 0
        d[nz] = np.maximum(0.0, -np.log(2.0 * j[nz] / (1.0 + j[nz])) / k)
        return d

    # -- the weighted side (bsk_sets_compare_counted)
    @property
    def weighted(self) -> bool:
        """whether the last compare into this object kept dot and min_sum (bsk_compare_weights_device gives arrays)"""
        if not self.h:
            return self._whost is not None
        pd, pm = C.c_void_p(), C.c_void_p()
        self.eng._chk(self.eng.lib.bsk_compare_weights_device(self.h, C.byref(pd), C.byref(pm)))
        return bool(pd.value) and bool(pm.value)

    def fetch_weights(self, first_row: int = 0, n_rows: Optional[int] = None):
        """bsk_compare_fetch_weights -> (dot[n_rows, n_b], min_sum[n_rows, n_b]) u64; an unweighted result raises"""
        inf = self.info()
        if n_rows is None:
            n_rows = inf["n_a"] - first_row
        cells = max(n_rows, 0) * inf["n_b"]
        dt, ms = np.zeros(max(cells, 1), np.uint64), np.zeros(max(cells, 1), np.uint64)
        self.eng._chk(self.eng.lib.bsk_compare_fetch_weights(self.eng.ctx, self.h, first_row, n_rows, dt.ctypes.data, ms.ctypes.data, cells))
        return dt[:cells].reshape(n_rows, inf["n_b"]), ms[:cells].reshape(n_rows, inf["n_b"])

    def _wcache(self):
        if self._whost is None:
            if not self.weighted:
                raise ValueError("not a weighted result: use Sets.compare_counted")
            self._whost = self.fetch_weights()
        return self._whost

    @property
    def dot(self) -> np.ndarray:
        return self._wcache()[0]

    @property
    def min_sum(self) -> np.ndarray:
        return self._wcache()[1]

    def _whole(self, what: str):
        """(dot, min_sum, sumsq_a, sumsq_b, totals_a, totals_b) of a weighted result over whole sets"""
        dt, ms = self._wcache()
        if self.info()["limit"] != 0:
            raise ValueError(what + " is defined on whole sets: compare_counted with limit=0")
        if self._norms is None:
            a, b = self._operands
            _same_sets((a, b), self._gens, what)
            qa, ta = a.sumsq(), a.totals()
            qb, tb = (qa, ta) if b is a else (b.sumsq(), b.totals())
            self._norms = (qa, qb, ta, tb)
        return (dt, ms) + tuple(self._norms)

    def cosine(self) -> np.ndarray:
        """dot / (sqrt(sumsq_a[i]) * sqrt(sumsq_b[j])) as float64: 0.0 where a norm is 0, NaN where dot or either norm is saturated"""
        dt, _, qa, qb, _, _ = self._whole("cosine")
        top = int(np.iinfo(np.uint64).max)
        den = np.sqrt(qa.astype(np.float64))[:, None] * np.sqrt(qb.astype(np.float64))[None, :]
        cos = np.divide(dt.astype(np.float64), den, out=np.zeros(dt.shape, np.float64), where=den != 0)
        cos[(dt == top) | (qa == top)[:, None] | (qb == top)[None, :]] = np.nan
        return cos

    def angular_similarity(self) -> np.ndarray:
        """1 - 2 acos(min(cosine, 1)) / pi: what sourmash compare reports for signatures with abundance"""
        return 1.0 - 2.0 * np.arccos(np.minimum(self.cosine(), 1.0)) / np.pi

    def weighted_jaccard(self) -> np.ndarray:
        """min_sum / (totals_a[i] + totals_b[j] - min_sum) -- the sum of minima over the sum of maxima -- 0.0 where that is 0"""
        _, ms, _, _, ta, tb = self._whole("weighted_jaccard")
        m = ms.astype(np.float64)
        den = ta.astype(np.float64)[:, None] + tb.astype(np.float64)[None, :] - m
        return np.divide(m, den, out=np.zeros_like(m), where=den != 0)

    def bray_curtis(self) -> np.ndarray:
        """1 - 2 min_sum / (totals_a[i] + totals_b[j]) (the dissimilarity), 0.0 where the denominator is 0"""
        _, ms, _, _, ta, tb = self._whole("bray_curtis")
        m = ms.astype(np.float64)
        den = ta.astype(np.float64)[:, None] + tb.astype(np.float64)[None, :]
        out, nz = np.zeros_like(m), den != 0
        out[nz] = 1.0 - 2.0 * m[nz] / den[nz]
        return out


class Index(_Owner):
    """Device-resident inverted index of target sets (bsk_index): value -> ascending target ids."""

    _release = "bsk_index_release"

    def __init__(self, eng: "Engine", handle, target_sizes: np.ndarray, norms=None):
        self.eng, self.h = eng, handle
        self.target_sizes = np.asarray(target_sizes, np.uint64)
        self._norms = norms  # (sumsq, totals) once norms() has fetched them; an attached handle inherits them

    def info(self):
        v = [C.c_uint64() for _ in range(5)]
        self.eng._chk(self.eng.lib.bsk_index_info(self.h, *[C.byref(x) for x in v]))
        return dict(n_targets=v[0].value, n_postings=v[1].value, n_distinct=v[2].value, max_bucket=v[3].value, device_bytes=v[4].value)

    def search(self, queries: Sets, min_shared: int = 1, min_query_cov: float = 0.0, min_target_cov: float = 0.0,
               reuse: Optional["Hits"] = None) -> "Hits":
        """Every (query, target) pair that shares s values with s >= max(min_shared, 1), s >= min_query_cov * |q| and
        s >= min_target_cov * |t| (bsk_index_search).  reuse: the Hits of an earlier search, whose device arrays are kept."""
        sp = L.SearchParams(min_shared, 0, min_query_cov, min_target_cov)
        h = _take_over(self.eng, reuse, lambda out: self.eng.lib.bsk_index_search(self.eng.ctx, self.h, queries.h, C.byref(sp), out))
        res = reuse if reuse is not None else Hits(self.eng)
        res._bind(h, np.diff(queries.offsets()), self.target_sizes)
        return res

    @property
    def counted(self) -> bool:
        """whether the index keeps counts (bsk_index_counted): built by Sets.index_counted from counted sets"""
        k = C.c_int()
        self.eng._chk(self.eng.lib.bsk_index_counted(self.h, C.byref(k)))
        return bool(k.value)

    def norms(self):
        """(sumsq, totals) of the targets, u64 each (bsk_index_fetch_norms), fetched once: what Sets.sumsq() and Sets.totals() gave for the
        sets the index was built from; the targets' sizes for an index without counts"""
        if self._norms is None:
            n = self.info()["n_targets"]
            q, t = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
            self.eng._chk(self.eng.lib.bsk_index_fetch_norms(self.eng.ctx, self.h, 0, n, q.ctypes.data, t.ctypes.data))
            self._norms = (q[:n], t[:n])
        return self._norms

    def search_counted(self, queries: Sets, min_shared: int = 1, min_query_cov: float = 0.0, min_target_cov: float = 0.0,
                       reuse: Optional["Hits"] = None) -> "Hits":
        """search() with the counts (bsk_index_search_counted): the same hits, bit for bit -- the thresholds read shared only -- and per
        hit .dot and .min_sum over the values both sets hold, as Sets.compare_counted defines them with limit 0.  Queries or an index
        without counts count 1 for every value.  The Hits are bound to the queries' sumsq() and totals() and the index's norms() -- fetched
        when a formula first asks for them, which raises ValueError once the queries were written or closed or this handle was closed -- so cosine() and its kin work without the target sets; against an index without counts weighted_containment() is the share of
        the query's mass found.  reuse: any Hits of this engine, whose device arrays are kept."""
        sp = L.SearchParams(min_shared, 0, min_query_cov, min_target_cov)
        h = _take_over(self.eng, reuse, lambda out: self.eng.lib.bsk_index_search_counted(self.eng.ctx, self.h, queries.h, C.byref(sp), out))
        res = reuse if reuse is not None else Hits(self.eng)
        res._bind(h, np.diff(queries.offsets()), self.target_sizes)

        def source():  # fetched when a formula first asks
            if self._norms is None and not self.h:
                raise ValueError("the index was closed since the call, before a formula fetched its norms")
            return queries.sumsq(), self.norms()[0], queries.totals(), self.norms()[1]

        res._norm_source = source
        res._gens = ((queries,), (queries._gen,))  # (the index's own norms cannot change)
        res._plain_targets = not self.counted
        return res

    def attach(self, engine: "Engine") -> "Index":
        """A handle on this index for another engine (bsk_index_attach): on the same device the arrays are shared, on another device
        they are copied there once.  Search it through the returned Index; the two may be closed in any order."""
        h = C.c_void_p()
        engine._chk(engine.lib.bsk_index_attach(engine.ctx, self.h, C.byref(h)))
        return Index(engine, h, self.target_sizes, self._norms)


class Hits(_Owner):
    """CSR hits of one search (bsk_hits): offsets[n_queries+1], target[] ascending inside a query, shared[]; fetched on first use."""

    _release = "bsk_hits_release"
    _totals = None  # total[] of hits with totals (Sets.neighbors), fetched with the others
    _members = None  # members[] of folded hits (Hits.fold), fetched with the others
    _weights = _norms = _operands = None  # the weighted side (Sets.neighbors_counted): (dot, min_sum), fetched with the others; (sumsq_a, sumsq_b, totals_a, totals_b); (a, b, limit)
    _plain_targets = None  # Index.search_counted: whether the index kept no counts (weighted_containment() is defined there); None for any other hits
    _norm_source = None  # Index.search_counted: () -> (sumsq_q, sumsq_t, totals_q, totals_t), from the queries and the index's own norms
    _gens = None  # (the Sets the norms will be fetched from, their generations at bind time): the norms are those of the call's operands
    _flip = None  # transpose(): (the _plain_targets of the hits this object is the transpose of,); None for hits in their own orientation

    def __init__(self, eng: "Engine"):
        self.eng, self.h = eng, None
        self._host = None

    def _bind(self, h, query_sizes: np.ndarray, target_sizes: np.ndarray, operands=None):
        self.h, self._host, self._totals, self._members = h, None, None, None
        self._weights, self._norms, self._operands, self._plain_targets, self._norm_source, self._flip = None, None, operands, None, None, None
        self._gens = None if operands is None else (operands[:2], tuple(x._gen for x in operands[:2]))
        self.query_sizes, self.target_sizes = query_sizes.astype(np.uint64), target_sizes

    def info(self):
        nq, nh = C.c_uint64(), C.c_uint64()
        self.eng._chk(self.eng.lib.bsk_hits_info(self.h, C.byref(nq), C.byref(nh)))
        return dict(n_queries=nq.value, n_hits=nh.value)

    def plan(self):
        """What the search ran (bsk_hits_plan): a description and how many queries took the large-query (sort) path."""
        p, n = C.c_char_p(), C.c_uint64()
        self.eng._chk(self.eng.lib.bsk_hits_plan(self.h, C.byref(p), C.byref(n)))
        return dict(plan=(p.value or b"").decode(), n_large_queries=n.value)

    def top(self, n: int, reuse: Optional["Hits"] = None) -> "Hits":
        """Every query's min(n, hits) best hits, largest shared count first, ties by ascending target (bsk_hits_top) -> Hits.
        reuse: the Hits of an earlier top() on this engine, whose device arrays are kept."""
        h = _take_over(self.eng, reuse, lambda out: self.eng.lib.bsk_hits_top(self.eng.ctx, self.h, n, out))
        res = reuse if reuse is not None else Hits(self.eng)
        res._bind(h, self.query_sizes, self.target_sizes)
        return res

    def fold(self, group_offsets, min_members: int = 1, min_fraction=None, reuse: Optional["Hits"] = None) -> "Hits":
        """The hits summed by target group (bsk_hits_fold) -> Hits whose targets are groups: group g is targets group_offsets[g] ..
        group_offsets[g + 1] - 1 (the chunks of a genome: Sets.group_offsets of BatchResult.window_sets).  Per row and group with a hit:
        shared summed (saturating), .members = how many of the group's targets the row hit.  A group is kept with at least min_members
        members and, with min_fraction = (num, den), members * den >= num * group_size.  The rows must list their targets strictly
        ascending (not the output of top()).  reuse: any Hits of this engine, but not self."""
        go = np.ascontiguousarray(group_offsets, np.uint64)
        if go.ndim != 1 or go.size == 0:
            raise ValueError("group_offsets: a one-dimensional array of n_groups + 1 entries")
        num, den = (0, 0) if min_fraction is None else (int(min_fraction[0]), int(min_fraction[1]))
        fp = L.FoldParams(min_members, 0, num, den)
        h = _take_over(self.eng, reuse, lambda out: self.eng.lib.bsk_hits_fold(self.eng.ctx, self.h, go.ctypes.data, go.size - 1, C.byref(fp), out))
        res = reuse if reuse is not None else Hits(self.eng)
        res._bind(h, self.query_sizes, np.diff(go))
        return res

    # -- selection by a measure (bsk_hits_filter, bsk_hits_top_by): every payload stays with its hit
    _MEASURES = {  # name -> (kind, which norms: None, "sizes", "sumsq", "totals"; which sides)
        "shared": (L.MEASURE_SHARED, None, ""), "members": (L.MEASURE_MEMBERS, None, ""), "dot": (L.MEASURE_DOT, None, ""), "min_sum": (L.MEASURE_MIN_SUM, None, ""),
        "query_cov": (L.MEASURE_QUERY_COV, "sizes", "q"), "target_cov": (L.MEASURE_TARGET_COV, "sizes", "t"), "jaccard": (L.MEASURE_JACCARD, "sizes", "qt"),
        "cosine": (L.MEASURE_COSINE, "sumsq", "qt"), "weighted_jaccard": (L.MEASURE_WEIGHTED_JACCARD, "totals", "qt"),
        "bray_curtis_similarity": (L.MEASURE_BC_SIMILARITY, "totals", "qt"), "weighted_containment": (L.MEASURE_QUERY_MASS, "totals", "q"),
    }

    def _measure(self, measure: str, qnorm, tnorm):
        """-> (L.Measure, the arrays it points into): the norms given, or those the formula of the same name would take"""
        if measure not in self._MEASURES:
            raise ValueError("measure: one of " + ", ".join(self._MEASURES))
        kind, norms, sides = self._MEASURES[measure]
        if measure == "jaccard" and self.has_totals():
            sides = ""  # shared / total: no norms
        if measure == "weighted_containment" and qnorm is None:
            if self._plain_targets is None:
                raise ValueError("weighted_containment is defined on the hits of Index.search_counted")
            if not self._plain_targets:
                raise ValueError("weighted_containment is defined against an index without counts (Sets.index): dot against a counted index is a product")
        q = t = None
        if "q" in sides:
            q = qnorm if qnorm is not None else self.query_sizes if norms == "sizes" else self._norm_arrays(measure)[0 if norms == "sumsq" else 2]
        if "t" in sides:
            t = tnorm if tnorm is not None else self.target_sizes if norms == "sizes" else self._norm_arrays(measure)[1 if norms == "sumsq" else 3]
        q = None if q is None else np.ascontiguousarray(q, np.uint64)
        t = None if t is None else np.ascontiguousarray(t, np.uint64)
        keep = [x if x is None or x.size else np.zeros(1, np.uint64) for x in (q, t)]  # (an empty array still has an address)
        m = L.Measure(kind, 0, None if q is None else keep[0].ctypes.data, 0 if q is None else q.size, None if t is None else keep[1].ctypes.data,
                      0 if t is None else t.size)
        return m, keep

    @staticmethod
    def _at_least(at_least):
        """-> (num, den) u64: an int, a fractions.Fraction, a (num, den) pair, or a float taken exactly"""
        if isinstance(at_least, tuple):
            num, den = int(at_least[0]), int(at_least[1])
        elif isinstance(at_least, fractions.Fraction):
            num, den = at_least.numerator, at_least.denominator
        elif isinstance(at_least, (int, np.integer)):
            num, den = int(at_least), 1
        else:
            x = float(at_least)
            if x != x or x in (float("inf"), float("-inf")):
                raise ValueError("at_least: not a finite number")
            num, den = x.as_integer_ratio()
        if den < 0:
            num, den = -num, -den
        if den == 0:
            raise ValueError("at_least: denominator 0")
        if num < 0:
            num, den = 0, 1  # (no measure is negative)
        if num >= 1 << 64 or den >= 1 << 64:
            raise ValueError("at_least: numerator or denominator beyond 64 bits; give a fractions.Fraction with smaller parts")
        return num, den

    def _selected(self, h, reuse: Optional["Hits"]) -> "Hits":
        """the Hits around a selection of self: the sizes, and the norms -- the snapshot if one was taken, else the way to take it"""
        res = reuse if reuse is not None else Hits(self.eng)
        carry = (self._norms, self._operands, self._gens, self._norm_source, self._plain_targets, self._flip)
        res._bind(h, self.query_sizes, self.target_sizes)
        res._norms, res._operands, res._gens, res._norm_source, res._plain_targets, res._flip = carry
        return res

    # -- hits by target (bsk_hits_transpose, bsk_hits_tally)
    def _n_targets(self, n_targets) -> int:
        return len(self.target_sizes) if n_targets is None else int(n_targets)

    def transpose(self, n_targets: Optional[int] = None, reuse: Optional["Hits"] = None) -> "Hits":
        """The hits by target (bsk_hits_transpose) -> Hits of n_targets rows (default: len(target_sizes)): row t lists the queries that hit
        t, ascending, every payload with its hit.  The result is bound with the sizes swapped, and so are the norms of the weighted
        side: jaccard(), containment(), cosine(), weighted_jaccard(), bray_curtis() and filter / top_by with their default norms read
        it as the hits of the targets against the queries.  weighted_containment(), which is one-sided, raises on it.  reuse: any Hits
        of this engine, but not self."""
        nt = self._n_targets(n_targets)
        h = _take_over(self.eng, reuse, lambda out: self.eng.lib.bsk_hits_transpose(self.eng.ctx, self.h, nt, out))
        res = reuse if reuse is not None else Hits(self.eng)
        norms, operands, gens, source = self._norms, self._operands, self._gens, self._norm_source
        plain, flip = self._plain_targets, self._flip
        rows = np.zeros(nt, np.uint64)  # (targets beyond the sizes known here are rows of size 0: nobody hit them)
        known = np.asarray(self.target_sizes, np.uint64)[:nt]
        rows[:len(known)] = known
        res._bind(h, rows, self.query_sizes)
        swap = lambda n: (n[1], n[0], n[3], n[2])  # noqa: E731
        if norms is not None:
            res._norms = swap(norms)
        else:
            res._norm_source = lambda: swap(Hits._resolve_norms(operands, gens, source, "a formula of transposed hits"))
        res._plain_targets, res._flip = (flip[0], None) if flip is not None else (None, (plain,))
        return res

    def tally(self, n_targets: Optional[int] = None, into: Optional["Tally"] = None, add: bool = False) -> "Tally":
        """The per-target table of the hits (bsk_hits_tally) -> Tally: .rows[t] the hits that name t, .unique[t] those that are the only
        hit of their row, .shared[t] the sum of their shared.  n_targets: default len(target_sizes).  into: the Tally of an earlier
        call on this engine, overwritten -- or, with add=True, added to (a table of the same n_targets; its info() adds up too)."""
        nt = self._n_targets(n_targets)
        h = _take_over(self.eng, into, lambda out: self.eng.lib.bsk_hits_tally(self.eng.ctx, self.h, nt, L.TALLY_ADD if add else 0, out))
        res = into if into is not None else Tally(self.eng)
        res._bind(h)
        return res

    def filter(self, measure: str, at_least, *, qnorm=None, tnorm=None, reuse: Optional["Hits"] = None) -> "Hits":
        """The hits whose measure is at least `at_least`, rows in their order, every payload kept (bsk_hits_filter) -> Hits.
        measure: "shared", "members", "dot", "min_sum", "query_cov", "target_cov", "jaccard", "cosine", "weighted_jaccard",
        "bray_curtis_similarity" (1 - bray_curtis()) or "weighted_containment".  at_least: an int, a fractions.Fraction, a (num, den)
        pair or a float, which is taken exactly (float.as_integer_ratio); the comparison is in integers, no rounding.  The norms are
        those the formula of the same name takes -- the sizes, or the operands' sumsq() / totals() under the rule of cosine() --
        unless qnorm / tnorm give them (u64 per query / per target).  The result keeps the norms: its formulas work without the
        operands.  reuse: any Hits of this engine, but not self."""
        m, keep = self._measure(measure, qnorm, tnorm)
        num, den = self._at_least(at_least)
        fp = L.FilterParams(num, den)
        h = _take_over(self.eng, reuse, lambda out: self.eng.lib.bsk_hits_filter(self.eng.ctx, self.h, C.byref(m), C.byref(fp), out))
        del keep
        return self._selected(h, reuse)

    def top_by(self, n: int, measure: str, *, qnorm=None, tnorm=None, reuse: Optional["Hits"] = None) -> "Hits":
        """Every query's min(n, hits) hits of largest measure, best first, ties by ascending target, every payload kept
        (bsk_hits_top_by) -> Hits.  measure and norms as in filter(); with "shared" the hits are those of top(n), which drops the
        payloads.  reuse: any Hits of this engine, but not self."""
        m, keep = self._measure(measure, qnorm, tnorm)
        h = _take_over(self.eng, reuse, lambda out: self.eng.lib.bsk_hits_top_by(self.eng.ctx, self.h, C.byref(m), n, out))
        del keep
        return self._selected(h, reuse)

    def has_members(self) -> bool:
        """whether the last entry that wrote these hits kept members (bsk_hits_members_device gives an array): fold() does"""
        if not self.h:
            return self._members is not None
        pm = C.c_void_p()
        self.eng._chk(self.eng.lib.bsk_hits_members_device(self.h, C.byref(pm)))
        return bool(pm.value)

    def fetch_members(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """bsk_hits_fetch_members -> members[] of the hits of the range; hits without members raise"""
        inf = self.info()
        if count is None:
            count = inf["n_queries"] - first
        mm = np.zeros(max(inf["n_hits"], 1), np.uint32)
        offs = np.zeros(count + 1, np.uint64)
        self.eng._chk(self.eng.lib.bsk_hits_fetch(self.eng.ctx, self.h, first, count, offs.ctypes.data, None, None, 0))
        self.eng._chk(self.eng.lib.bsk_hits_fetch_members(self.eng.ctx, self.h, first, count, mm.ctypes.data, mm.size))
        return mm[:int(offs[-1])]

    @property
    def members(self) -> Optional[np.ndarray]:
        """per hit of folded hits how many targets of its group the row hit; None for hits without members (anything but fold())"""
        self._cache()
        return self._members

    def cluster(self, method="components", score=None, reuse: Optional["Clusters"] = None) -> "Clusters":
        """The hits read as an undirected graph over their queries, clustered on the device (bsk_hits_cluster) -> Clusters.
        method "components": the connected components, each represented by its member of best rank; "greedy": by ascending rank a
        node joins the best representative it neighbours, or becomes one (cd-hit, galah).  score: n u64, higher is better, ties to
        the smaller index; None: index order.  reuse: the Clusters of an earlier call on this engine, whose device arrays are kept."""
        m = {"components": L.CLUSTER_COMPONENTS, "greedy": L.CLUSTER_GREEDY}.get(method, method)
        if not isinstance(m, int):
            raise ValueError("cluster: method is 'components' or 'greedy'")
        cp = L.ClusterParams(m, 0)
        sp = None
        if score is not None:
            score = np.ascontiguousarray(score, np.uint64)
            if score.ndim != 1 or len(score) != self.info()["n_queries"]:
                raise ValueError("cluster: score must hold one u64 per query")
            sp = score.ctypes.data if len(score) else None
        h = _take_over(self.eng, reuse, lambda out: self.eng.lib.bsk_hits_cluster(self.eng.ctx, self.h, C.byref(cp), sp, out))
        res = reuse if reuse is not None else Clusters(self.eng)
        res._bind(h)
        return res

    def device(self):
        """bsk_hits_device -> (offsets_ptr, target_ptr, shared_ptr)"""
        po, pt, ps = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.eng._chk(self.eng.lib.bsk_hits_device(self.h, C.byref(po), C.byref(pt), C.byref(ps)))
        return po.value, pt.value, ps.value

    def fetch(self, first: int = 0, count: Optional[int] = None):
        """bsk_hits_fetch -> (offsets[count+1] rebased, target[], shared[])"""
        inf = self.info()
        if count is None:
            count = inf["n_queries"] - first
        offs = np.zeros(count + 1, np.uint64)
        self.eng._chk(self.eng.lib.bsk_hits_fetch(self.eng.ctx, self.h, first, count, offs.ctypes.data, None, None, 0))
        n = int(offs[-1])
        tgt = np.zeros(max(n, 1), np.uint32)
        sh = np.zeros(max(n, 1), np.uint32)
        self.eng._chk(self.eng.lib.bsk_hits_fetch(self.eng.ctx, self.h, first, count, offs.ctypes.data, tgt.ctypes.data, sh.ctypes.data, tgt.size))
        return offs, tgt[:n], sh[:n]

    def has_totals(self) -> bool:
        """whether the last entry that wrote these hits kept totals (bsk_hits_totals_device gives an array): Sets.neighbors does"""
        if not self.h:
            return self._totals is not None
        pt = C.c_void_p()
        self.eng._chk(self.eng.lib.bsk_hits_totals_device(self.h, C.byref(pt)))
        return bool(pt.value)

    def fetch_totals(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """bsk_hits_fetch_totals -> total[] of the hits of the range; hits without totals raise"""
        inf = self.info()
        if count is None:
            count = inf["n_queries"] - first
        tt = np.zeros(max(inf["n_hits"], 1), np.uint32)
        offs = np.zeros(count + 1, np.uint64)
        self.eng._chk(self.eng.lib.bsk_hits_fetch(self.eng.ctx, self.h, first, count, offs.ctypes.data, None, None, 0))
        self.eng._chk(self.eng.lib.bsk_hits_fetch_totals(self.eng.ctx, self.h, first, count, tt.ctypes.data, tt.size))
        return tt[:int(offs[-1])]

    def has_weights(self) -> bool:
        """whether the last entry that wrote these hits kept dot and min_sum (bsk_hits_weights_device gives arrays): Sets.neighbors_counted does"""
        if not self.h:
            return self._weights is not None
        pd, pm = C.c_void_p(), C.c_void_p()
        self.eng._chk(self.eng.lib.bsk_hits_weights_device(self.h, C.byref(pd), C.byref(pm)))
        return bool(pd.value) and bool(pm.value)

    def fetch_weights(self, first: int = 0, count: Optional[int] = None):
        """bsk_hits_fetch_weights -> (dot[], min_sum[]) u64 of the hits of the range; hits without weights raise"""
        inf = self.info()
        if count is None:
            count = inf["n_queries"] - first
        dt, ms = np.zeros(max(inf["n_hits"], 1), np.uint64), np.zeros(max(inf["n_hits"], 1), np.uint64)
        offs = np.zeros(count + 1, np.uint64)
        self.eng._chk(self.eng.lib.bsk_hits_fetch(self.eng.ctx, self.h, first, count, offs.ctypes.data, None, None, 0))
        self.eng._chk(self.eng.lib.bsk_hits_fetch_weights(self.eng.ctx, self.h, first, count, dt.ctypes.data, ms.ctypes.data, dt.size))
        return dt[:int(offs[-1])], ms[:int(offs[-1])]

    def _cache(self):
        if self._host is None:
            self._host = self.fetch()
            self._totals = self.fetch_totals() if self.has_totals() else None
            self._weights = self.fetch_weights() if self.has_weights() else None
            self._members = self.fetch_members() if self.has_members() else None
        return self._host

    @property
    def offsets(self) -> np.ndarray:
        return self._cache()[0]

    @property
    def target(self) -> np.ndarray:
        return self._cache()[1]

    @property
    def shared(self) -> np.ndarray:
        return self._cache()[2]

    @property
    def total(self) -> Optional[np.ndarray]:
        """per hit the values walked (min(limit, |a | b|)); None for hits without totals (a search, top())"""
        self._cache()
        return self._totals

    @property
    def dot(self) -> Optional[np.ndarray]:
        """per hit the sum of the products of the two counts over the walked values both sets hold (u64, saturating); None for hits
        without weights (anything but Sets.neighbors_counted)"""
        self._cache()
        return None if self._weights is None else self._weights[0]

    @property
    def min_sum(self) -> Optional[np.ndarray]:
        """per hit the sum of the minima of the two counts (u64, exact); None for hits without weights"""
        self._cache()
        return None if self._weights is None else self._weights[1]

    def query(self) -> np.ndarray:
        """the query index of every hit"""
        return np.repeat(np.arange(len(self.offsets) - 1, dtype=np.uint64), np.diff(self.offsets).astype(np.int64))

    def containment(self) -> np.ndarray:
        """shared / |q| per hit"""
        q = self.query_sizes[self.query().astype(np.int64)].astype(np.float64)
        return self.shared.astype(np.float64) / q

    def jaccard(self) -> np.ndarray:
        """per hit shared / total where the hits carry totals (Sets.neighbors: the Mash estimator under a limit), else
        shared / (|q| + |t| - shared)"""
        s = self.shared.astype(np.float64)
        if self.total is not None:
            return s / self.total.astype(np.float64)  # (a listed pair shares a value: its total is not 0)
        q = self.query_sizes[self.query().astype(np.int64)].astype(np.float64)
        t = self.target_sizes[self.target.astype(np.int64)].astype(np.float64)
        return s / (q + t - s)

    def mash_distance(self, k: int) -> np.ndarray:
        """per hit, with j its Jaccard: 1.0 where j is 0, elsewhere max(0, -ln(2j / (1 + j)) / k) -- Compare.mash_distance's formula"""
        j = self.jaccard()
        d = np.ones_like(j)
        nz = j > 0
        d[nz] = np.maximum(0.0, -np.log(2.0 * j[nz] / (1.0 + j[nz])) / k)
        return d


    # -- the weighted side (bsk_sets_neighbors_counted): Compare's formulas, per hit
    def _norm_arrays(self, what: str):
        """(sumsq_a, sumsq_b, totals_a, totals_b) of the operands as the call that made the hits saw them: kept once fetched, fetched
        only while the operands are unwritten"""
        if self._norms is None:
            self._norms = Hits._resolve_norms(self._operands, self._gens, self._norm_source, what)
        return self._norms

    @staticmethod
    def _resolve_norms(operands, gens, source, what: str):
        """the norms from what a Hits knows of its operands (transpose() hands these on without the Hits itself)"""
        if gens is not None:
            _same_sets(*gens, what)
        if source is not None:
            return source()
        if operands is None:
            raise ValueError(what + ": these hits know no operands to take norms from; pass qnorm= and tnorm=")
        a, b, limit = operands
        if limit != 0:
            raise ValueError(what + " is defined on whole sets: neighbors_counted with limit=0")
        qa, ta = a.sumsq(), a.totals()
        qb, tb = (qa, ta) if b is a else (b.sumsq(), b.totals())
        return (qa, qb, ta, tb)

    def _whole(self, what: str):
        """(dot, min_sum, sumsq_a, sumsq_b, totals_a, totals_b) per hit of weighted hits over whole sets: the norms of the two operands
        gathered by query() and target"""
        self._cache()
        if self._weights is None:
            raise ValueError("hits without weights: use Sets.neighbors_counted or Index.search_counted")
        qa, qb, ta, tb = self._norm_arrays(what)
        i, j = self.query().astype(np.int64), self.target.astype(np.int64)
        return self._weights[0], self._weights[1], qa[i], qb[j], ta[i], tb[j]

    def cosine(self) -> np.ndarray:
        """per hit dot / (sqrt(sumsq_a[i]) * sqrt(sumsq_b[j])) as float64: 0.0 where a norm is 0, NaN where dot or either norm is saturated"""
        dt, _, qa, qb, _, _ = self._whole("cosine")
        top = int(np.iinfo(np.uint64).max)
        den = np.sqrt(qa.astype(np.float64)) * np.sqrt(qb.astype(np.float64))
        cos = np.divide(dt.astype(np.float64), den, out=np.zeros(dt.shape, np.float64), where=den != 0)
        cos[(dt == top) | (qa == top) | (qb == top)] = np.nan
        return cos

    def angular_similarity(self) -> np.ndarray:
        """per hit 1 - 2 acos(min(cosine, 1)) / pi: what sourmash compare reports for signatures with abundance"""
        return 1.0 - 2.0 * np.arccos(np.minimum(self.cosine(), 1.0)) / np.pi

    def weighted_jaccard(self) -> np.ndarray:
        """per hit min_sum / (totals_a[i] + totals_b[j] - min_sum) -- the sum of minima over the sum of maxima -- 0.0 where that is 0"""
        _, ms, _, _, ta, tb = self._whole("weighted_jaccard")
        m = ms.astype(np.float64)
        den = ta.astype(np.float64) + tb.astype(np.float64) - m
        return np.divide(m, den, out=np.zeros_like(m), where=den != 0)

    def bray_curtis(self) -> np.ndarray:
        """per hit 1 - 2 min_sum / (totals_a[i] + totals_b[j]) (the dissimilarity), 0.0 where the denominator is 0"""
        _, ms, _, _, ta, tb = self._whole("bray_curtis")
        m = ms.astype(np.float64)
        den = ta.astype(np.float64) + tb.astype(np.float64)
        out, nz = np.zeros_like(m), den != 0
        out[nz] = 1.0 - 2.0 * m[nz] / den[nz]
        return out

    def weighted_containment(self) -> np.ndarray:
        """per hit dot / totals_q[i]: the share of the query's mass -- the sum of its counts -- that lies on values the target holds
        (sourmash's abundance-weighted containment).  Defined for Index.search_counted against an index WITHOUT counts, where dot is
        the sum of the query's counts over the shared values; any other hits raise.  NaN where dot is saturated."""
        if self._flip is not None:
            raise ValueError("weighted_containment is one-sided (the share of the QUERY's mass): not defined on transposed hits; ask the hits before transpose()")
        if self._plain_targets is None:
            raise ValueError("weighted_containment is defined on the hits of Index.search_counted")
        if not self._plain_targets:
            raise ValueError("weighted_containment is defined against an index without counts (Sets.index): dot against a counted index is a product")
        dt, _, _, _, ta, _ = self._whole("weighted_containment")
        out = np.divide(dt.astype(np.float64), ta.astype(np.float64), out=np.zeros(dt.shape, np.float64), where=ta != 0)
        out[dt == int(np.iinfo(np.uint64).max)] = np.nan
        return out


class Tally(_Owner):
    """The per-target table of hits (bsk_tally): rows[n_targets], unique[n_targets], shared[n_targets], u64 each; fetched on first use."""

    _release = "bsk_tally_release"

    def __init__(self, eng: "Engine"):
        self.eng, self.h = eng, None
        self._host = None

    def _bind(self, h):
        self.h, self._host = h, None

    def info(self):
        v = [C.c_uint64() for _ in range(4)]
        self.eng._chk(self.eng.lib.bsk_tally_info(self.h, *[C.byref(x) for x in v]))
        return dict(n_targets=v[0].value, queries=v[1].value, hits=v[2].value, calls=v[3].value)

    def plan(self) -> str:
        """What the last call ran (bsk_tally_plan): the path -- counters in LDS or adds to the table -- with targets= and hits=."""
        p = C.c_char_p()
        self.eng._chk(self.eng.lib.bsk_tally_plan(self.h, C.byref(p)))
        return (p.value or b"").decode()

    def fetch(self, first: int = 0, count: Optional[int] = None):
        """bsk_tally_fetch -> (rows[count], unique[count], shared[count]) of targets first .. first + count - 1"""
        if count is None:
            count = self.info()["n_targets"] - first
        out = [np.zeros(max(count, 1), np.uint64) for _ in range(3)]
        self.eng._chk(self.eng.lib.bsk_tally_fetch(self.eng.ctx, self.h, first, count, *[x.ctypes.data for x in out]))
        return tuple(x[:count] for x in out)

    def device(self):
        """bsk_tally_device -> (rows_ptr, unique_ptr, shared_ptr)"""
        p = [C.c_void_p() for _ in range(3)]
        self.eng._chk(self.eng.lib.bsk_tally_device(self.h, *[C.byref(x) for x in p]))
        return tuple(x.value for x in p)

    def _cache(self):
        if self._host is None:
            self._host = self.fetch()
        return self._host

    @property
    def rows(self) -> np.ndarray:
        """per target the hits that name it"""
        return self._cache()[0]

    @property
    def unique(self) -> np.ndarray:
        """per target the hits that name it and are the only hit of their row"""
        return self._cache()[1]

    @property
    def shared(self) -> np.ndarray:
        """per target the sum of shared over the hits that name it"""
        return self._cache()[2]


class Clusters(_Owner):
    """Clusters of a hits graph (bsk_clusters): label[n], rep[n_clusters] ascending, offsets[n_clusters+1] and members[n]
    ascending inside a cluster; fetched on first use."""

    _release = "bsk_clusters_release"

    def __init__(self, eng: "Engine"):
        self.eng, self.h = eng, None
        self._host = None

    def _bind(self, h):
        self.h, self._host = h, None

    def info(self):
        n, nc, lg = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.eng._chk(self.eng.lib.bsk_clusters_info(self.h, C.byref(n), C.byref(nc), C.byref(lg)))
        return dict(n_items=n.value, n_clusters=nc.value, largest=lg.value)

    def plan(self):
        """What ran (bsk_clusters_plan): the kernels' names with n=, edges= and rounds=, and the two figures."""
        p, f = C.c_char_p(), (C.c_uint64 * 2)()
        self.eng._chk(self.eng.lib.bsk_clusters_plan(self.h, C.byref(p), f))
        return dict(plan=(p.value or b"").decode(), rounds=int(f[0]), edges=int(f[1]))

    def device(self):
        """bsk_clusters_device -> (label_ptr, rep_ptr, offsets_ptr, members_ptr)"""
        pl, pr, po, pm = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.eng._chk(self.eng.lib.bsk_clusters_device(self.h, C.byref(pl), C.byref(pr), C.byref(po), C.byref(pm)))
        return pl.value, pr.value, po.value, pm.value

    def fetch(self):
        """bsk_clusters_fetch -> (label[n], rep[n_clusters], offsets[n_clusters+1], members[n])"""
        inf = self.info()
        n, nc = inf["n_items"], inf["n_clusters"]
        label, rep = np.zeros(max(n, 1), np.uint32), np.zeros(max(nc, 1), np.uint32)
        offsets, members = np.zeros(nc + 1, np.uint64), np.zeros(max(n, 1), np.uint32)
        self.eng._chk(self.eng.lib.bsk_clusters_fetch(self.eng.ctx, self.h, label.ctypes.data, rep.ctypes.data, offsets.ctypes.data, members.ctypes.data))
        return label[:n], rep[:nc], offsets, members[:n]

    def _cache(self):
        if self._host is None:
            self._host = self.fetch()
        return self._host

    @property
    def label(self) -> np.ndarray:
        return self._cache()[0]

    @property
    def rep(self) -> np.ndarray:
        return self._cache()[1]

    @property
    def offsets(self) -> np.ndarray:
        return self._cache()[2]

    @property
    def members(self) -> np.ndarray:
        return self._cache()[3]

    @property
    def sizes(self) -> np.ndarray:
        """the number of members of every cluster"""
        return np.diff(self.offsets)


class Engine(_Owner):
    """One GPU context (bsk_ctx)."""

    _release, _slot = "bsk_ctx_destroy", "ctx"  # (no .h: a constructor that failed leaves no ctx either, which close() allows for)

    def __init__(self, device: int = 0):
        self.lib = L.load()
        h = C.c_void_p()
        rc = self.lib.bsk_ctx_create(device, C.byref(h))
        if rc != L.OK:
            raise DeviceError(f"bsk_ctx_create({device}) failed: {self.lib.bsk_err_name(rc).decode()}")
        self.ctx = h
        self._opts_seen = self._opts_env()

    @staticmethod
    def _opts_env():
        return tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("BSK_")))

    def _opts(self):
        """The library reads its developer switches (BSK_*) once per context; the test suite flips them inside one process, so this
        mirror reloads them (bsk_ctx_reload_options) when the environment changed since the last call.  Only when BSK_PY_WATCH_ENV
        is set (tests/conftest.py sets it): a production caller pays no scan of its environment per call and uses reload_options()."""
        if not (Engine._watch_env or os.environ.get("BSK_PY_WATCH_ENV")):  # (one dict lookup: set at any time, not only before import)
            return
        now = self._opts_env()
        if now != self._opts_seen:
            self._opts_seen = now
            self.lib.bsk_ctx_reload_options(self.ctx)

    _watch_env = bool(os.environ.get("BSK_PY_WATCH_ENV"))

    def reload_options(self):
        """Re-read the BSK_* developer switches from the environment now (bsk_ctx_reload_options)."""
        self._opts_seen = self._opts_env()
        self.lib.bsk_ctx_reload_options(self.ctx)

    def _chk(self, rc: int):
        if rc == L.OK:
            return
        if rc in _SENTINELS:
            raise _SENTINELS[rc]
        raise DeviceError(f"{self.lib.bsk_err_name(rc).decode()}: {self.lib.bsk_last_error(self.ctx).decode()}")

    # -- multi-GPU: the one collective of the path (bsk_comm_* / bsk_gather_counts: RCCL behind the C ABI)
    def comm_unique_id(self) -> bytes:
        buf = (C.c_uint8 * 128)()
        self._chk(self.lib.bsk_comm_unique_id(buf))
        return bytes(buf)

    def comm_init_rank(self, uid: bytes, rank: int, world: int) -> None:
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._chk(self.lib.bsk_comm_init_rank(self.ctx, buf, rank, world))
        self._world = world

    def gather_counts(self, mine: Sequence[int]) -> List[List[int]]:
        """all_gather of this rank's u64 counters; one list per rank, in rank order."""
        world = getattr(self, "_world", 0)
        a = np.asarray(list(mine), np.uint64)
        out = np.zeros(max(world, 1) * len(a), np.uint64)
        self._chk(self.lib.bsk_gather_counts(self.ctx, a.ctypes.data, len(a), out.ctypes.data))
        return [[int(v) for v in row] for row in out.reshape(world, len(a))]

    # -- end to end: file / host memory -> tuples on the host, stages overlapped over n_streams contexts (bsk_pipeline_*)
    @staticmethod
    def pipeline_fastx(path: str, params, n_streams: int = 2, chunk_records: int = 1 << 18, fetch: bool = True, alphabet: int = -1, device: int = 0):
        lib = L.load()
        st = L.PipelineStats()
        rc = lib.bsk_pipeline_fastx(device, path.encode(), alphabet, C.byref(params), n_streams, chunk_records, 1 if fetch else 0, C.byref(st))
        _chk_pipeline(lib, "bsk_pipeline_fastx", rc)
        return st.asdict()

    @staticmethod
    def pipeline_memory_multi(devices, data: np.ndarray, offsets: np.ndarray, params, n_streams: int = 2, chunk_records: int = 1 << 18,
                              repeat: int = 1, fetch: bool = True, alphabet: int = L.ALPHA_DNA):
        """bsk_pipeline_memory over several GPUs of the node (a device may be named more than once): one chunk queue, n_streams workers per device."""
        lib = L.load()
        data = np.ascontiguousarray(data, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        dev = (C.c_int * len(devices))(*devices)
        st = L.PipelineStats()
        rc = lib.bsk_pipeline_memory_multi(dev, len(devices), data.ctypes.data, offsets.ctypes.data, len(offsets) - 1, alphabet, C.byref(params),
                                           n_streams, chunk_records, repeat, 1 if fetch else 0, C.byref(st))
        _chk_pipeline(lib, "bsk_pipeline_memory_multi", rc)
        return st.asdict()

    @staticmethod
    def pipeline_fastx_multi(devices, path: str, params, n_streams: int = 2, chunk_records: int = 1 << 18, fetch: bool = True, alphabet: int = -1):
        lib = L.load()
        dev = (C.c_int * len(devices))(*devices)
        st = L.PipelineStats()
        rc = lib.bsk_pipeline_fastx_multi(dev, len(devices), path.encode(), alphabet, C.byref(params), n_streams, chunk_records, 1 if fetch else 0, C.byref(st))
        _chk_pipeline(lib, "bsk_pipeline_fastx_multi", rc)
        return st.asdict()

    @staticmethod
    def pipeline_open(params, *, paths=None, data: np.ndarray = None, offsets: np.ndarray = None, devices=(0,), n_streams: int = 2,
                      chunk_records: int = 1 << 18, sink: int = L.SINK_TUPLES, sets_scale: int = 1, alphabet: int = -1, repeat: int = 1,
                      host_checksum: bool = False, n_readers: int = 0, search: Optional["Index"] = None, top_n: int = 0, min_shared: int = 1,
                      min_query_cov: float = 0.0, min_target_cov: float = 0.0) -> "Pipeline":
        """bsk_pipeline_open_fastx / _memory: the pipeline with a consumer (the role of fastx's ChunkChan, seqio/fastx/reader.go:562-608).
        search=index (with sink=SINK_HITS): bsk_pipeline_open_*_search -- every chunk's per-record sets (sets_scale) are searched against
        the index on the device and the chunks carry hits (ChunkView.target / .shared), every read's top_n best when top_n != 0.  The
        index must have been built from sets of the same params and scale, and stay open until the pipeline is closed."""
        sp = None
        if search is not None:
            sp = L.PipelineSearch(search.h.value if isinstance(search.h, C.c_void_p) else search.h, L.SearchParams(min_shared, 0, min_query_cov, min_target_cov),
                                  top_n, 0)
        return Pipeline(params, paths, data, offsets, devices, n_streams, chunk_records, sink, sets_scale, alphabet, repeat, host_checksum, n_readers, sp, search)

    @staticmethod
    def pipeline_trim() -> None:
        """Return the pinned host buffers the pipelines pool between calls (bsk_pipeline_trim)."""
        L.load().bsk_pipeline_trim()

    @staticmethod
    def pipeline_fastx_files(paths, params, n_streams: int = 3, n_readers: int = 0, chunk_records: int = 1 << 18, fetch: bool = True,
                             alphabet: int = -1, device: int = 0):
        """Several FASTA/FASTQ files (plain or gzip) through one pipeline, n_readers of them read at once."""
        lib = L.load()
        st = L.PipelineStats()
        arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
        rc = lib.bsk_pipeline_fastx_files(device, arr, len(paths), alphabet, C.byref(params), n_streams, n_readers, chunk_records, 1 if fetch else 0,
                                          C.byref(st))
        _chk_pipeline(lib, "bsk_pipeline_fastx_files", rc)
        return st.asdict()

    @staticmethod
    def pipeline_memory(data: np.ndarray, offsets: np.ndarray, params, n_streams: int = 2, chunk_records: int = 1 << 20, repeat: int = 1,
                        fetch: bool = True, alphabet: int = L.ALPHA_DNA, device: int = 0):
        lib = L.load()
        data = np.ascontiguousarray(data, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        st = L.PipelineStats()
        rc = lib.bsk_pipeline_memory(device, data.ctypes.data, offsets.ctypes.data, len(offsets) - 1, alphabet, C.byref(params), n_streams,
                                     chunk_records, repeat, 1 if fetch else 0, C.byref(st))
        _chk_pipeline(lib, "bsk_pipeline_memory", rc)
        return st.asdict()

    # -- batches
    def batch(self, seqs: Sequence, alphabet: int = L.ALPHA_DNA) -> Batch:
        bs = [s.Seq if isinstance(s, Seq) else (s.encode() if isinstance(s, str) else bytes(s)) for s in seqs]
        offs = np.zeros(len(bs) + 1, np.uint64)
        if bs:
            offs[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
        data = np.frombuffer(b"".join(bs), np.uint8) if offs[-1] else np.zeros(1, np.uint8)
        return self.batch_from_arrays(data, offs, alphabet)

    def batch_from_arrays(self, data: np.ndarray, offsets: np.ndarray, alphabet: int = L.ALPHA_DNA) -> Batch:
        data = np.ascontiguousarray(data, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        h = C.c_void_p()
        self._opts()
        self._chk(self.lib.bsk_batch_from_ascii(self.ctx, data.ctypes.data, offsets.ctypes.data, len(offsets) - 1,
                                                alphabet, C.byref(h)))
        return Batch(self, h)

    def sets_from_arrays(self, offsets: np.ndarray, values: np.ndarray) -> Sets:
        """Sets from the host (bsk_sets_from_host): offsets[n_sets+1] (offsets[0] = 0, offsets[-1] = len(values)), values strictly
        ascending inside every set -- e.g. a reference collection loaded from disk."""
        offsets = np.ascontiguousarray(offsets, np.uint64)
        values = np.ascontiguousarray(values, np.uint64)
        if offsets.ndim != 1 or len(offsets) < 1 or int(offsets[-1]) != len(values):
            raise ValueError("sets_from_arrays: offsets must have n_sets + 1 entries and end at len(values)")
        h = C.c_void_p()
        self._chk(self.lib.bsk_sets_from_host(self.ctx, offsets.ctypes.data, len(offsets) - 1, values.ctypes.data if len(values) else None,
                                              C.byref(h)))
        return Sets(self, h)

    def hits_from_arrays(self, offsets: np.ndarray, target: np.ndarray, shared: np.ndarray, total: Optional[np.ndarray] = None,
                         reuse: Optional["Hits"] = None) -> "Hits":
        """Hits from the host (bsk_hits_from_host): CSR offsets[n_queries+1] (offsets[0] = 0, offsets[-1] = len(target)), targets
        strictly ascending inside a row, shared[] and, optionally, total[] -- edges computed elsewhere, ready for Hits.cluster.  The
        Hits know no set sizes: containment() and the size-based jaccard() are not defined for them."""
        offsets = np.ascontiguousarray(offsets, np.uint64)
        target = np.ascontiguousarray(target, np.uint32)
        shared = np.ascontiguousarray(shared, np.uint32)
        if offsets.ndim != 1 or len(offsets) < 1 or int(offsets[-1]) != len(target) or len(shared) != len(target):
            raise ValueError("hits_from_arrays: offsets must have n_queries + 1 entries and end at len(target) == len(shared)")
        if total is not None:
            total = np.ascontiguousarray(total, np.uint32)
            if len(total) != len(target):
                raise ValueError("hits_from_arrays: total must be as long as target")
            if not len(total):
                total = np.zeros(1, np.uint32)  # (no hits, but hits WITH totals)
        nh = len(target)
        h = _take_over(self, reuse, lambda out: self.lib.bsk_hits_from_host(self.ctx, offsets.ctypes.data, len(offsets) - 1, target.ctypes.data if nh else None,
                                                                           shared.ctypes.data if nh else None, None if total is None else total.ctypes.data, out))
        res = reuse if reuse is not None else Hits(self)
        res._bind(h, np.zeros(len(offsets) - 1, np.uint64), np.zeros(0, np.uint64))
        return res

    def merge_hits(self, parts: Sequence["Hits"], target_base=None, add: bool = False, reuse: Optional["Hits"] = None) -> "Hits":
        """One Hits out of the hits of several searches of the same queries (bsk_hits_merge): a database split over many indexes.
        Row q holds every hit of row q of every part with target_base[p] added to its target, strictly ascending, with every payload
        all parts carry.  target_base: default the running sum of len(part.target_sizes) -- shards by target, shard p holds the
        targets behind those of the shards before it.  Shards by value (every shard holds all targets and part of the hash space):
        target_base=[0] * len(parts) and add=True, which sums the fields of a pair that several parts report, saturating; without
        add such a pair is an error.  Search the value shards with min_shared=1 and filter("shared", m) the merged hits: the
        threshold is on the sum.  The parts may belong to other engines, on this device or another; at most 64 parts.
        The result's query_sizes are those of parts[0] (unequal ones raise ValueError); target_sizes[base_p + i] +=
        part_p.target_sizes[i].  The weighted side is a snapshot taken now: with weights on every part, every part's norms are
        resolved (a part that cannot raises the ValueError of its own formulas), the query norms are those of parts[0] and the target
        norms are added at base_p like the sizes, saturating.  reuse: any Hits of this engine that is not among the parts."""
        parts = list(parts)
        P = len(parts)
        if target_base is None:
            base = np.zeros(P, np.uint64)
            base[1:] = np.cumsum([len(p.target_sizes) for p in parts[:-1]], dtype=np.uint64)
        else:
            base = np.array([int(b) for b in target_base], np.uint64)  # (a negative or a 65-bit base raises here)
            if base.shape != (P,):
                raise ValueError("merge_hits: target_base needs one entry per part")
        snap = None
        if P:
            if any(not np.array_equal(p.query_sizes, parts[0].query_sizes) for p in parts[1:]):
                raise ValueError("merge_hits: the parts differ in their query_sizes: they are not hits of the same queries")
            for what in ("_plain_targets", "_flip"):
                if any(getattr(p, what) != getattr(parts[0], what) for p in parts[1:]):
                    raise ValueError("merge_hits: the parts differ in " + what.strip("_") + " (hits against counted and plain indexes, or transposed and not)")
            n = max(int(b) + len(p.target_sizes) for b, p in zip(base, parts))
            top = np.uint64(np.iinfo(np.uint64).max)

            def spread(arrays):  # arrays[p] added at base[p], saturating
                out = np.zeros(n, np.uint64)
                for b, a in zip(base, arrays):
                    a = np.asarray(a, np.uint64)
                    s = out[int(b):int(b) + len(a)]
                    t = s + a
                    t[t < a] = top
                    s[:] = t
                return out

            sizes = spread([p.target_sizes for p in parts])
            norms = None
            if all(p.has_weights() for p in parts):
                each = [p._norm_arrays("merge_hits") for p in parts]
                norms = (each[0][0], spread([x[1] for x in each]), each[0][2], spread([x[3] for x in each]))
            snap = (parts[0].query_sizes, sizes, norms, parts[0]._plain_targets, parts[0]._flip)
        hs = (C.c_void_p * max(P, 1))(*[p.h for p in parts])
        h = _take_over(self, reuse, lambda out: self.lib.bsk_hits_merge(self.ctx, hs, base.ctypes.data if P else None, P, L.MERGE_ADD if add else 0, out))
        res = reuse if reuse is not None else Hits(self)
        res._bind(h, snap[0], snap[1])
        res._norms, res._plain_targets, res._flip = snap[2:]
        return res

    def sets_from_arrays_counted(self, offsets: np.ndarray, values: np.ndarray, counts: np.ndarray) -> Sets:
        """sets_from_arrays with counts[len(values)] (u32, none of them 0): bsk_sets_from_host_counted"""
        offsets = np.ascontiguousarray(offsets, np.uint64)
        values = np.ascontiguousarray(values, np.uint64)
        counts = np.ascontiguousarray(counts, np.uint32)
        if offsets.ndim != 1 or len(offsets) < 1 or int(offsets[-1]) != len(values) or len(counts) != len(values):
            raise ValueError("sets_from_arrays_counted: offsets must have n_sets + 1 entries and end at len(values) == len(counts)")
        h = C.c_void_p()
        self._chk(self.lib.bsk_sets_from_host_counted(self.ctx, offsets.ctypes.data, len(offsets) - 1, values.ctypes.data if len(values) else None,
                                                      counts.ctypes.data if len(counts) else None, C.byref(h)))
        return Sets(self, h)

    def batch_from_packed(self, words: np.ndarray, desc: np.ndarray) -> Batch:
        words = np.ascontiguousarray(words, np.uint32)
        desc = np.ascontiguousarray(desc, np.uint64)
        h = C.c_void_p()
        self._opts()
        self._chk(self.lib.bsk_batch_from_packed(self.ctx, words.ctypes.data, len(words), desc.ctypes.data, len(desc),
                                                 C.byref(h)))
        return Batch(self, h)

    def batch_from_fastx(self, reader, max_records: int = 0, max_bytes: int = 0, alphabet: int = -1):
        """Next chunk of a bio_amd.fastx.Reader straight into a device batch (bsk_batch_from_fastx): (Batch or None, n_records).
        alphabet < 0: the reader's guess from its first record, as the reference does."""
        h = C.c_void_p()
        n = C.c_uint64()
        self._opts()
        self._chk(self.lib.bsk_batch_from_fastx(self.ctx, reader.h, max_records, max_bytes, alphabet, C.byref(h), C.byref(n)))
        return (Batch(self, h) if n.value else None), n.value

    def synth(self, alphabet: int, n: int, length: int, seed: int) -> Batch:
        h = C.c_void_p()
        self._opts()
        self._chk(self.lib.bsk_batch_synth(self.ctx, alphabet, n, length, seed, C.byref(h)))
        return Batch(self, h)

    # -- compute
    @staticmethod
    def params(kind, k, w=0, s=0, m=0, scale=0, canonical=True, circular=False, codon_table=1, frame=1) -> L.Params:
        return L.Params(kind, k, w, s, m, scale, int(bool(canonical)), int(bool(circular)), codon_table, frame)

    def run(self, batch: Batch, p: L.Params, reuse: Optional[BatchResult] = None) -> BatchResult:
        h = reuse.h if reuse is not None else C.c_void_p()
        self._opts()
        self._chk(self.lib.bsk_sketch(self.ctx, batch.h, C.byref(p), C.byref(h)))
        if reuse is not None:
            reuse.h, reuse.params, reuse._host = h, p, None
            return reuse
        return BatchResult(self, h, p)

    def run_timed(self, batch: Batch, p: L.Params, warmup: int, iters: int, reuse: Optional[BatchResult] = None):
        h = reuse.h if reuse is not None else C.c_void_p()
        ms = (C.c_float * max(iters, 1))()
        self._opts()
        self._chk(self.lib.bsk_sketch_timed(self.ctx, batch.h, C.byref(p), C.byref(h), warmup, iters, ms))
        res = reuse if reuse is not None else BatchResult(self, h, p)
        res.h, res.params, res._host = h, p, None
        return res, [ms[i] for i in range(iters)]

    def prepare(self, batch: Batch, p: L.Params) -> float:
        """Per-batch preparation a sketch with these parameters would do on its first call (length-binned units of a ragged batch),
        done now; returns the device milliseconds of the pass (0.0: the plan needs none).  bsk_batch_prepare."""
        ms = C.c_float(0.0)
        self._opts()
        self._chk(self.lib.bsk_batch_prepare(self.ctx, batch.h, C.byref(p), C.byref(ms)))
        return float(ms.value)

    def sync(self):
        self._chk(self.lib.bsk_ctx_sync(self.ctx))


_default_engine: Optional[Engine] = None


def default_engine() -> Engine:
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine(0)
    return _default_engine


# ---- cursors: the reference's iterator types over one read's slice of a BatchResult -----------------
class _Cursor:
    def __init__(self, status: int, codes: np.ndarray, pos: Optional[np.ndarray]):
        self._status, self._codes, self._pos = status, codes, pos
        self._i = 0
        self._idx = -1

    def _next(self):
        if self._i >= len(self._codes):
            return 0, False
        c = int(self._codes[self._i])
        self._idx = int(self._pos[self._i] & L.POS_MASK) if self._pos is not None else self._i
        self._strand = int(self._pos[self._i] >> 31) if self._pos is not None else 0
        self._i += 1
        return c, True

    def Index(self) -> int:
        return self._idx

    def flags(self) -> int:
        """engine extension: the read's BSK_ST_* status byte"""
        return self._status


class Iterator(_Cursor):
    """k-mer code / ntHash / SimHash iterator (iterator.go:60-106)."""

    def __init__(self, status, codes, kind, n_per_strand=None):
        super().__init__(status, codes, None)
        self._kind = kind
        self._nps = n_per_strand

    def NextHash(self):  # iterator.go:658
        return self._next()

    def NextSimHash(self):  # iterator.go:191
        return self._next()

    def NextKmer(self):  # iterator.go:708 -> (code, ok, err)
        c, ok = self._next()
        if not ok and (self._status & L.ST_CODE_MASK) == L.ST_ILLEGAL:
            return 0, False, ErrIllegalBase
        if ok and self._nps:  # non-canonical: Index() restarts at 0 on the reverse strand (iterator.go:720)
            self._idx = self._idx % self._nps
        return c, ok, None

    def Next(self):  # iterator.go:762
        if self._kind == L.KMER:
            return self.NextKmer()
        c, ok = self._next()
        return c, ok, None


class Sketch(_Cursor):
    """minimizer / syncmer sketch iterator (sketch.go:45-77)."""

    def NextMinimizer(self):  # sketch.go:205
        return self._next()

    def NextSyncmer(self):  # sketch.go:312
        return self._next()

    def Next(self):  # sketch.go:480
        return self._next()

    def Strand(self) -> int:
        """engine extension: 1 iff the reverse-strand hash was the canonical one for the last tuple"""
        return self._strand


class ProteinIterator(_Cursor):
    def Next(self):  # iterator-protein.go:76
        return self._next()


class ProteinMinimizerSketch(_Cursor):
    def Next(self):  # sketch-protein.go:106
        return self._next()


class ChunkView:
    """One chunk of a Pipeline: numpy VIEWS over the pipeline's pinned arrays (no copy is made on delivery), valid until the next chunk is
    taken -- copy what you keep.  offsets / status / hash are views; pos / strand are decoded from the narrow arrays on first use."""

    def __init__(self, c: L.Chunk):
        self.sequence, self.source_index, self.device = c.sequence, c.source_index, c.device
        self.first_record, self.n_records, self.n_bases, self.n_tuples, self.n_values = c.first_record, c.n_records, c.n_bases, c.n_tuples, c.n_values
        self.checksum, self.link_bytes, self.sink, self.has_pos = c.checksum, c.link_bytes, c.sink, bool(c.has_pos)
        n, nv = int(c.n_records), int(c.n_values)

        def view(ptr, count, dtype):
            if not ptr:
                return None
            if count == 0:
                return np.empty(0, dtype)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(count,))

        self.status = view(c.status, n, np.uint8)
        self.offsets = view(c.offsets32, n + 1, np.uint32) if c.offsets32 else view(c.offsets64, n + 1, np.uint64)
        self.hash = view(c.hash, nv, np.uint64)
        self.pos16 = view(c.pos16, nv, np.uint16) if nv else None   # BSK_POS16 encoding (bit 15 = strand), as delivered
        self.pos32 = view(c.pos32, nv, np.uint32) if nv else None   # BSK_POS encoding (bit 31 = strand): chunks with a read of 32 768 bases or more
        self._pos = self._strand = None
        self.target = self.shared = None  # SINK_HITS: record i owns target / shared[offsets[i] : offsets[i + 1]] (bsk_chunk_hits)
        if c.sink == L.SINK_HITS:
            pt, ps = C.c_void_p(), C.c_void_p()
            if L.load().bsk_chunk_hits(C.byref(c), C.byref(pt), C.byref(ps)) == L.OK:
                self.target, self.shared = view(pt.value, nv, np.uint32), view(ps.value, nv, np.uint32)

    @property
    def pos(self):
        """positions (u32, strand bit removed), decoded on first use; None for kinds with implicit positions / sets"""
        if self._pos is None:
            if self.pos16 is not None:
                self._pos = (self.pos16 & 0x7FFF).astype(np.uint32)
            elif self.pos32 is not None:
                self._pos = self.pos32 & L.POS_MASK
        return self._pos

    @property
    def strand(self):
        if self._strand is None:
            if self.pos16 is not None:
                self._strand = (self.pos16 >> 15).astype(np.uint8)
            elif self.pos32 is not None:
                self._strand = (self.pos32 >> 31).astype(np.uint8)
        return self._strand


class PipelineStopped(Exception):
    """bsk_pipeline_next after bsk_pipeline_cancel / an early close: the run was stopped, not failed."""


class Pipeline:
    """bsk_pipeline: sketches of every chunk of the input, delivered in input order (include/biosketch.h, "the pipeline with a consumer").

        with Engine.pipeline_open(params, paths=["reads.fq"], sink=L.SINK_SETS, sets_scale=100) as pl:
            for chunk in pl.chunks():
                ...chunk.offsets / chunk.hash / chunk.pos / chunk.status...
        pl.stats
    """

    def __init__(self, params, paths, data, offsets, devices, n_streams, chunk_records, sink, sets_scale, alphabet, repeat, host_checksum, n_readers,
                 search=None, index=None):
        self.lib = L.load()
        self._dev = (C.c_int * len(devices))(*devices)
        cfg = L.PipelineConfig(self._dev, len(devices), n_streams, chunk_records, sink, sets_scale, alphabet, 1 if host_checksum else 0, n_readers, 0)
        self.h = C.c_void_p()
        self._keep = (data, offsets, params)
        self._index = index  # (the searched index lives at least as long as the pipeline)
        if paths is not None:
            arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
            if search is not None:
                rc = self.lib.bsk_pipeline_open_fastx_search(C.byref(cfg), arr, len(paths), C.byref(params), C.byref(search), C.byref(self.h))
            else:
                rc = self.lib.bsk_pipeline_open_fastx(C.byref(cfg), arr, len(paths), C.byref(params), C.byref(self.h))
        else:
            data = np.ascontiguousarray(data, dtype=np.uint8)
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            self._keep = (data, offsets, params)
            if search is not None:
                rc = self.lib.bsk_pipeline_open_memory_search(C.byref(cfg), data.ctypes.data, offsets.ctypes.data, len(offsets) - 1, repeat, C.byref(params),
                                                              C.byref(search), C.byref(self.h))
            else:
                rc = self.lib.bsk_pipeline_open_memory(C.byref(cfg), data.ctypes.data, offsets.ctypes.data, len(offsets) - 1, repeat, C.byref(params),
                                                       C.byref(self.h))
        if rc != L.OK:
            self.h = C.c_void_p()
            raise _SENTINELS.get(rc) or DeviceError(f"bsk_pipeline_open: {self.lib.bsk_err_name(rc).decode()}")
        self.stats = None
        self._held = None

    def next(self) -> Optional[ChunkView]:
        """The next chunk in input order, None at the end.  Releases the chunk handed out before."""
        self._release()
        c = C.POINTER(L.Chunk)()
        rc = self.lib.bsk_pipeline_next(self.h, C.byref(c))
        if rc == -1:
            raise PipelineStopped("the pipeline was cancelled")
        if rc != L.OK:
            msg = self.lib.bsk_pipeline_error(self.h).decode()
            raise _SENTINELS.get(rc) or DeviceError(f"bsk_pipeline_next: {self.lib.bsk_err_name(rc).decode()}: {msg}")
        if not c:
            return None
        self._held = c
        return ChunkView(c.contents)

    def _release(self):
        if self._held is not None:
            self.lib.bsk_pipeline_release(self.h, self._held)
            self._held = None

    def chunks(self):
        while True:
            c = self.next()
            if c is None:
                return
            yield c

    def cancel(self) -> None:
        """Stops the run from any thread and frees nothing (bsk_pipeline_cancel): a consumer blocked in next() gets PipelineStopped."""
        if self.h:
            self.lib.bsk_pipeline_cancel(self.h)

    def close(self):
        if self.h:
            self._release()
            st = L.PipelineStats()
            rc = self.lib.bsk_pipeline_close(self.h, C.byref(st))
            self.h = C.c_void_p()
            self.stats = st.asdict()
            if rc not in (L.OK, -1):
                raise _SENTINELS.get(rc) or DeviceError(f"bsk_pipeline_close: {self.lib.bsk_err_name(rc).decode()}")
        return self.stats

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _single(seq: Seq, p: L.Params, alphabet: int, eng: Optional[Engine]):
    eng = eng or default_engine()
    b = eng.batch([seq], alphabet)
    try:
        res = eng.run(b, p)
    except SketchError as e:
        b.close()
        return None, None, e
    status, codes, pos = res.read(0)
    res.close()
    b.close()
    if (status & L.ST_CODE_MASK) == L.ST_SHORT:
        return None, None, ErrShortSeq
    return (status, codes, pos), None, None


def NewHashIterator(s: Seq, k: int, canonical: bool, circular: bool, engine: Optional[Engine] = None):
    got, _, err = _single(s, Engine.params(L.NTHASH, k, canonical=canonical, circular=circular), L.ALPHA_DNA, engine)
    if err is not None:
        return None, err
    return Iterator(got[0], got[1], L.NTHASH), None


def NewKmerIterator(s: Seq, k: int, canonical: bool, circular: bool, engine: Optional[Engine] = None):
    alpha = _alpha_code(s.Alphabet)
    got, _, err = _single(s, Engine.params(L.KMER, k, canonical=canonical, circular=circular), L.ALPHA_DNA if alpha == L.ALPHA_PROTEIN else alpha, engine)
    if err is not None:
        return None, err
    nps = None if canonical else (len(s.Seq) + (k - 1 if circular else 0) - k + 1)
    return Iterator(got[0], got[1], L.KMER, nps), None


def NewSimHashIterator(s: Seq, k: int, m: int, scale: int, canonical: bool, circular: bool,
                       engine: Optional[Engine] = None):
    got, _, err = _single(s, Engine.params(L.SIMHASH, k, m=m, scale=scale, canonical=canonical, circular=circular),
                          L.ALPHA_DNA, engine)
    if err is not None:
        return None, err
    return Iterator(got[0], got[1], L.SIMHASH), None


def NewMinimizerSketch(S: Seq, k: int, w: int, circular: bool, engine: Optional[Engine] = None):
    got, _, err = _single(S, Engine.params(L.MINIMIZER, k, w=w, circular=circular), L.ALPHA_DNA, engine)
    if err is not None:
        return None, err
    return Sketch(*got), None


def NewSyncmerSketch(S: Seq, k: int, s: int, circular: bool, engine: Optional[Engine] = None):
    got, _, err = _single(S, Engine.params(L.SYNCMER, k, s=s, circular=circular), L.ALPHA_DNA, engine)
    if err is not None:
        return None, err
    return Sketch(*got), None


def NewProteinIterator(s: Seq, k: int, codonTable: int, frame: int, engine: Optional[Engine] = None):
    alpha = L.ALPHA_PROTEIN if s.Alphabet is Protein else L.ALPHA_DNA
    got, _, err = _single(s, Engine.params(L.PROT_HASH, k, codon_table=codonTable, frame=frame), alpha, engine)
    if err is not None:
        return None, err
    return ProteinIterator(got[0], got[1], None), None


def NewProteinMinimizerSketch(S: Seq, k: int, codonTable: int, frame: int, w: int, engine: Optional[Engine] = None):
    alpha = L.ALPHA_PROTEIN if S.Alphabet is Protein else L.ALPHA_DNA
    if k >= 1 and len(S.Seq) < k * 3:  # upstream's order: k, then this length check (sketch-protein.go:66), only then w (:69)
        return None, ErrShortSeq
    got, _, err = _single(S, Engine.params(L.PROT_MINIMIZER, k, w=w, codon_table=codonTable, frame=frame), alpha, engine)
    if err is not None:
        return None, err
    return ProteinMinimizerSketch(*got), None
