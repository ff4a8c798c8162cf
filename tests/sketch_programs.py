"""Seeded programs over the sketch-side entries (batches, bsk_sketch, the result objects and their fetches) and their model.

program(seed) is a list of steps, fully determined by the seed: a program owns a few batch slots and a few result slots on one
context and runs 12 to 20 steps over them -- batches made (ASCII or packed, sometimes two back to back), re-filled through both
entries in turn, translated and destroyed; bsk_sketch into a fresh result or into one that any other batch, kind or layout made;
bsk_sketch_timed and bsk_batch_prepare inside their contracts; every read entry of a result (info, fetch, fetch_narrow, fetch_status,
digest, sets, counted sets, compact with its arrays read back later, the raw device arrays decoded on the host); releases; and
switches of the BSK_* options that move these small batches across plan boundaries.  The oracle does not depend on the plan, so no
switch changes what is expected.

run(program, backend) drives a back-end step by step and returns one record per step and a last one for everything alive at the end.
Model(oracle) is the back-end that answers from the oracle; tests/test_gpu_sketch_programs.py holds the device's back-end;
same(want, got) is the one comparison.  SABOTAGES are models with one piece of state left stale, named after the host mistake they
stand for: tests/test_sketch_programs.py shows that `same` catches each of them in every block, and what the campaign reaches.
Every step that leaves another result alive carries `recheck`, one of them (drawn), which is fetched again after the step and
must be what it was.

The first ten programs of a block follow the nine THEMES (the reserve's twice), one per state the sketch side keeps between calls (the reserve of released arrays, a
result re-used across kinds, sizes and layouts, the pool slots the fetches share, the class lists, the codon table, a re-filled
batch, the pinned staging); the other six draw their steps at random.  Nothing here imports the engine.

    python -m tests.sketch_programs SEED      prints the program of that seed, call by call"""
import sys
import zlib

import numpy as np

from tests import counts_cases as CN
from tests.algebra_programs import same  # noqa: F401  (the one comparison, shared with the sets-side campaign)

U64, U32, U16, U8 = np.uint64, np.uint32, np.uint16, np.uint8
BASE, BLOCKS, PER_BLOCK = 0x5CE7C000, 6, 16
ST_OK, ST_SHORT, ST_ILLEGAL = 0, 1, 2
TIE, NON_ACGT = 0x10, 0x20
REF_ROWS = 1 << 63
AA = "ACDEFGHIKLMNPQRSTVWY"
FRAMES = (1, 2, 3, -1, -2, -3)
POSITIONAL = ("minimizer", "syncmer", "prot_minimizer")
# the flag bits of an accepted read that are compared, per kind, as tests/test_gpu_plan_atlas.py and test_gpu_parity_kinds.py compare
# them: both flags for minimizers and syncmers, the first-window tie for protein minimizers, the non-ACGT flag for ntHash and SimHash
# (k-mer codes map IUPAC letters to a base: no flag there)
FLAG_MASK = dict(minimizer=TIE | NON_ACGT, syncmer=TIE | NON_ACGT, prot_minimizer=TIE, nthash=NON_ACGT, simhash=NON_ACGT, kmer=0, prot_hash=0)
# one row per kernel family the planner can choose at these lengths (tests/test_gpu_state_machine.py: CASES; tests/plan_atlas.py)
PARAMS = (
    ("minimizer", dict(k=21, w=11)), ("minimizer", dict(k=21, w=5)), ("minimizer", dict(k=31, w=15)), ("minimizer", dict(k=15, w=7)),
    ("minimizer", dict(k=64, w=20)), ("minimizer", dict(k=21, w=1)), ("minimizer", dict(k=21, w=11, circular=True)),
    ("syncmer", dict(k=31, s=11)), ("syncmer", dict(k=31, s=7)), ("syncmer", dict(k=33, s=8)), ("syncmer", dict(k=31, s=31)),
    ("nthash", dict(k=21, canonical=True)), ("nthash", dict(k=21, canonical=False)),
    ("kmer", dict(k=21, canonical=True)), ("kmer", dict(k=21, canonical=False)), ("kmer", dict(k=32, canonical=True)), ("kmer", dict(k=32, canonical=False)),
    ("simhash", dict(k=21, m=5, scale=5)), ("simhash", dict(k=70, m=6, scale=3)),
    ("prot_hash", dict(k=9)), ("prot_hash", dict(k=17)),
    ("prot_minimizer", dict(k=9, w=5)), ("prot_minimizer", dict(k=3, w=1)),
)
KINDS = tuple(dict.fromkeys(k for k, _ in PARAMS))
SWITCHES = ("BSK_TILE_MIN", "BSK_TILE_POS", "BSK_BIN_MIN", "BSK_CLASS_FORCE", "BSK_CLASS_MIN", "BSK_CLASS_VIEW", "BSK_NO_MIXED", "BSK_FORCE_GENERIC",
            "BSK_NO_TILES", "BSK_NO_TILE_DEFER", "BSK_NO_SPARE", "BSK_NO_SYN_PF")
TILED_40 = {"BSK_TILE_MIN": "40", "BSK_TILE_POS": "32"}
TILED_64 = {"BSK_TILE_MIN": "64", "BSK_TILE_POS": "48"}
CLASSED = {"BSK_CLASS_FORCE": "1", "BSK_CLASS_MIN": "64"}  # (16 384 reads by default: these batches hold a few hundred)
ENVS = (TILED_40, TILED_64, {"BSK_TILE_MIN": "40", "BSK_TILE_POS": "16", "BSK_NO_TILE_DEFER": "1"}, {"BSK_BIN_MIN": "1"}, CLASSED,
        dict(CLASSED, BSK_CLASS_VIEW="1"), {"BSK_NO_MIXED": "1"}, {"BSK_FORCE_GENERIC": "1"}, {"BSK_NO_TILES": "1"}, {"BSK_NO_SPARE": "1"}, {"BSK_NO_SYN_PF": "1"}, {}, {})
# The reserve (biosketch.hip: spare_give / spare_take) keeps a released array of 1 MiB or more -- 2^20 / 8 = 131 072 tuples of the u64 hash
# array, which holds at least the result's tuples -- and hands it to a request of b bytes when b <= its bytes <= 2 b + 64 MiB.  A pair
# counts when both results hold that many tuples and the second holds no more than the first.
RESERVE_TUPLES = (1 << 20) // 8
RESERVE_SLACK_TUPLES = (64 << 20) // 8
NARROW_LIMIT = 32768        # bsk_result_fetch_narrow refuses a position of 15 bits or more
BASES_BUDGET = 400_000      # the bases of a program's batches, about
ORACLE_BUDGET = 1_300_000   # the bases its sketch steps hand to the oracle, about
UNIT_EDGES = (1, 63, 64, 65, 511, 512, 513)
READS = ("info", "fetch", "narrow", "status", "digest", "sets", "counted", "compact", "device")
THEMES = ("reserve", "reserve", "kinds", "sizes", "tiles", "fetches", "classes", "translate", "refill", "pairs") + ("random",) * 6


def seeds(block):
    return [BASE + PER_BLOCK * block + i for i in range(PER_BLOCK)]


def theme_of(seed):
    return THEMES[(seed - BASE) % PER_BLOCK]


def genetic_codes(oracle):
    """every id oracle.genetic_code accepts"""
    out = []
    for t in range(0, 64):
        try:
            oracle.genetic_code(t)
            out.append(t)
        except ValueError:
            pass
    return out


def flagged(q):
    """whether a DNA read holds a byte outside ACGTacgt"""
    return bool(q.translate(None, b"ACGTacgt"))


def pkey(p):
    return tuple(sorted(p.items()))


# ---- one read through the oracle -> (status code, flag bits, hashes, positions with the strand in bit 31 or None) ----
_cache = {}


def clear_cache():
    _cache.clear()


def oracle_read(O, kind, p, protein, q):
    key = (kind, pkey(p), protein, q)
    hit = _cache.get(key)
    if hit is not None:
        return hit
    k, circ = p["k"], bool(p.get("circular"))
    pos = np.zeros(0, U32) if kind in POSITIONAL else None
    try:
        fl = 0
        if kind in ("minimizer", "syncmer"):
            fn = O.minimizer if kind == "minimizer" else O.syncmer
            h, ps, strand, ofl = fn(q, k, p["w"] if kind == "minimizer" else p["s"], circ, closed=True)
            pos = ps.astype(U32) | (strand.astype(U32) << U32(31))
            fl = (ofl & TIE) | (NON_ACGT if flagged(q) else 0)
        elif kind == "nthash":
            h = O.nthash(q, k, p["canonical"], circ)[0]
            fl = NON_ACGT if flagged(q) else 0
        elif kind == "kmer":
            h = O.kmer_codes(q, k, p["canonical"], circ, 0)
        elif kind == "simhash":
            h = O.simhash(q, k, p["m"], p["scale"], True)
            fl = NON_ACGT if flagged(q) else 0
        elif kind == "prot_hash":
            h = O.protein_hashes(q, k) if protein else O.protein_hashes_nt(q, k, p["codon_table"], p["frame"])
        else:
            h, ps, ofl = O.protein_minimizer(q, k, p["w"], closed=True) if protein else O.protein_minimizer_nt(q, k, p["w"], p["codon_table"], p["frame"])
            pos, fl = ps.astype(U32), ofl & TIE
        out = (ST_OK, fl & FLAG_MASK[kind], h.astype(U64), pos)
    except O.OracleError as e:
        if e.name not in ("ErrShortSeq", "ErrIllegalBase"):
            raise
        out = (ST_SHORT if e.name == "ErrShortSeq" else ST_ILLEGAL, 0, np.zeros(0, U64), pos)
    _cache[key] = out
    return out


def translation(O, q, table, frame):
    return O.translate(q, table, frame).encode("latin-1") if len(q) >= 3 else b""


# ---- results as the model and the records hold them ----
def result_of(kind, p, per_read):
    """per_read: (code, flags, hash, pos) of every read -> the result's state"""
    n = len(per_read)
    counts = np.array([len(r[2]) for r in per_read], np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(U64)
    has_pos = kind in POSITIONAL
    return dict(kind=kind, p=p, n=n, has_pos=has_pos, offsets=offsets, code=np.array([r[0] for r in per_read], U8), flags=np.array([r[1] for r in per_read], U8),
                hash=np.concatenate([r[2] for r in per_read] + [np.zeros(0, U64)]).astype(U64),
                pos=np.concatenate([r[3] for r in per_read] + [np.zeros(0, U32)]).astype(U32) if has_pos else None)


def status_parts(kind, status):
    """a result's status bytes -> (codes, the compared flag bits of the accepted reads)"""
    status = np.asarray(status, U8)
    code = status & U8(0x0F)
    return code, np.where(code == ST_OK, status & U8(FLAG_MASK[kind]), 0).astype(U8)


def fetch_record(r, first=0, count=None):
    count = r["n"] - first if count is None else count
    a, b = int(r["offsets"][first]), int(r["offsets"][first + count])
    return dict(offsets=(r["offsets"][first:first + count + 1] - r["offsets"][first]).astype(U64), code=r["code"][first:first + count], flags=r["flags"][first:first + count],
                hash=r["hash"][a:b], pos=None if r["pos"] is None else r["pos"][a:b])


def narrow_record(r, first, count, keep_strand=True):
    f = fetch_record(r, first, count)
    if f["pos"] is not None and len(f["pos"]) and int((f["pos"] & U32(0x7FFFFFFF)).max()) >= NARROW_LIMIT:
        return dict(refused="BSK_ERR_UNSUPPORTED")
    if f["pos"] is not None:
        f["pos"] = ((f["pos"] & U32(0x7FFF)) | ((f["pos"] >> U32(16)) & U32(0x8000 if keep_strand else 0))).astype(U16)
    f["offsets"] = f["offsets"].astype(U32)
    return f


def digest_record(r):
    T = len(r["hash"])
    if r["pos"] is not None:
        weight = U64(2) * (r["pos"] & U32(0x7FFFFFFF)).astype(U64) + U64(1)
    else:
        weight = U64(2) * (np.arange(T, dtype=U64) - np.repeat(r["offsets"][:-1], np.diff(r["offsets"]).astype(np.int64))) + U64(1)
    return dict(checksum=int((r["hash"] * weight).sum(dtype=U64)) if T else 0, n_tuples=T, short=int((r["code"] == ST_SHORT).sum()), illegal=int((r["code"] == ST_ILLEGAL).sum()))


def sets_record(r, whole, scale, counted, extra=None):
    per = [r["hash"][int(a):int(b)] for a, b in zip(r["offsets"][:-1], r["offsets"][1:])]
    if extra is not None and whole:
        per = per + [extra]
    o, v, c = CN.ref_counted(per, scale, whole) if per else (np.zeros(2 if whole else 1, U64), np.zeros(0, U64), np.zeros(0, U32))
    return dict(offsets=o.astype(U64), values=v.astype(U64), counts=c.astype(U32) if counted else None)


def compact_record(r):
    return dict(n_tuples=len(r["hash"]), offsets=r["offsets"].copy(), hash=r["hash"].copy(), pos=None if r["pos"] is None else r["pos"].copy())


def raw_layout(r):
    """A device layout of a result as include/biosketch.h describes it, for the decoder below: results with positions write units of 64
    reads as rows (tuple j of the unit's read l at base + l + 64 j, BSK_REF_ROWS set), the others lie dense with gaps between the reads"""
    n, counts = r["n"], np.diff(r["offsets"]).astype(np.int64)
    first, stride = np.zeros(n, np.int64), np.ones(n, np.int64)
    at = 0
    if r["has_pos"]:
        for u in range(0, n, 64):
            c = counts[u:u + 64]
            first[u:u + 64], stride[u:u + 64] = at + np.arange(len(c)), 64
            at += 64 * int(c.max(initial=0)) + 64
    else:
        for i in range(n):
            first[i] = at
            at += int(counts[i]) + 3
    size = at + 64
    hash_, pos = np.full(size, 0xDEADBEEFDEADBEEF, U64), (np.full(size, 0xFFFFFFFF, U32) if r["has_pos"] else None)
    idx = np.repeat(first, counts) + (np.arange(len(r["hash"])) - np.repeat(r["offsets"][:-1].astype(np.int64), counts)) * np.repeat(stride, counts)
    hash_[idx] = r["hash"]
    if pos is not None:
        pos[idx] = r["pos"]
    refs = (first.astype(U64) << U64(24)) | counts.astype(U64) | np.where(stride == 64, U64(REF_ROWS), U64(0))
    return refs, hash_, pos


def decode_refs(refs, ignore_stride=False):
    """reference words -> (first, count, stride) of every read (BSK_REF_FIRST / _COUNT / _STRIDE)"""
    refs = np.asarray(refs, U64)
    first = ((refs & U64(REF_ROWS - 1)) >> U64(24)).astype(np.int64)
    count = (refs & U64(0xFFFFFF)).astype(np.int64)
    stride = np.where((refs & U64(REF_ROWS)) != 0, 1 if ignore_stride else 64, 1).astype(np.int64)
    return first, count, stride


def tuple_index(first, count, stride):
    """the index of every tuple in the raw arrays, read by read: first + j * stride"""
    j = np.arange(int(count.sum()), dtype=np.int64) - np.repeat(np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64), count)
    return np.repeat(first, count) + j * np.repeat(stride, count)


def device_record(kind, first, count, stride, status, read_hash, read_pos, layout_ok=True):
    """what the raw arrays of a result decode to; read_hash(idx) / read_pos(idx) gather from the raw arrays (read_pos None: implicit)"""
    idx = tuple_index(first, count, stride)
    code, flags = status_parts(kind, status)
    return dict(offsets=np.concatenate([[0], np.cumsum(count)]).astype(U64), code=code, flags=flags, hash=read_hash(idx).astype(U64),
                pos=None if read_pos is None else read_pos(idx).astype(U32), layout_ok=layout_ok)


# ---- the model: the back-end that answers from the oracle ----
class Model:
    name = "the oracle"

    def __init__(self, O):
        self.O = O
        self.batches, self.results, self.env = {}, {}, {}
        self.cls_owner = None  # the result whose class plan the context's pooled lists describe (bsk_ctx::cls_owner)
        self.compact_arrays = None

    # -- hooks the sabotages override
    def content(self, slot, seqs, protein, refilled):
        """what a batch object holds after it was made or re-filled with seqs"""
        return list(seqs)

    def table_for(self, table):
        return table

    def stale_flags(self, batch):
        return None

    def adopt(self, slot, new, old):
        """the state of result `slot` after a sketch made `new` (old: what the object held, None for a fresh one)"""
        return new

    def narrow_keeps_strand(self):
        return True

    def ignore_stride(self):
        return False

    def after_fetch(self, rec):
        pass

    def after_timed(self, slot):
        pass

    def timed_refuses(self):
        return True

    def sets_extra(self, slot):
        return None

    # -- batches
    def batch_record(self, slot):
        b = self.batches[slot]
        offs = np.concatenate([[0], np.cumsum([len(q) for q in b["seqs"]])]).astype(U64)
        return dict(n_reads=len(b["seqs"]), n_bases=int(offs[-1]), n_non_acgt=None if b["protein"] else sum(flagged(q) for q in b["seqs"]),
                    offsets=offs, bytes=np.frombuffer(b"".join(b["seqs"]), U8).copy())

    def _set_batch(self, slot, seqs, protein, refilled):
        old = self.batches.get(slot)
        self.batches[slot] = dict(seqs=self.content(slot, seqs, protein, refilled), protein=protein, version=(old["version"] + 1 if old else 0),
                                  before=old["seqs"] if old else None)

    def make(self, s):
        self._set_batch(s["slot"], s["seqs"], s["protein"], False)
        return self.batch_record(s["slot"])

    def make2(self, s):
        for x in (s["a"], s["b"]):
            self._set_batch(x["slot"], x["seqs"], x["protein"], False)
        self.second_of_a_pair(s["a"]["slot"], s["b"]["slot"])
        return dict(a=self.batch_record(s["a"]["slot"]), b=self.batch_record(s["b"]["slot"]))

    def second_of_a_pair(self, a, b):
        pass

    def refill(self, s):
        self._set_batch(s["slot"], s["seqs"], s["protein"], True)
        return self.batch_record(s["slot"])

    def translate(self, s):
        src = self.batches[s["src"]]
        t = self.table_for(s["table"])
        self.batches[s["slot"]] = dict(seqs=[translation(self.O, q, t, s["frame"]) for q in src["seqs"]], protein=True, version=0, before=None)
        return self.batch_record(s["slot"])

    def destroy(self, s):
        del self.batches[s["slot"]]
        return dict(done=True)

    def switch(self, s):
        self.env = dict(s["env"])
        return dict(done=True)

    def prepare(self, s):
        return dict(done=True)

    # -- sketches
    def sketch(self, s):
        b = self.batches[s["batch"]]
        stale = self.stale_flags(b)
        per = []
        for i, q in enumerate(b["seqs"]):
            code, fl, h, pos = oracle_read(self.O, s["sketch"], s["p"], b["protein"], q)
            if stale is not None and code == ST_OK and i < len(stale) and stale[i]:
                fl |= NON_ACGT & FLAG_MASK[s["sketch"]]
            per.append((code, fl, h, pos))
        new = result_of(s["sketch"], s["p"], per)
        new["made"] = dict(batch=s["batch"], tiled=s.get("tiled", False), classed=s.get("classed", False), lens=[len(q) for q in b["seqs"]])
        self.results[s["res"]] = r = self.adopt(s["res"], new, self.results.get(s["res"]))
        if s.get("classed"):
            self.cls_owner = s["res"]
        self.after_sketch(s["res"])
        return self.info_record(r)

    def after_sketch(self, slot):
        pass

    def timed(self, s):
        r = self.results[s["res"]]
        if r["made"]["classed"] and self.cls_owner != s["res"] and self.timed_refuses():  # a younger class plan took the pooled lists: BSK_ERR_ARG, the result as it was
            return dict(refused="BSK_ERR_ARG", all=fetch_record(r))
        self.after_timed(s["res"])
        return dict(info=self.info_record(self.results[s["res"]]), all=fetch_record(self.results[s["res"]]))

    @staticmethod
    def info_record(r):
        return dict(n_reads=r["n"], n_tuples=len(r["hash"]), has_pos=r["has_pos"])

    def read(self, s):
        r, how = self.results[s["res"]], s["how"]
        if "first" in s and s["first"] + s["count"] > r["n"]:  # (only a sabotaged model gets here)
            return dict(refused="BSK_ERR_ARG")
        if how == "info":
            return self.info_record(r)
        if how == "fetch":
            rec = fetch_record(r, s["first"], s["count"])
            self.after_fetch(rec)
            return rec
        if how == "narrow":
            return narrow_record(r, s["first"], s["count"], self.narrow_keeps_strand())
        if how == "status":
            f = fetch_record(r, s["first"], s["count"])
            return dict(code=f["code"], flags=f["flags"])
        if how == "digest":
            return digest_record(r)
        if how in ("sets", "counted"):
            return sets_record(r, s["whole"], s["scale"], how == "counted", self.sets_extra(s["res"]))
        if how == "compact":
            self.compact_arrays = compact_record(r)
            return dict(n_tuples=len(r["hash"]), has_pos=r["pos"] is not None)
        assert how == "device", how
        refs, hash_, pos = raw_layout(r)
        first, count, stride = decode_refs(refs, self.ignore_stride())
        status = r["code"] | r["flags"]
        return device_record(r["kind"], first, count, stride, status, lambda i: hash_[i], None if pos is None else (lambda i: pos[i]))

    def compact_read(self, s):
        return self.compact_arrays

    def release(self, s):
        self.released(self.results.pop(s["res"]))
        if self.cls_owner == s["res"]:
            self.cls_owner = None
        return dict(done=True)

    def released(self, r):
        pass

    def recheck(self, slot):
        return fetch_record(self.results[slot])

    def end(self):
        return dict(results={i: fetch_record(r) for i, r in self.results.items()}, batches={i: self.batch_record(i) for i in self.batches})


def run(program, backend, upto=None):
    """every step on the back-end -> one record per step, then the record of everything alive at the end"""
    records = []
    for step in program[:upto]:
        rec = getattr(backend, step["kind"])(step)
        if step.get("recheck") is not None:
            rec = dict(step=rec, recheck=backend.recheck(step["recheck"]))
        records.append(rec)
    if upto is None:
        records.append(backend.end())
    return records


# ---- the sabotages: one piece of state left stale each ----
def _cut(data, lens):
    """data cut into reads of the given lengths, as far as it goes"""
    out, at = [], 0
    for n in lens:
        out.append(data[at:at + n])
        at += n
    return out


class StaleCodonTable(Model):
    name = "1 the codon table of the previous translation is used"
    last = None

    def table_for(self, table):
        t, self.last = (self.last if self.last is not None else table), table
        return t


class KeepsPreviousN(Model):
    name = "2 a re-used result keeps the previous n"

    def adopt(self, slot, new, old):
        if old is None or old["n"] == new["n"]:
            return new
        n = old["n"]
        per = [(int(new["code"][i]), int(new["flags"][i]), new["hash"][int(new["offsets"][i]):int(new["offsets"][i + 1])],
                None if new["pos"] is None else new["pos"][int(new["offsets"][i]):int(new["offsets"][i + 1])]) if i < new["n"] else
               (ST_SHORT, 0, np.zeros(0, U64), None if new["pos"] is None else np.zeros(0, U32)) for i in range(n)]
        out = result_of(new["kind"], new["p"], per)
        out["made"] = new["made"]
        return out


class KeepsPositions(Model):
    name = "3 a re-used result keeps its positions after a change to an every-position kind, and lacks them after the change back"

    def adopt(self, slot, new, old):
        if old is not None and old["has_pos"] != new["has_pos"]:
            new["has_pos"] = old["has_pos"]
            new["pos"] = np.zeros(len(new["hash"]), U32) if old["has_pos"] else None
        return new


class NarrowLosesStrand(Model):
    name = "4 the narrow fetch loses the strand bit"

    def narrow_keeps_strand(self):
        return False


class DecodeIgnoresStride(Model):
    name = "5 the reference-word decode ignores the row stride"

    def ignore_stride(self):
        return True


class CompactOverwritten(Model):
    name = "6 the compact arrays are overwritten by a later fetch"

    def after_fetch(self, rec):
        c = self.compact_arrays
        if c is not None and len(rec["hash"]):
            m = min(len(rec["hash"]), len(c["hash"]))
            c["hash"][:m] = rec["hash"][:m]


class RefillKeepsFlags(Model):
    name = "7 a re-filled batch keeps the previous chunk's non-ACGT flags"

    def stale_flags(self, batch):
        return None if batch["before"] is None or batch["protein"] else [flagged(q) for q in batch["before"]]


class RefillKeepsStride(Model):
    name = "8 a re-filled ragged batch keeps the previous fixed-length stride"

    def content(self, slot, seqs, protein, refilled):
        old = self.batches.get(slot)
        if refilled and old and seqs and len({len(q) for q in old["seqs"]}) == 1 and len({len(q) for q in seqs}) > 1:
            stride, data = len(old["seqs"][0]), b"".join(seqs)
            return [data[i * stride:i * stride + len(q)] for i, q in enumerate(seqs)]
        return list(seqs)


class SecondGetsFirstDescriptors(Model):
    name = "9 the second of two batches made back to back gets the first's descriptors"

    def second_of_a_pair(self, a, b):
        A, B = self.batches[a], self.batches[b]
        B["seqs"] = _cut(b"".join(B["seqs"]), [len(q) for q in A["seqs"]])


class StatusShowsThrough(Model):
    name = "10 a released result's status bytes show through in the next result's short reads"
    ghost = None

    def released(self, r):
        self.ghost = (r["code"], r["flags"])

    def adopt(self, slot, new, old):
        if old is None and self.ghost is not None:
            m = min(new["n"], len(self.ghost[0]))
            short = new["code"][:m] == ST_SHORT
            new["code"][:m][short] = self.ghost[0][:m][short]
        return new


class TimedUsesYoungerLists(Model):
    name = "11 a timed re-run of a class-plan result uses the lists of the younger one"

    def timed_refuses(self):
        return False

    def after_timed(self, slot):
        r = self.results[slot]
        younger = [x for i, x in self.results.items() if i != slot and x["made"]["classed"]]
        if not r["made"]["classed"] or not younger:
            return
        lens = younger[-1]["made"]["lens"]
        bulk = max(set(lens), key=lens.count)
        listed = [i for i, n in enumerate(lens) if n != bulk and i < r["n"]]
        per = [(int(r["code"][i]), int(r["flags"][i]), np.zeros(0, U64) if i in listed else r["hash"][int(r["offsets"][i]):int(r["offsets"][i + 1])],
                np.zeros(0, U32) if i in listed else r["pos"][int(r["offsets"][i]):int(r["offsets"][i + 1])]) for i in range(r["n"])]
        out = result_of(r["kind"], r["p"], per)
        out["made"] = r["made"]
        self.results[slot] = out


class SetsHoldTheTiledValues(Model):
    name = "12 the whole-batch sets of a result made after a tiled call contain the tiled call's values"
    tiled_values = None

    def after_sketch(self, slot):
        r = self.results[slot]
        r["ghost"] = None if r["made"]["tiled"] else self.tiled_values
        if r["made"]["tiled"]:
            self.tiled_values = r["hash"][:64].copy()

    def sets_extra(self, slot):
        return self.results[slot].get("ghost")


SABOTAGES = (StaleCodonTable, KeepsPreviousN, KeepsPositions, NarrowLosesStrand, DecodeIgnoresStride, CompactOverwritten, RefillKeepsFlags, RefillKeepsStride,
             SecondGetsFirstDescriptors, StatusShowsThrough, TimedUsesYoungerLists, SetsHoldTheTiledValues)


# ---- the generator ----
_ACGT = np.frombuffer(b"ACGT", U8)
_IUPAC = np.frombuffer(b"NRYKMSWBDHVnacgtU", U8)
_AA = np.frombuffer(AA.encode(), U8)


def _dna(rng, n):
    return _ACGT[rng.integers(0, 4, n)].tobytes()


def _flag(rng, q, style):
    """q with one to three letters outside ACGTacgt (junk: one that is no IUPAC letter either)"""
    if not q:
        return q
    a = bytearray(q)
    a[int(rng.integers(0, len(a)))] = ord("N") if style != "junk" else int(rng.choice(np.frombuffer(b"X-*.7", U8)))
    if style == "iupac":
        for _ in range(int(rng.integers(0, max(1, len(a) // 10) + 1))):
            a[int(rng.integers(0, len(a)))] = int(_IUPAC[rng.integers(0, len(_IUPAC))])
    return bytes(a)


def lengths(rng, shape):
    if shape == "fixed":
        n = int(rng.choice(UNIT_EDGES)) if rng.random() < 0.8 else int(rng.integers(1100, 2201))
        return [150] * n
    if shape == "ragged":
        return [int(x) for x in rng.integers(0, 401, int(rng.integers(20, 300)))]
    if shape == "classmix":
        lens = [150] * int(rng.integers(200, 500)) + [400] * int(rng.integers(3, 7)) + [3000] * int(rng.integers(1, 4))
        return [int(x) for x in rng.permutation(lens)]
    if shape == "long":
        return [int(x) for x in rng.integers(200, 3001, int(rng.integers(3, 30)))]
    if shape == "long5000":
        return [int(x) for x in rng.integers(200, 3001, int(rng.integers(3, 12)))] + [5000]
    if shape == "empty":
        return []
    if shape == "tooshort":
        return [int(x) for x in rng.integers(0, 9, int(rng.integers(1, 100)))]
    assert shape == "big", shape
    return [150] * int(rng.integers(2, 20)) + [33000]


def dna_reads(rng, shape, style):
    """style: acgt | fewN | manyN | allN | iupac | junk -- letters outside ACGT only in flagged reads, which hold one outside ACGTacgt"""
    share = dict(acgt=0.0, fewN=0.05, manyN=0.6, allN=1.0, iupac=0.4, junk=0.2)[style]
    return [_flag(rng, q, style) if share and rng.random() < share else q for q in (_dna(rng, n) for n in lengths(rng, shape))]


def protein_reads(rng):
    alpha = (_AA, _AA, np.frombuffer((AA + "X*").encode(), U8), np.frombuffer(b"AC", U8))[int(rng.integers(0, 4))]
    return [alpha[rng.integers(0, len(alpha), int(n))].tobytes() for n in rng.integers(0, 401, int(rng.integers(5, 200)))]


def packable(seqs):
    return len(seqs) > 0 and all(not q.translate(None, b"ACGT") for q in seqs)


def pack(seqs):
    """2-bit words and descriptors of bsk_batch_from_packed: 16 bases a word, A0 C1 G2 T3, every read on a word boundary"""
    words, desc, w = [], np.zeros(len(seqs), U64), 0
    for r, q in enumerate(seqs):
        s = np.frombuffer(q, U8)
        nw = (len(s) + 15) // 16
        pad = np.zeros(nw * 16, U64)
        pad[:len(s)] = ((s >> 1) ^ (s >> 2)) & 3
        words.append((pad.reshape(nw, 16) << (U64(2) * np.arange(16, dtype=U64))).sum(axis=1).astype(U32))
        desc[r] = (w << 24) | len(s)
        w += nw
    return np.concatenate(words + [np.zeros(1, U32)]), w, desc


def predicted_tiled(env, kind, p, seqs, protein):
    """whether the call is expected to run over tiles (a wide result): what the reach figures count, never what a record holds"""
    if protein or kind in ("prot_hash", "prot_minimizer") or "BSK_NO_TILES" in env or not seqs:
        return False
    longest = max(len(q) for q in seqs) + (p["k"] - 1 if p.get("circular") else 0)
    if "BSK_TILE_MIN" in env:
        return longest > int(env["BSK_TILE_MIN"]) + 64
    return longest > (4096 if kind in ("minimizer", "syncmer") else 512)


def predicted_classed(env, kind, p, seqs):
    return "BSK_CLASS_FORCE" in env and kind in ("minimizer", "syncmer") and not p.get("circular") and len(seqs) >= int(env.get("BSK_CLASS_MIN", 16384)) and \
        len({len(q) for q in seqs}) > 1 and "BSK_NO_TILES" not in env


class _Gen:
    def __init__(self, seed, O):
        self.seed, self.rng, self.O, self.model = seed, np.random.default_rng(seed), O, Model(O)
        self.steps, self.records = [], []
        self.bases = self.work = self.next_b = self.next_r = 0
        self.sized = {}          # result slot -> (batch slot, batch version, kind, pkey, env, prepares) of the sketch that sized it
        self.prepares = 0
        self.compact_at = None   # index of the step whose compact arrays are still the context's
        self.codes = genetic_codes(O)

    def block_tables(self):
        """the four genetic codes of this program's block"""
        at = 4 * ((self.seed - BASE) // PER_BLOCK)
        return [self.codes[(at + i) % len(self.codes)] for i in range(4)]

    # -- plumbing
    def emit(self, step):
        live = [i for i in self.model.results if i != step.get("res")]  # (the results alive after the step, but for its own)
        if live:
            step["recheck"] = live[int(self.rng.integers(0, len(live)))]
        rec = getattr(self.model, step["kind"])(step)
        if "recheck" in step:
            rec = dict(step=rec, recheck=self.model.recheck(step["recheck"]))
        self.steps.append(step)
        self.records.append(rec)
        return rec

    def new_batch(self):
        self.next_b += 1
        return "b%d" % (self.next_b - 1)

    def new_result(self):
        self.next_r += 1
        return "r%d" % (self.next_r - 1)

    def choice(self, xs):
        return xs[int(self.rng.integers(0, len(xs)))]

    # -- batch steps
    def how(self, seqs, protein, prefer=None):
        ok = not protein and packable(seqs)
        return "packed" if ok and (prefer == "packed" or (prefer is None and self.rng.random() < 0.4)) else "ascii"

    def make_step(self, seqs, protein=False, slot=None, note=""):
        self.bases += sum(len(q) for q in seqs)
        return dict(kind="make", slot=slot or self.new_batch(), how=self.how(seqs, protein), protein=protein, seqs=seqs, note=note)

    def make(self, seqs, protein=False, note=""):
        s = self.make_step(seqs, protein, note=note)
        self.emit(s)
        return s["slot"]

    def refill(self, slot, seqs, prefer=None, note=""):
        protein = self.model.batches[slot]["protein"]  # (the alphabet is fixed per object: a re-fill with another one is not drawn)
        self.bases += sum(len(q) for q in seqs)
        self.emit(dict(kind="refill", slot=slot, how=self.how(seqs, protein, prefer), protein=protein, seqs=seqs, note=note))

    def draw_dna(self, shapes=("fixed", "ragged", "ragged", "long", "tooshort"), styles=("acgt", "acgt", "fewN", "manyN", "allN", "iupac", "junk")):
        shape, style = self.choice(shapes), self.choice(styles)
        return dna_reads(self.rng, shape, style), "%s, %s" % (shape, style)

    # -- sketch steps
    def params(self, kind=None, protein=False, positional=None):
        rows = [(k, p) for k, p in PARAMS if (kind is None or k == kind) and (not protein or k.startswith("prot_")) and
                (positional is None or (k in POSITIONAL) == positional)]
        k, p = self.choice(rows)
        p = dict(p)
        if k.startswith("prot_") and not protein:
            p.update(codon_table=int(self.choice(self.codes)), frame=int(self.choice(FRAMES)))
        return k, p

    def sketch(self, batch, res=None, kind=None, p=None, positional=None, reads=True):
        b = self.model.batches[batch]
        longest = max((len(x) for x in b["seqs"]), default=0)
        if longest > 9000 and (kind is None and p is None):  # the longest reads: the kinds whose positions the narrow fetch can refuse, and ntHash
            kind = self.choice(("minimizer", "syncmer", "nthash"))
        if longest > 9000 and ({"BSK_NO_TILES", "BSK_FORCE_GENERIC"} & set(self.model.env) or (kind or "").startswith("prot_")):
            return None
        for _ in range(8):  # k-mer codes of a read with a letter that is no base stop at it (ErrIllegalBase): the oracle keeps no tuples then, so another kind is drawn
            k, q = (kind, p) if p is not None else self.params(kind, b["protein"], positional)
            if all(oracle_read(self.O, k, q, b["protein"], x)[0] != ST_ILLEGAL for x in b["seqs"]):
                break
            if p is not None or kind is not None:
                return None
        else:
            return None
        fresh = res is None or res not in self.model.results
        res = res or self.new_result()
        self.work += sum(len(x) for x in b["seqs"])
        env = self.model.env
        step = dict(kind="sketch", batch=batch, res=res, sketch=k, p=q, fresh=fresh, tiled=predicted_tiled(env, k, q, b["seqs"], b["protein"]),
                    classed=predicted_classed(env, k, q, b["seqs"]), before=None if fresh else self.model.info_record(self.model.results[res]) | dict(
                        kind=self.model.results[res]["kind"], tiled=self.model.results[res]["made"]["tiled"]))
        self.emit(step)
        self.sized[res] = (batch, b["version"], k, pkey(q), dict(env), self.prepares)
        if reads:
            self.read(res)
        return res

    def timed_ok(self, res, refusal=False):
        """refusal: the one documented refusal may be drawn -- the result's class plan is no longer the one the context's lists describe"""
        if res not in self.sized or res not in self.model.results:
            return False
        if self.model.results[res]["made"]["classed"] and self.model.cls_owner != res and not refusal:
            return False
        batch, version, _, _, env, prepares = self.sized[res]
        b = self.model.batches.get(batch)
        return b is not None and b["version"] == version and env == self.model.env and prepares == self.prepares and len(b["seqs"]) > 0

    def timed(self, res, refusal=False):
        assert self.timed_ok(res, refusal)
        batch, _, k, _, _, _ = self.sized[res]
        self.work += sum(len(x) for x in self.model.batches[batch]["seqs"]) // 4
        self.emit(dict(kind="timed", res=res, batch=batch, sketch=k, p=self.model.results[res]["p"], warmup=int(self.rng.integers(0, 2)), iters=int(self.rng.integers(1, 3))))

    # -- read steps
    def read(self, res, how=None, **kw):
        r = self.model.results[res]
        n = r["n"]
        hows = [h for h in READS if n > 0 or h in ("info", "fetch", "status", "digest")]  # (an empty result: only the entries that take a range of 0 reads)
        how = how or self.choice(hows)
        step = dict(kind="read", res=res, how=how)
        if how in ("fetch", "narrow", "status"):
            inner = n >= 3 and self.rng.random() < 0.5  # the range that begins past read 0 and ends before n
            first = int(self.rng.integers(1, n - 1)) if inner else 0
            step.update(first=first, count=int(self.rng.integers(1, n - first)) if inner else n)
        if how in ("sets", "counted"):
            step.update(whole=bool(self.rng.random() < 0.4), scale=int(self.choice((1, 9))))
        step.update(kw)
        self.emit(step)
        if how == "compact":
            self.compact_at = len(self.steps) - 1

    def compact_read(self):
        if self.compact_at is not None:
            self.emit(dict(kind="compact_read", since=len(self.steps) - 1 - self.compact_at))
            self.compact_at = None

    def release(self, res):
        self.emit(dict(kind="release", res=res, tuples=len(self.model.results[res]["hash"])))
        self.sized.pop(res, None)

    def switch(self, env):
        if env != self.model.env:
            self.emit(dict(kind="switch", env=dict(env)))

    def destroy(self, slot):
        self.emit(dict(kind="destroy", slot=slot))

    def random_read(self):
        live = list(self.model.results)
        if live:
            self.read(self.choice(live))
        elif self.model.batches:
            self.sketch(self.choice(list(self.model.batches)))

    def random_step(self):
        """one step drawn from everything a program may do at this point"""
        rng, M = self.rng, self.model
        room = self.bases < BASES_BUDGET and self.work < ORACLE_BUDGET
        kinds = ["read"] * 4 + ["sketch"] * 7 + ["make", "make", "refill", "refill", "translate", "destroy", "release", "switch", "timed", "prepare", "make2", "compact_read"]
        k = self.choice(kinds)
        dna = [i for i, b in M.batches.items() if not b["protein"]]
        if k == "read" or not room:
            return self.random_read()
        if k == "make" and len(M.batches) < 4:
            r = rng.random()
            if r < 0.2:
                return self.make(protein_reads(rng), True, "protein")
            if r < 0.3:
                return self.make([], note="empty")
            if r < 0.4 and self.bases < BASES_BUDGET // 2:
                return self.make(dna_reads(rng, "big", "acgt"), note="big, acgt")
            if r < 0.5:
                return self.make(dna_reads(rng, "long5000", self.choice(("acgt", "fewN"))), note="long5000")
            seqs, note = self.draw_dna()
            if self.bases + sum(len(q) for q in seqs) > BASES_BUDGET:
                return self.random_read()
            return self.make(seqs, note=note)
        if k == "make2" and len(M.batches) < 3:
            a, b = self.draw_dna(("ragged", "fixed")), self.draw_dna(("ragged", "fixed"))
            if self.bases + sum(len(q) for q in a[0] + b[0]) > BASES_BUDGET:
                return self.random_read()
            return self.emit(dict(kind="make2", a=self.make_step(a[0], note=a[1]), b=self.make_step(b[0], note=b[1])))
        if k == "refill" and M.batches:
            slot = self.choice(list(M.batches))
            if M.batches[slot]["protein"]:
                return self.refill(slot, protein_reads(rng), note="protein")
            seqs, note = self.draw_dna()
            if self.bases + sum(len(q) for q in seqs) > BASES_BUDGET:
                return self.random_read()
            return self.refill(slot, seqs, note=note)
        if k == "translate" and dna and len(M.batches) < 4:
            src = self.choice(dna)
            if max((len(q) for q in M.batches[src]["seqs"]), default=0) < 5000 and M.batches[src]["seqs"]:
                return self.emit(dict(kind="translate", src=src, slot=self.new_batch(), table=int(self.choice(self.codes)), frame=int(self.choice(FRAMES))))
        if k == "destroy" and len(M.batches) > 1:
            return self.destroy(self.choice(list(M.batches)))
        if k == "release" and len(M.results) > 1:
            return self.release(self.choice(list(M.results)))
        if k == "switch":
            return self.switch(self.choice(ENVS))
        if k == "timed":
            ok = [r for r in M.results if self.timed_ok(r)]
            if ok:
                return self.timed(self.choice(ok))
        if k == "prepare" and M.batches:
            b = self.choice(list(M.batches))
            if M.batches[b]["protein"]:
                return self.random_read()
            kind, p = self.params(self.choice(("minimizer", "syncmer", "nthash")))
            self.prepares += 1
            return self.emit(dict(kind="prepare", batch=b, sketch=kind, p=p))
        if k == "compact_read":
            return self.compact_read()
        if k == "sketch" and M.batches:
            b = self.choice(list(M.batches))
            reuse = self.choice(list(M.results)) if M.results and rng.random() < 0.6 else None
            if len(M.results) >= 4 and reuse is None:
                reuse = self.choice(list(M.results))
            return self.sketch(b, reuse, reads=len(self.steps) + 2 <= 20)
        return self.random_read()


# -- the themes: the first steps of a program, one per kind of state that outlives a call
def _theme_reserve(g):
    """release -> sketch pairs of results whose arrays pass the reserve's size rule: descending tuple counts on one fixed-length batch"""
    n = int(g.rng.integers(1700, 2201))
    b = g.make([_dna(g.rng, 150) for _ in range(n)], note="fixed, acgt, %d reads" % n)
    res = None
    for kind, p in (("nthash", dict(k=21, canonical=True)), ("kmer", dict(k=32, canonical=True)), ("simhash", dict(k=70, m=6, scale=3))):
        if res is not None:
            g.release(res)
        res = g.sketch(b, None, kind, p, reads=False)
        g.read(res, g.choice(("digest", "status", "info")))
    g.read(res, "fetch", first=3, count=40)
    g.work = ORACLE_BUDGET  # (no further sketch of this batch: the steps that follow read)


def _theme_kinds(g):
    """one result object through every kind, position and every-position kinds in turn"""
    seqs, note = g.draw_dna(("ragged",), ("acgt", "fewN", "iupac"))
    b = g.make(seqs[:120], note=note)
    res = None
    tables = list(g.block_tables()[2:])
    for kind in ("minimizer", "nthash", "syncmer", "kmer", "prot_minimizer", "simhash", "minimizer", "prot_hash", "syncmer"):
        p = None
        if kind.startswith("prot_"):
            p = dict(g.params(kind, True)[1], codon_table=tables.pop(), frame=int(g.choice(FRAMES)))
        res = g.sketch(b, res, kind, p, reads=False) or res
        g.read(res, g.choice(("fetch", "device", "narrow")))


def _theme_sizes(g):
    """one result object through batches of growing and shrinking n (n_cap), another kind each time"""
    res = b = None
    for i, n in enumerate((1, 65, 63, 513, 64, 512)):
        seqs = [_dna(g.rng, 150) for _ in range(n)]
        if b is None:
            b = g.make(seqs, note="%d reads" % n)
        else:
            g.refill(b, seqs, prefer=("ascii", "packed")[i % 2], note="%d reads" % n)
        res = g.sketch(b, res, reads=False) or res
        g.read(res, g.choice(("fetch", "device", "status")))


def _theme_tiles(g):
    """tiled and untiled calls in turn on one context: slots 0-9 between two tiled calls serve bsk_result_sets, one result goes wide and back"""
    g.switch(TILED_40 if g.rng.random() < 0.5 else TILED_64)
    b = g.make(dna_reads(g.rng, "long", g.choice(("acgt", "fewN")))[:12], note="long")
    short = g.make(dna_reads(g.rng, "tooshort", "acgt")[:30] + [_dna(g.rng, 30)], note="too short for most kinds")
    r0 = g.sketch(b, None, "minimizer", reads=False)
    other = g.sketch(short, None, "nthash", dict(k=21, canonical=True), reads=False)
    g.read(other, "sets", whole=True, scale=1)
    g.read(r0, "sets", whole=False, scale=1)
    r1 = g.sketch(b, None, "syncmer", reads=False)
    g.read(r1, "device")
    for env, kind in (({"BSK_NO_TILES": "1"}, "nthash"), (TILED_40, "kmer"), ({"BSK_NO_TILES": "1"}, "minimizer")):
        g.switch(env)
        g.sketch(b, r0, kind, reads=False)
        g.read(r0, g.choice(("fetch", "device", "digest")))
    g.read(other, "counted", whole=True, scale=1)


def _theme_fetches(g):
    """the pool slots the fetches share: fetch -> narrow -> fetch on different results, compact arrays read back after other calls"""
    a = g.make(g.draw_dna(("ragged", "fixed"))[0][:300])
    b = g.make(protein_reads(g.rng), True, "protein")
    r0, r1 = g.sketch(a, None, "minimizer", reads=False), g.sketch(b, None, "prot_hash", reads=False)
    r2 = g.sketch(a, None, "kmer", reads=False) or g.sketch(a, None, "nthash", reads=False)
    g.read(r0, "compact")
    g.read(r0, "fetch")
    g.read(r1, "narrow")
    g.read(r2, "fetch")
    g.compact_read()
    g.read(r2, "compact")
    g.read(r0, "narrow")
    g.read(r1, "device")
    g.read(r0, "sets", whole=True, scale=9)
    g.compact_read()


def _theme_classes(g):
    """two class-plan results alive at once: the pooled lists belong to the younger one, so the timed re-run of the older is refused
    and leaves it as it was; sketched again it runs, and then the other one's is refused"""
    g.switch(CLASSED if g.rng.random() < 0.5 else dict(CLASSED, BSK_CLASS_VIEW="1"))
    a, b = g.make(dna_reads(g.rng, "classmix", "acgt"), note="classmix"), g.make(dna_reads(g.rng, "classmix", g.choice(("acgt", "fewN"))), note="classmix")
    p = g.choice((dict(k=21, w=11), dict(k=15, w=7)))
    r0 = g.sketch(a, None, "minimizer", p, reads=False)
    r1 = g.sketch(b, None, g.choice(("minimizer", "syncmer")), reads=False)
    g.read(r1, "digest")
    g.timed(r0, refusal=True)  # refused: "call bsk_sketch first"
    g.sketch(a, r0, "minimizer", p, reads=False)
    g.timed(r0)
    g.read(r0, "narrow", first=0, count=g.model.results[r0]["n"])
    g.timed(r1, refusal=True)  # now the lists are r0's
    g.read(r1, "device")


def _theme_translate(g):
    """the cached codon table: two translations with different tables, then the first table again"""
    b = g.make(g.draw_dna(("ragged",), ("acgt", "iupac", "junk"))[0][:150])
    t1, t2 = g.block_tables()[:2]  # (over the campaign: every genetic code)
    assert g.O.genetic_code(t1) != g.O.genetic_code(t2)
    res = None
    for i, t in enumerate((t1, t2, t1)):
        frame = int(g.choice(FRAMES))
        slot = g.new_batch()
        g.emit(dict(kind="translate", src=b, slot=slot, table=t, frame=frame))
        kind, p = g.params("prot_minimizer" if i % 2 else "prot_hash", False)
        res = g.sketch(b, res, kind, dict(p, codon_table=t, frame=frame), reads=False) or res
        g.read(res, "fetch")
        if i == 2:  # the translated batch through the protein path: the same values
            r2 = g.sketch(slot, None, kind, {k: v for k, v in p.items() if k not in ("codon_table", "frame")}, reads=False)
            g.read(r2, "digest")
        g.destroy(slot)


def _theme_refill(g):
    """one batch object re-filled through both entries in turn: pure ACGT, flagged, fixed-length, ragged and empty contents in every order"""
    rng = g.rng
    n = int(rng.integers(66, 140))

    def content(state):
        if state == "E":
            return []
        lens = [150] * n if state[1] == "X" else [int(x) for x in rng.integers(30, 301, int(rng.integers(40, 140)))]
        seqs = [_dna(rng, x) for x in lens]
        return [_flag(rng, q, "fewN") if rng.random() < 0.5 else q for q in seqs] if state[0] == "F" else seqs

    order = ("PX", "FR", "FR", "E", "PX", "PX", "E", "FR", "PX")
    slot = g.make(content(order[0]), note=order[0])
    res = g.sketch(slot, None, "minimizer", dict(k=21, w=11), reads=False)
    for i, state in enumerate(order[1:]):
        g.refill(slot, content(state), prefer=("ascii", "packed")[i % 2], note=state)
        if state != "E" and i in (0, 1, 3, 4, 7):
            res = g.sketch(slot, res, g.choice(("minimizer", "nthash", "syncmer", "simhash")), reads=False) or res
            g.read(res, "status", first=0, count=g.model.results[res]["n"])


def _theme_pairs(g):
    """two batches made back to back before either is used (the descriptors go through the context's pinned staging), and a fresh result
    right after a release (the status bytes of the released one)"""
    style = g.choice(("acgt", "fewN", "manyN"))
    a, b = ([_flag(g.rng, q, style) if style != "acgt" and g.rng.random() < 0.3 else q for q in (_dna(g.rng, 150) for _ in range(511))], "511 reads, " + style), g.draw_dna(("ragged",))
    g.emit(dict(kind="make2", a=g.make_step(a[0], note=a[1]), b=g.make_step(b[0][:150], note=b[1])))
    sa, sb = g.steps[-1]["a"]["slot"], g.steps[-1]["b"]["slot"]
    r0 = g.sketch(sb, None, "minimizer", reads=False)
    r1 = g.sketch(sa, None, "nthash", reads=False)
    g.read(r0, "info")
    g.read(r1, "digest")
    g.release(r1)
    short = g.make([_dna(g.rng, int(x)) for x in g.rng.integers(0, 30, 80)], note="mostly too short")
    r2 = g.sketch(short, None, "syncmer", dict(k=31, s=11), reads=False)
    g.read(r2, "status", first=0, count=80)
    g.timed(r2)


_THEMES = dict(reserve=_theme_reserve, kinds=_theme_kinds, sizes=_theme_sizes, tiles=_theme_tiles, fetches=_theme_fetches, classes=_theme_classes,
               translate=_theme_translate, refill=_theme_refill, pairs=_theme_pairs)


def program(seed, O=None):
    return program_and_records(seed, O)[0]


def program_and_records(seed, O=None):
    """the program of a seed and the model's records of it (the generator runs the model as it goes)"""
    if O is None:
        from oracle import oracle as O
    clear_cache()
    g = _Gen(seed, O)
    todo = int(g.rng.integers(12, 21))
    theme = theme_of(seed)
    if theme == "random":
        blk, j = (seed - BASE) // PER_BLOCK, (seed - BASE) % PER_BLOCK - THEMES.index("random")  # the j-th random program of its block
        seqs, note = (dna_reads(g.rng, "big", "acgt"), "big, acgt") if j == 1 else (dna_reads(g.rng, "long5000", "fewN"), "long5000, fewN") if j == 0 and blk % 2 else g.draw_dna()
        b = g.make(seqs, note=note)
        if j == 1:  # a read of 32 768 bases or more: the narrow fetch refuses the range that holds its last positions
            res = g.sketch(b, None, g.choice(("minimizer", "syncmer")), reads=False)
            g.read(res, "narrow", first=0, count=len(seqs))
            g.read(res, "narrow", first=0, count=len(seqs) - 1)
        g.switch(ENVS[(blk * 6 + j) % len(ENVS)])  # (over the campaign: every option)
    else:
        _THEMES[theme](g)
    guard = 0
    while len(g.steps) < todo and guard < 200:
        guard += 1
        g.random_step()
    return g.steps, run(g.steps, Model(O))  # (the back-ends put the options back when a program ends)


# ---- the text of a program ----
def _crc(seqs):
    return "%08x" % zlib.crc32(b"/".join(seqs))


def _reads_text(seqs):
    lens = [len(q) for q in seqs]
    return "%d reads of %s..%s bases, %d flagged, crc %s" % (len(seqs), min(lens, default=0), max(lens, default=0), sum(flagged(q) for q in seqs), _crc(seqs))


def _params_text(kind, p):
    return "%s(%s)" % (kind, ", ".join("%s=%s" % kv for kv in p.items()))


def describe_step(i, s):
    k = s["kind"]
    if k in ("make", "refill"):
        entry = ("bsk_batch_from_%s" if k == "make" else "bsk_batch_refill_%s") % s["how"]
        text = "%s = %s(%s%s) [%s]" % (s["slot"], entry, "protein, " if s["protein"] else "", _reads_text(s["seqs"]), s["note"])
    elif k == "make2":
        text = "back to back: " + "; ".join(describe_step(i, x)[4:] for x in (s["a"], s["b"]))
    elif k == "translate":
        text = "%s = bsk_batch_translate(%s, table %d, frame %d)" % (s["slot"], s["src"], s["table"], s["frame"])
    elif k == "destroy":
        text = "bsk_batch_destroy(%s)" % s["slot"]
    elif k == "switch":
        text = "options: %s" % (" ".join("%s=%s" % kv for kv in s["env"].items()) or "none")
    elif k == "prepare":
        text = "bsk_batch_prepare(%s, %s)" % (s["batch"], _params_text(s["sketch"], s["p"]))
    elif k == "sketch":
        text = "%s = bsk_sketch(%s, %s)%s" % (s["res"], s["batch"], _params_text(s["sketch"], s["p"]), "" if s["fresh"] else " into the object that held %s" % (s["before"],))
    elif k == "timed":
        text = "bsk_sketch_timed(%s, %s, warmup %d, iters %d) on %s" % (s["batch"], _params_text(s["sketch"], s["p"]), s["warmup"], s["iters"], s["res"])
    elif k == "read":
        args = ", ".join("%s=%s" % (a, s[a]) for a in ("first", "count", "whole", "scale") if a in s)
        text = "%s.%s(%s)" % (s["res"], s["how"], args)
    elif k == "compact_read":
        text = "the compact arrays read back (%d calls later)" % s["since"]
    else:
        assert k == "release", k
        text = "bsk_result_release(%s) [%d tuples]" % (s["res"], s["tuples"])
    return "%2d  %s%s" % (i, text, "; then %s is fetched again" % s["recheck"] if s.get("recheck") is not None else "")


def describe(prog, upto=None):
    return "\n".join(describe_step(i, s) for i, s in enumerate(prog[:upto]))


def message(seed, i, prog, what):
    """what an assertion says: the seed, the step and the program up to it"""
    return "seed %#x (%s), step %d: %s\n%s\n(python -m tests.sketch_programs %#x)" % (seed, theme_of(seed), i, what, describe(prog, i + 1), seed)


# ---- the contract a program must stay inside, walked step by step ----
def contract_violations(prog):
    """every step that leaves the header's contract, as text; [] for a program inside it"""
    bad, batches, results, env, prepares, compact = [], {}, {}, {}, 0, False
    for i, s in enumerate(prog):
        k = s["kind"]
        for x in ([s["a"], s["b"]] if k == "make2" else [s] if k in ("make", "refill") else []):
            if x["kind"] == "make" and x["slot"] in batches:
                bad.append("%d: makes a batch into the live slot %s" % (i, x["slot"]))
            if x["kind"] == "refill" and (x["slot"] not in batches or batches[x["slot"]]["protein"] != x["protein"]):
                bad.append("%d: re-fills %s with another alphabet, or a dead slot" % (i, x["slot"]))
            if x["how"] == "packed" and not packable(x["seqs"]):
                bad.append("%d: packs reads that are not pure ACGT" % i)
            old = batches.get(x["slot"])
            batches[x["slot"]] = dict(protein=x["protein"], version=old["version"] + 1 if old else 0, n=len(x["seqs"]), longest=max((len(q) for q in x["seqs"]), default=0))
        if k == "translate":
            if s["src"] not in batches or batches[s["src"]]["protein"] or s["slot"] in batches or s["frame"] not in FRAMES:
                bad.append("%d: translate of a dead or protein batch, into a live slot, or with a bad frame" % i)
            batches[s["slot"]] = dict(protein=True, version=0, n=batches[s["src"]]["n"], longest=0)
        elif k == "destroy":
            if batches.pop(s["slot"], None) is None:
                bad.append("%d: destroys a dead batch" % i)
        elif k == "switch":
            if set(s["env"]) - set(SWITCHES):
                bad.append("%d: a switch outside the allowed ones: %s" % (i, sorted(set(s["env"]) - set(SWITCHES))))
            env = dict(s["env"])
        elif k == "prepare":
            prepares += 1
            if s["batch"] not in batches:
                bad.append("%d: prepare of a dead batch" % i)
        elif k == "sketch":
            b = batches.get(s["batch"])
            if b is None or (b["protein"] and not s["sketch"].startswith("prot_")) or (s["sketch"], {x: v for x, v in s["p"].items() if x not in ("codon_table", "frame")}) not in \
                    [(kk, pp) for kk, pp in PARAMS]:
                bad.append("%d: sketch of a dead batch, a DNA kind on proteins, or parameters outside the list" % i)
            if s["fresh"] != (s["res"] not in results):
                bad.append("%d: `fresh` is wrong" % i)
            results[s["res"]] = dict(batch=s["batch"], version=b["version"] if b else -1, key=(s["sketch"], pkey(s["p"])), env=dict(env), prepares=prepares, n=b["n"] if b else 0)
        elif k == "timed":
            r, b = results.get(s["res"]), batches.get(s["batch"])
            if r is None or b is None or r["batch"] != s["batch"] or r["version"] != b["version"] or r["key"] != (s["sketch"], pkey(s["p"])) or r["env"] != env or \
                    r["prepares"] != prepares or not (0 <= s["warmup"] <= 1 and 1 <= s["iters"] <= 2):
                bad.append("%d: a timed re-run outside its contract (same batch, not re-filled, same parameters and options as the call that sized the result)" % i)
        elif k == "read":
            r = results.get(s["res"])
            if r is None:
                bad.append("%d: reads a released result" % i)
            elif "first" in s and not (0 <= s["first"] and s["first"] + s["count"] <= r["n"]):
                bad.append("%d: a range outside the result" % i)
            elif r["n"] == 0 and s["how"] not in ("info", "fetch", "status", "digest"):
                bad.append("%d: %s of an empty result" % (i, s["how"]))
            if s["how"] == "compact":
                compact = True
        elif k == "compact_read":
            if not compact:
                bad.append("%d: compact arrays read after the next compact, or before the first" % i)
            compact = False
        elif k == "release":
            if results.pop(s["res"], None) is None:
                bad.append("%d: releases a dead result" % i)
        others = set(results) - {s.get("res")}
        if (s.get("recheck") is None and others) or (s.get("recheck") is not None and s["recheck"] not in others):
            bad.append("%d: %s" % (i, "no other live result is fetched again" if s.get("recheck") is None else "re-checks a dead result, or the step's own"))
    return bad


# ---- what a campaign reaches ----
def figures(programs_and_records):
    """counts over programs with their model records: what tests/test_sketch_programs.py holds the campaign to"""
    f = dict(kinds=set(), kind_changes=0, pos_to_stream=0, stream_to_pos=0, grows=0, layout_changes=0, refill_orders=set(), tiled_sets_tiled=0, fetch_narrow_fetch=0,
             compact_later=0, class_pairs_timed=0, table_aba=0, reserve_pairs=0, tables=set(), frames=set(), steps=0, refused=0, reads=set(), entries=set(),
             switches=set(), shapes=set(), bases=[], both_refills=0)
    for prog, recs in programs_and_records:
        results, batches, classed_alive, tables, last, released, how3, calls_since_tiled = {}, {}, {}, [], None, None, [], None
        bases = 0
        for i, (s, rec) in enumerate(zip(prog, recs)):
            k = s["kind"]
            f["steps"] += 1
            step_rec = rec["step"] if s.get("recheck") is not None else rec
            f["refused"] += isinstance(step_rec, dict) and "refused" in step_rec
            for x in ([s["a"], s["b"]] if k == "make2" else [s] if k in ("make", "refill") else []):
                bases += sum(len(q) for q in x["seqs"])
                f["entries"].add(("bsk_batch_from_" if x["kind"] == "make" else "bsk_batch_refill_") + x["how"])
                cats = {"empty"} if not x["seqs"] else {("flagged" if any(flagged(q) for q in x["seqs"]) else "pure") if not x["protein"] else "protein",
                                                         "fixed" if len({len(q) for q in x["seqs"]}) == 1 else "ragged"}
                if x["kind"] == "refill":
                    f["refill_orders"] |= {(a, b) for a in batches[x["slot"]]["cats"] for b in cats}
                    batches[x["slot"]]["hows"].add(x["how"])
                    f["both_refills"] += batches[x["slot"]]["hows"] == {"ascii", "packed"} and not batches[x["slot"]]["counted"]
                    batches[x["slot"]]["counted"] |= batches[x["slot"]]["hows"] == {"ascii", "packed"}
                    batches[x["slot"]]["cats"] = cats
                else:
                    batches[x["slot"]] = dict(cats=cats, hows=set(), counted=False)
            if k == "translate":
                f["tables"].add(s["table"])
                f["frames"].add(s["frame"])
                tables.append(s["table"])
                f["table_aba"] += len(tables) >= 3 and tables[-1] == tables[-3] != tables[-2]
                batches[s["slot"]] = dict(cats={"protein"}, hows=set(), counted=False)
            elif k == "switch":
                f["switches"] |= set(s["env"])
            elif k == "sketch":
                f["kinds"].add(s["sketch"])
                if "codon_table" in s["p"]:
                    f["tables"].add(s["p"]["codon_table"])
                    f["frames"].add(s["p"]["frame"])
                old, new = s["before"], step_rec
                if old is not None:
                    f["kind_changes"] += old["kind"] != s["sketch"]
                    f["pos_to_stream"] += old["has_pos"] and not new["has_pos"]
                    f["stream_to_pos"] += new["has_pos"] and not old["has_pos"]
                    f["grows"] += new["n_reads"] > old["n_reads"]
                    f["layout_changes"] += old["tiled"] != s["tiled"]
                elif released is not None and released[0] == i - 1:
                    t = step_rec["n_tuples"]
                    f["reserve_pairs"] += RESERVE_TUPLES <= t <= released[1] <= 2 * t + RESERVE_SLACK_TUPLES
                results[s["res"]] = s
                if s["classed"]:
                    classed_alive[s["res"]] = i
                else:
                    classed_alive.pop(s["res"], None)
                if s["tiled"]:
                    f["tiled_sets_tiled"] += calls_since_tiled == "sets"
                    calls_since_tiled = "tiled"
            elif k == "timed":
                f["entries"].add("bsk_sketch_timed")
                f["class_pairs_timed"] += s["res"] in classed_alive and any(j > classed_alive[s["res"]] for r, j in classed_alive.items() if r != s["res"])
            elif k == "read":
                f["reads"].add(s["how"])
                if s["how"] in ("fetch", "narrow"):
                    how3 = (how3 + [(s["how"], s["res"])])[-3:]
                    f["fetch_narrow_fetch"] += [h for h, _ in how3] == ["fetch", "narrow", "fetch"] and len({r for _, r in how3}) == 3
                if s["how"] in ("sets", "counted") and calls_since_tiled == "tiled":
                    calls_since_tiled = "sets"
            elif k == "compact_read":
                f["compact_later"] += s["since"] >= 2
            elif k == "release":
                released = (i, s["tuples"])
                results.pop(s["res"], None)
                classed_alive.pop(s["res"], None)
        f["bases"].append(bases)
    return f


if __name__ == "__main__":
    for arg in sys.argv[1:]:
        print("program %#x (%s)" % (int(arg, 0), theme_of(int(arg, 0))))
        print(describe(program(int(arg, 0))))
