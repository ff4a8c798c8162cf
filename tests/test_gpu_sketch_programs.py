"""GPU: seeded programs over the sketch-side entries against the oracle (tests/sketch_programs.py), exactly.

A program owns a few batches and a few results on one context and runs 12 to 20 steps over them: batches made, re-filled through both
entries in turn, translated, destroyed, two made back to back; bsk_sketch into a fresh result or into one any other batch, kind or
layout made, bsk_sketch_timed and bsk_batch_prepare inside their contracts; every read entry -- info, fetch, fetch_narrow,
fetch_status, digest, sets, counted sets, compact (its arrays read back calls later), and bsk_result_device / _device_wide decoded on
the host from the raw arrays; releases; switches of the BSK_* options that move small batches across plan boundaries.  After EVERY
step the device's record is compared with the model's (status code, the kind's flag bits, hashes, positions, strands of every read),
every step that leaves another result alive fetches one of them (drawn) again, and at the end every live result and batch is read once more: a later call must not
have damaged an earlier object, and a result must outlive its batch.  The programs of a block run on ONE context of this module's
own, the odd ones on a second, so that what a context keeps between calls accumulates; per block at least one result must have
received an array back from the reserve of released results (a pointer a released result held).

A failure names its block, seed and step, the seeds that ran on that context before, and prints the program up to there;
`python -m tests.sketch_programs SEED` prints all of it.  tests/test_sketch_programs.py shows on the CPU what the campaign reaches
and that this comparison catches each of twelve stale-state models.

Time, one MI355X, one `pytest --durations=0` run: the slowest test here (8 programs) 0.52 s, the slowest test_differential_fuzz
block 1.14 s (the bound is 1.5 x that)."""
import ctypes as C
import os

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests import sketch_programs as SP

pytestmark = pytest.mark.gpu
U64, U32, U8 = np.uint64, np.uint32, np.uint8
KIND = dict(minimizer=L.MINIMIZER, syncmer=L.SYNCMER, nthash=L.NTHASH, kmer=L.KMER, simhash=L.SIMHASH, prot_hash=L.PROT_HASH, prot_minimizer=L.PROT_MINIMIZER)
SLICE = 8  # programs per test: half a block
RAW_LIMIT = 32 * SP.BASES_BUDGET  # tuples: a program's batches hold at most BASES_BUDGET bases, a read's tuples lie at most 64 apart, a plan's slabs leave gaps


@pytest.fixture(scope="module")
def engines():
    a, b = S.Engine(0), S.Engine(0)
    yield a, b
    b.close()
    a.close()


SP_TILES = "(over tiles)"
HISTORY = {0: [], 1: []}  # the seeds that ran on either context so far


def d2h(eng, ptr, n, dt):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    a = np.empty(n, dt)
    if n:
        assert ptr, "NULL device array"
        eng.sync()
        assert hip.hipMemcpy(a.ctypes.data, ptr, a.nbytes, 2) == 0
    return a


class Device:
    """one program on one engine: the device side of sketch_programs.Model"""

    def __init__(self, eng):
        self.eng = eng
        self.batches, self.protein, self.results, self.kinds, self.compact = {}, {}, {}, {}, None
        self.released, self.reserve_hits, self.plans, self.timed_refused = set(), 0, [], 0
        self.saved = {k: os.environ.get(k) for k in SP.SWITCHES}
        self._env({})

    def _env(self, env):
        for k in SP.SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)

    # -- batches
    def _make(self, s):
        if s["how"] == "packed":
            words, _, desc = SP.pack(s["seqs"])
            return self.eng.batch_from_packed(words, desc)
        return self.eng.batch(s["seqs"], L.ALPHA_PROTEIN if s["protein"] else L.ALPHA_DNA)

    def batch_record(self, slot, protein):
        b = self.batches[slot]
        inf = b.info()
        data, offs = b.fetch_ascii(0, inf["n_reads"])
        return dict(n_reads=inf["n_reads"], n_bases=inf["n_bases"], n_non_acgt=None if protein else inf["n_non_acgt_reads"], offsets=offs, bytes=data)

    def make(self, s):
        self.batches[s["slot"]] = self._make(s)
        self.protein[s["slot"]] = s["protein"]
        return self.batch_record(s["slot"], s["protein"])

    def make2(self, s):
        for x in (s["a"], s["b"]):  # both before either is used
            self.batches[x["slot"]] = self._make(x)
            self.protein[x["slot"]] = x["protein"]
        return dict(a=self.batch_record(s["a"]["slot"], s["a"]["protein"]), b=self.batch_record(s["b"]["slot"], s["b"]["protein"]))

    def refill(self, s):
        b = self.batches[s["slot"]]
        if s["how"] == "packed":
            words, _, desc = SP.pack(s["seqs"])
            b.refill_packed(words, desc)
        else:
            offs = np.concatenate([[0], np.cumsum([len(q) for q in s["seqs"]])]).astype(U64)
            data = np.frombuffer(b"".join(s["seqs"]), U8) if offs[-1] else np.zeros(1, U8)
            b.refill(data, offs, L.ALPHA_PROTEIN if s["protein"] else L.ALPHA_DNA)
        return self.batch_record(s["slot"], s["protein"])

    def translate(self, s):
        self.batches[s["slot"]] = self.batches[s["src"]].translate(s["table"], s["frame"])
        self.protein[s["slot"]] = True
        return self.batch_record(s["slot"], True)

    def destroy(self, s):
        self.batches.pop(s["slot"]).close()
        return dict(done=True)

    def switch(self, s):
        self._env(s["env"])
        return dict(done=True)

    def prepare(self, s):
        self.eng.prepare(self.batches[s["batch"]], self.eng.params(KIND[s["sketch"]], **s["p"]))
        return dict(done=True)

    # -- sketches
    def sketch(self, s):
        reuse = self.results.get(s["res"])
        r = self.eng.run(self.batches[s["batch"]], self.eng.params(KIND[s["sketch"]], **s["p"]), reuse=reuse)
        self.results[s["res"]], self.kinds[s["res"]] = r, s["sketch"]
        self.plans.append(r.plan()["kernel"])
        if reuse is None and self.released & {r.device()[x] for x in ("refs", "status", "hash", "pos")}:  # (spare_take serves the reference words first)
            self.reserve_hits += 1
        return r.info()

    def timed(self, s):
        b, p, r = self.batches[s["batch"]], self.eng.params(KIND[s["sketch"]], **s["p"]), self.results[s["res"]]
        try:
            self.eng.run_timed(b, p, s["warmup"], s["iters"], reuse=r)
        except S.DeviceError as e:  # the pooled lists went to a younger class-plan result (include/biosketch.h): refused, the result as it was
            if "class plan belongs to another batch" not in str(e) or not r.h:
                raise
            self.timed_refused += 1
            return dict(refused="BSK_ERR_ARG", all=self.recheck(s["res"]))
        return dict(info=r.info(), all=self.recheck(s["res"]))

    def _fetched(self, slot, offs, status, hash_, pos):
        code, flags = SP.status_parts(self.kinds[slot], status)
        return dict(offsets=offs, code=code, flags=flags, hash=hash_, pos=pos)

    def read(self, s):
        r, how, slot = self.results[s["res"]], s["how"], s["res"]
        if how == "info":
            return r.info()
        if how == "fetch":
            return self._fetched(slot, *r.fetch(s["first"], s["count"]))
        if how == "narrow":
            try:
                return self._fetched(slot, *r.fetch_narrow(s["first"], s["count"]))
            except S.DeviceError as e:
                if "unsupported" not in str(e).lower():
                    raise
                return dict(refused="BSK_ERR_UNSUPPORTED")
        if how == "status":
            code, flags = SP.status_parts(self.kinds[slot], r.fetch_status(s["first"], s["count"]))
            return dict(code=code, flags=flags)
        if how == "digest":
            d = r.digest()
            return dict(checksum=d["checksum"], n_tuples=d["n_tuples"], short=d["short"], illegal=d["illegal"])
        if how == "sets":
            o, v = r.sets(s["whole"], s["scale"])
            return dict(offsets=o, values=v, counts=None)
        if how == "counted":
            c = r.counted_sets(s["whole"], s["scale"])
            try:
                o, v = c.fetch()
                return dict(offsets=o, values=v, counts=c.fetch_counts())
            finally:
                c.close()
        if how == "compact":
            po, ph, pp, nt = r.compact()
            self.compact = (po, ph, pp, nt, r.info()["n_reads"])
            return dict(n_tuples=nt, has_pos=pp is not None)
        assert how == "device", how
        return self.decoded(slot)

    def decoded(self, slot):
        """bsk_result_device / _device_wide, decoded on the host from the raw arrays: tuple j of a read at first + j * stride"""
        r, eng = self.results[slot], self.eng
        inf, p = r.info(), r.device()
        n = inf["n_reads"]
        if p["wide"]:
            first, count = d2h(eng, p["first"], n, U64).astype(np.int64), d2h(eng, p["count"], n, U64).astype(np.int64)
            stride = np.ones(n, np.int64)
        else:
            first, count, stride = SP.decode_refs(d2h(eng, p["refs"], n, U64))
        plan = r.plan()["kernel"]  # refs is NULL exactly for the results of calls that ran over tiles (a class plan's parts may: its result is not wide)
        layout_ok = p["wide"] == bool(p["first"]) == bool(p["count"]) and bool(p["pos"]) == inf["has_pos"] and (" reads of " in plan or p["wide"] == plan.endswith(SP_TILES))
        last = np.where(count > 0, first + (count - 1) * stride, -1)
        extent = int(last.max(initial=-1)) + 1
        assert 0 <= extent <= RAW_LIMIT and int(count.sum()) <= RAW_LIMIT, ("reference words point beyond any array of this batch", extent, int(count.sum()))
        hash_ = d2h(eng, p["hash"], extent, U64)
        pos = d2h(eng, p["pos"], extent, U32) if p["pos"] else None
        return SP.device_record(self.kinds[slot], first, count, stride, d2h(eng, p["status"], n, U8), lambda i: hash_[i], None if pos is None else (lambda i: pos[i]), layout_ok)

    def compact_read(self, s):
        po, ph, pp, nt, n = self.compact
        return dict(n_tuples=nt, offsets=d2h(self.eng, po, n + 1, U64), hash=d2h(self.eng, ph, nt, U64), pos=d2h(self.eng, pp, nt, U32) if pp else None)

    def release(self, s):
        r = self.results.pop(s["res"])
        if s["tuples"] >= SP.RESERVE_TUPLES:
            self.released.add(r.device()["hash"])  # (1 MiB or more: the reserve keeps it, so no other allocation can be handed this address)
        r.close()
        return dict(done=True)

    def recheck(self, slot):
        return self._fetched(slot, *self.results[slot].fetch())

    def end(self):
        return dict(results={i: self.recheck(i) for i in self.results}, batches={i: self.batch_record(i, self.protein[i]) for i in self.batches})

    def close(self):
        for pool in (self.results, self.batches):
            for x in pool.values():
                x.close()
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_program(eng, which, block, seed, oracle):
    prog, want = SP.program_and_records(seed, oracle)
    where = "block %d, context %d after the seeds %s" % (block, which, " ".join("%#x" % s for s in HISTORY[which]) or "(none)")
    HISTORY[which].append(seed)
    dev, i = Device(eng), 0
    try:
        for i, step in enumerate(prog):
            got = SP.run([step], dev, upto=1)[0]
            diff = SP.same(want[i], got)
            assert not diff, where + "\n" + SP.message(seed, i, prog, diff)
        diff = SP.same(want[-1], dev.end())
        assert not diff, where + "\n" + SP.message(seed, len(prog) - 1, prog, ["at the end of the program"] + diff)
    except AssertionError:
        raise
    except Exception as e:  # a call the model expects to succeed was refused
        raise AssertionError(where + "\n" + SP.message(seed, i, prog, "%s: %s" % (type(e).__name__, e))) from e
    finally:
        dev.close()
    return dev


@pytest.mark.parametrize("part", range(SP.PER_BLOCK // SLICE))
@pytest.mark.parametrize("block", range(SP.BLOCKS))
def test_sketch_programs(engines, oracle, block, part):
    hits, done = 0, {}
    for n, seed in enumerate(SP.seeds(block)[part * SLICE:(part + 1) * SLICE]):
        which = (part * SLICE + n) % 2
        dev = run_program(engines[which], which, block, seed, oracle)
        hits += dev.reserve_hits
        done[SP.theme_of(seed)] = dev
    if "reserve" in done:  # spare_take is deterministic, and tests/test_sketch_programs.py pins the sizes: the block's release -> sketch pairs
        assert hits >= 1, "no result of block %d received an array back from the reserve of released results" % block
    if "tiles" in done:  # the options did move these small batches across the plan boundaries the themes are about
        assert any("(over tiles)" in p for p in done["tiles"].plans) and not all("(over tiles)" in p for p in done["tiles"].plans), done["tiles"].plans
    if "classes" in done:
        assert sum(" reads of " in p for p in done["classes"].plans) >= 2 and done["classes"].timed_refused == 2, (done["classes"].plans, done["classes"].timed_refused)
