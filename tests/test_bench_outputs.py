"""bench.py --dump-outputs: what the timed path's last step computed, as float64 .npy files that two builds compare file for file.

CPU: dump_outputs() over a stand-in result -- files, exact u64 halves, the seeded sample, the size bound at the headline size.
GPU: a plain bench run writes the sample, its tuples equal what bsk_sketch gives a caller for the same reads, and the run times
exactly --steps launches with none of the --full side measurements in its line.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

MIX = 0x9E3779B97F4A7C15


class StandIn:
    """A result of n reads with `per` tuples each, every value a function of its index."""

    def __init__(self, n, per, has_pos=True):
        self.n, self.per, self.has_pos = n, per, has_pos

    def info(self):
        return dict(n_reads=self.n, n_tuples=self.n * self.per, has_pos=self.has_pos)

    def digest(self):
        return dict(checksum=0xFEDCBA9876543210, n_tuples=self.n * self.per, short=1, illegal=2, first_window_tie=3, has_non_acgt=4)

    def fetch(self, first, count):
        offs = np.arange(count + 1, dtype=np.uint64) * np.uint64(self.per)
        status = ((first + np.arange(count)) % 7).astype(np.uint8)
        t = np.arange(first * self.per, (first + count) * self.per, dtype=np.uint64)
        h = t * np.uint64(MIX)
        return offs, status, h, ((t & np.uint64(0xFFFF)).astype(np.uint32) | np.uint32(1 << 31)) if self.has_pos else None


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_stand_in(tmp_path):
    _, n, read_len, k, _, _ = bench.WORKLOADS["minimizer"]
    res = StandIn(n, read_len - k + 1)  # the most tuples a read can yield: the size bound holds at the headline size
    bench.dump_outputs(res, str(tmp_path / "a"), read_len, k, 0x5EED0003)
    a = load(tmp_path / "a")
    assert set(a) == {"digest", "read_index", "status", "tuples_per_read", "hash_hi", "hash_lo", "pos"}
    assert all(v.dtype == np.float64 for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / (f + ".npy")) for f in a) <= 64 << 20
    ck = 0xFEDCBA9876543210
    assert a["digest"].tolist() == [n, n * res.per, ck >> 32, ck & 0xFFFFFFFF, 1, 2, 3, 4]
    idx = a["read_index"].astype(np.uint64)
    assert idx.size >= 1000 and np.all(np.diff(idx.astype(np.int64)) > 0) and idx.size % bench.DUMP_BLOCK == 0
    assert np.array_equal(a["status"], (idx % np.uint64(7)).astype(np.float64))
    assert np.all(a["tuples_per_read"] == res.per)
    t = (idx[:, None] * np.uint64(res.per) + np.arange(res.per, dtype=np.uint64)[None, :]).ravel()
    h = a["hash_hi"].astype(np.uint64) << np.uint64(32) | a["hash_lo"].astype(np.uint64)
    assert np.array_equal(h, t * np.uint64(MIX))  # exact: no u64 bit lost to float64
    assert np.array_equal(a["pos"].astype(np.uint64), (t & np.uint64(0xFFFF)) | np.uint64(1 << 31))
    # the same arguments give the same files; another seed another sample
    bench.dump_outputs(res, str(tmp_path / "b"), read_len, k, 0x5EED0003)
    b = load(tmp_path / "b")
    assert all(np.array_equal(a[f], b[f]) for f in a)
    bench.dump_outputs(res, str(tmp_path / "c"), read_len, k, 0x5EED0004)
    assert not np.array_equal(load(tmp_path / "c")["read_index"], a["read_index"])


def test_dump_outputs_small_and_positionless(tmp_path):
    res = StandIn(100, 5, has_pos=False)  # fewer reads than a block: one block of all of them
    bench.dump_outputs(res, str(tmp_path), 150, 21, 1)
    a = load(tmp_path)
    assert "pos" not in a and a["read_index"].tolist() == list(range(100)) and a["hash_hi"].size == 500


@pytest.mark.gpu
def test_bench_dump_outputs_equal_the_callers_result(engine, tmp_path):
    from bio_amd import _lib as L
    n, steps = 300_000, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--reads", str(n),
           "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["steps"] == steps and out["roofline"]["launches_timed"] == steps and out["ms_per_step"] > 0
    assert not {"cpu_baseline", "end_to_end", "plain_call", "dense_copy"} & set(out) and "power" not in out["roofline"]
    a = load(tmp_path)
    # the same batch and parameters in this process (bench.py: rank 0's synthetic stream, k=21 w=11)
    b = engine.synth(L.ALPHA_DNA, n, 150, 0x5EED0003)
    res = engine.run(b, engine.params(L.MINIMIZER, 21, w=11))
    dg = res.digest()
    assert a["digest"][:2].tolist() == [n, dg["n_tuples"]] and int(a["digest"][2]) << 32 | int(a["digest"][3]) == dg["checksum"]
    assert dg["n_tuples"] == out["config"]["tuples_per_gpu"]
    idx = a["read_index"].astype(np.int64)
    starts = idx[::bench.DUMP_BLOCK]
    got_h = a["hash_hi"].astype(np.uint64) << np.uint64(32) | a["hash_lo"].astype(np.uint64)
    hs, ps, sts, cnt = [], [], [], []
    for s in starts:
        offs, st, h, pp = res.fetch(int(s), bench.DUMP_BLOCK)
        hs.append(h)
        ps.append(pp)
        sts.append(st)
        cnt.append(np.diff(offs))
    assert np.array_equal(got_h, np.concatenate(hs))
    assert np.array_equal(a["pos"].astype(np.uint32), np.concatenate(ps))
    assert np.array_equal(a["status"].astype(np.uint8), np.concatenate(sts))
    assert np.array_equal(a["tuples_per_read"].astype(np.uint64), np.concatenate(cnt))
    res.close()
    b.close()
