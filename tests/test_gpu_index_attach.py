"""GPU: bsk_index_attach -- handles of one index for several contexts: the same hits as the owner's, the device arrays shared on one
device (no copy), safe whichever handle is released first, searched from two threads at once; copied once to another device."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

from bio_amd import _lib as L
from bio_amd import sketches as S
from tests.search_cases import collection, ref_search

pytestmark = pytest.mark.gpu
U64 = np.uint64


@functools.lru_cache(None)
def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    hip.hipSetDevice.argtypes = [C.c_int]
    return hip


def free_bytes(device):
    f, t = C.c_size_t(), C.c_size_t()
    assert _hip().hipSetDevice(device) == 0 and _hip().hipMemGetInfo(C.byref(f), C.byref(t)) == 0
    return f.value


def n_devices():
    n = C.c_int()
    L.load().bsk_device_count(C.byref(n))
    return n.value


def case(seed=5, n_targets=60, tsize=150_000, nq=4000):
    """targets of tsize values from a pool (an index of some tens of MB), queries of 0 .. 80 values of the pool or outside it"""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 2**64, 2_000_000, dtype=U64)
    tg = collection([pool[rng.integers(0, len(pool), tsize)] for _ in range(n_targets)])
    qsets = [pool[rng.integers(0, len(pool), int(m))] for m in rng.integers(0, 81, nq)]
    qsets[3] = rng.integers(0, 2**64, 50, dtype=U64)  # (misses)
    qsets[10] = tg[1][int(tg[0][7]):int(tg[0][7]) + 3000]  # 3 000 values of one target
    return tg, collection(qsets)


def fetch(hits):
    return tuple(a.copy() for a in hits.fetch())


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_second_context_on_the_same_device(engine):
    tg, qs = case()
    want = ref_search(*tg, *qs, 1, 0.0, 0.0)
    tsets = engine.sets_from_arrays(*tg)
    ix = tsets.index()
    tsets.close()
    dev_bytes = ix.info()["device_bytes"]
    assert dev_bytes > 20 << 20
    other = S.Engine(0)
    q_own, q_other = engine.sets_from_arrays(*qs), other.sets_from_arrays(*qs)
    own = fetch(ix.search(q_own))
    assert same(own, want)
    other.sync()
    before = free_bytes(0)
    handle = ix.attach(other)
    after = free_bytes(0)
    assert abs(before - after) < dev_bytes // 20, ("a handle on the same device shares the arrays", before - after, dev_bytes)
    assert handle.info() == ix.info()
    got = fetch(handle.search(q_other))
    assert same(got, own)
    for kw in (dict(min_shared=2), dict(min_query_cov=0.05, min_target_cov=0.0001)):
        assert same(fetch(handle.search(q_other, **kw)), fetch(ix.search(q_own, **kw)))
    # a handle is searched on the context it was attached to, and on no other
    hits = C.c_void_p()
    sp = L.SearchParams(1, 0, 0.0, 0.0)
    assert engine.lib.bsk_index_search(engine.ctx, handle.h, q_own.h, C.byref(sp), C.byref(hits)) == L.ERR_ARG and not hits.value
    assert engine.lib.bsk_index_search(other.ctx, ix.h, q_other.h, C.byref(sp), C.byref(hits)) == L.ERR_ARG and not hits.value
    # the owner goes first: the arrays stay with the handle
    engine.sync()
    held = free_bytes(0)
    ix.close()
    assert abs(free_bytes(0) - held) < dev_bytes // 20
    assert handle.info()["device_bytes"] == dev_bytes
    assert same(fetch(handle.search(q_other)), own)
    # a handle of a handle, back on the first context; then the last handle frees the arrays
    back = handle.attach(engine)
    handle.close()
    assert same(fetch(back.search(q_own)), own)
    engine.sync()
    held = free_bytes(0)
    back.close()
    assert free_bytes(0) - held > dev_bytes * 0.8, "the arrays go with their last handle"
    other.close()


def test_two_threads_search_two_handles_at_once(engine):
    tg, qs = case(seed=6, n_targets=30, tsize=40_000, nq=20_000)
    want = ref_search(*tg, *qs, 1, 0.0, 0.0)
    ix = engine.sets_from_arrays(*tg).index()
    other = S.Engine(0)
    handle = ix.attach(other)
    work = [(engine, ix, engine.sets_from_arrays(*qs)), (other, handle, other.sets_from_arrays(*qs))]
    results, errors = [[], []], []
    start = threading.Barrier(2)

    def run(i):
        try:
            eng, index, q = work[i]
            start.wait(30)
            hits = None
            for _ in range(20):
                hits = index.search(q, reuse=hits)
                results[i].append(fetch(hits))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not errors and not any(t.is_alive() for t in threads), errors
    assert len(results[0]) == len(results[1]) == 20
    for r in results[0] + results[1]:
        assert same(r, want)
    handle.close()
    ix.close()
    other.close()


def test_handle_on_a_second_device(engine):
    if n_devices() < 2:
        pytest.skip("one GPU visible: a handle on another device needs two")
    tg, qs = case(seed=8)
    want = ref_search(*tg, *qs, 1, 0.0, 0.0)
    ix = engine.sets_from_arrays(*tg).index()
    dev_bytes = ix.info()["device_bytes"]
    far = S.Engine(1)
    q_far = far.sets_from_arrays(*qs)
    far.sync()
    before = free_bytes(1)
    handle = ix.attach(far)
    copied = before - free_bytes(1)
    assert copied > dev_bytes * 0.8, ("a handle on another device holds a copy", copied, dev_bytes)
    assert handle.info() == ix.info()
    assert same(fetch(handle.search(q_far)), want)
    second = handle.attach(far)  # the same device as the copy: shared
    assert abs(before - copied - free_bytes(1)) < dev_bytes // 20
    ix.close()
    handle.close()
    assert same(fetch(second.search(q_far)), want)
    top = second.search(q_far).top(1)
    assert top.info()["n_queries"] == len(qs[0]) - 1
    second.close()
    far.close()
