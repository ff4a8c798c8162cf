"""The stream kernels at their word boundaries and length limits, every call with the kernel it must run on asserted by name.

k_nthash_fast<0|1|2> (ntHash forward / canonical, canonical k-mer codes) get the length list test_two_strand_kmer_codes_on_the_stream_kernel
uses for mode 3 -- 1, 2, k-1, k, k+1, and both sides of every packed-word and LDS-row boundary up to the kernel's 512 bases -- in ragged and
fixed-length batches, at k on both sides of 16 / 32 / 64 (one, two, four words of a k-mer); circular calls on both sides of the limit.

k_simhash_fast keeps its 64 counters as 5 (nh = k - m + 1 <= 31) or 6 (<= 63) bit planes.  A counter reaches nh only when every m-mer of
a k-mer has that bit set -- a homopolymer or a short repeat, never random bases (2^-31) -- so nh = 31 and 63, where every plane of a full
counter is 1 and the threshold compare's borrow chain is longest, run here on `A...`, `AC...`, `ACG...` repeats, with scale 1 and nh,
canonical and forward, plain and circular, at each of the three LDS sizes' limits (160 / 288 / 512 bases) and one base beyond.

Circular calls: the engine appends the first k - 1 bases (make_circular), and the planner then keeps another k bases of room, so a
circular read of `len` bases takes the place of len + 2k - 1 (k > 1).  Beyond the stream kernels' 512 bases a plain batch runs as tiles on
the same kernel; a circular batch whose extended reads still fit 512 bases runs on the general kernel (k_nthash_stream<0>, k_kmer<0>,
k_simhash<0>).
"""
import random

import numpy as np
import pytest

from bio_amd import _lib as L
from tests import plan_atlas as A

pytestmark = pytest.mark.gpu

LIMIT = A.STREAM_BASES


def planned_len(n, k, circular):
    """the length the planner compares with a stream kernel's limit"""
    return n + ((k - 1 if k > 1 else 0) + k if circular else 0)


def check_stream(engine, oracle, seqs, kind, ref, plan, **par):
    b = engine.batch(seqs)
    res = engine.run(b, engine.params(kind, **par))
    assert res.plan()["kernel"] == plan, (res.plan(), plan, par, max(map(len, seqs)))
    n_tuples = 0
    for i, q in enumerate(seqs):
        st, h, _ = res.read(i)
        try:
            e = ref(q)
        except oracle.OracleError as err:
            assert err.name == "ErrShortSeq" and (st & L.ST_CODE_MASK) == L.ST_SHORT and len(h) == 0, (par, i, len(q), err.name, st)
            continue
        assert (st & L.ST_CODE_MASK) == L.ST_OK and np.array_equal(h, e), (par, i, len(q), len(h), len(e))
        n_tuples += len(h)
    assert res.digest()["n_tuples"] == n_tuples, par
    res.close()
    b.close()


def boundary_lengths(k):
    return sorted({n for n in (1, 2, k - 1, k, k + 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512) if 1 <= n <= LIMIT})


# (mode of k_nthash_fast, kind, canonical, the general kernel of the kind, the values of k)
MODES = [(0, L.NTHASH, False, "k_nthash_stream<0>", (1, 16, 17, 31, 32, 33, 63, 64, 65, 100)),
         (1, L.NTHASH, True, "k_nthash_stream<0>", (1, 16, 17, 31, 32, 33, 63, 64, 65, 100)),
         (2, L.KMER, True, "k_kmer<0>", (1, 16, 17, 31, 32))]


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_stream_kernel_word_boundaries(engine, oracle, mode):
    _, kind, canonical, general, ks = MODES[mode]
    fast = "k_nthash_fast<%d>" % mode
    for k in ks:
        rng = random.Random(5120 + 10 * k + mode)

        def ref(q, circular=False):
            if kind == L.NTHASH:
                return oracle.nthash(q, k, canonical, circular)[0]
            return oracle.kmer_codes(q, k, canonical, circular)

        ragged = [A.fast_seq(rng, n) for n in boundary_lengths(k)] + [A.fast_seq(rng, rng.randint(1, LIMIT)) for _ in range(120)] + ["", "A" * LIMIT, "AC" * (LIMIT // 2)]
        fixed = [A.fast_seq(rng, 150) for _ in range(300)]
        for seqs in (ragged, fixed):
            check_stream(engine, oracle, seqs, kind, ref, fast, k=k, canonical=canonical)
        # one base beyond the kernel's limit: tiles, on the same kernel
        check_stream(engine, oracle, ragged + [A.fast_seq(rng, LIMIT + 1)], kind, ref, fast + A.TILES, k=k, canonical=canonical)
        # circular: the longest read the kernel takes, and one base more -- the general kernel while the extended read fits 512 bases
        top = LIMIT - planned_len(0, k, True)
        for n, plan in ((top, fast), (top + 1, general)):
            seqs = [A.fast_seq(rng, m) for m in (1, 2, k - 1, k, k + 1, n - 1, n) if m >= 1] + [A.fast_seq(rng, rng.randint(1, n)) for _ in range(80)] + ["A" * n]
            check_stream(engine, oracle, seqs, kind, lambda q: ref(q, True), plan, k=k, canonical=canonical, circular=True)


# nh = 1, 31 (five planes, all set), 32 (six planes: 100000), 63 (six planes, all set), 64 (scalar counters: k_simhash<0>)
SIM = [(1, 21, 21), (31, 35, 5), (32, 36, 5), (63, 67, 5), (64, 68, 5)]


def simhash_plan(nh, n, k, circular):
    """the plan of a batch whose longest read has n bases"""
    ext = planned_len(n, k, circular)
    in_batch = n + (k - 1 if circular and k > 1 else 0)  # what the (extended) batch holds: tiles from 513 bases
    if in_batch > LIMIT:
        return None  # tiles: the tile batch's plan + " (over tiles)"
    if nh > 63 or ext > LIMIT:
        return "k_simhash<0>"
    words = next(w for w in sorted(A.SIM_BASES) if ext <= A.SIM_BASES[w])
    return "k_simhash_fast<%d,%d>" % (5 if nh <= 31 else 6, words)


@pytest.mark.parametrize("nh,k,m", SIM)
@pytest.mark.parametrize("circular", [False, True])
def test_simhash_full_counters_at_every_lds_size(engine, oracle, nh, k, m, circular):
    rng = random.Random(100 * nh + circular)
    seen, sizes = set(), set()
    for scale in sorted({1, nh}):
        for canonical in (True, False):
            for lim in (160, 288, 512):
                for n in (lim - planned_len(0, k, circular), lim - planned_len(0, k, circular) + 1):
                    if n < 1 or (circular and n < k):  # (a circular read shorter than k is refused and not extended: nothing to hold against the limit)
                        continue
                    sizes.add(next(w for w in sorted(A.SIM_BASES) if lim <= A.SIM_BASES[w]))
                    seqs = ["A" * n, ("AC" * n)[:n], ("ACG" * n)[:n], ("AC" * n)[:n - 1], "G" * (n // 2), ""]
                    seqs += [A.fast_seq(rng, n) for _ in range(10)] + [A.fast_seq(rng, rng.randint(1, n)) for _ in range(50)] + [A.fast_seq(rng, m_) for m_ in (k - 1, k, k + 1) if 1 <= m_ <= n]
                    plan = simhash_plan(nh, n, k, circular)
                    b = engine.batch(seqs)
                    res = engine.run(b, engine.params(L.SIMHASH, k, m=m, scale=scale, canonical=canonical, circular=circular))
                    got = res.plan()["kernel"]
                    if plan is None:
                        assert got.endswith(A.TILES) and got.startswith("k_simhash<0>" if nh > 63 else "k_simhash_fast<%d," % (5 if nh <= 31 else 6)), (res.plan(), n, k, circular)
                    else:
                        assert got == plan, (res.plan(), plan, n, k, circular)
                    seen.add(got)
                    for i, q in enumerate(seqs):
                        st, h, _ = res.read(i)
                        try:
                            e = oracle.simhash(q, k, m, scale, canonical, circular)
                        except oracle.OracleError as err:
                            assert err.name == "ErrShortSeq" and (st & L.ST_CODE_MASK) == L.ST_SHORT and len(h) == 0, (nh, scale, canonical, circular, n, i, len(q), err.name, st)
                            continue
                        assert (st & L.ST_CODE_MASK) == L.ST_OK and np.array_equal(h, e), (nh, scale, canonical, circular, n, i, len(q), got)
                    res.close()
                    b.close()
    if nh <= 63:  # every LDS size of the row's plane count ran (circular calls at k = 67 begin at 3k - 1 = 200 planned bases: no 160-base size there)
        assert sizes >= ({20, 34} if circular else {12, 20, 34}) and {"k_simhash_fast<%d,%d>" % (5 if nh <= 31 else 6, w) for w in sizes} <= seen, (sizes, seen)
    else:
        assert "k_simhash<0>" in seen, seen
