"""The sketch sets' host-side reference and crafted reads (include/biosketch.h "sketch sets", bio_amd/csrc/sets.hip).

ref_sets is the header's rule in NumPy -- keep v <= MaxUint64 / scale, sort, de-duplicate -- over values that come from the CPU ORACLE,
never from the engine's own tuples; ref_sets_rows is the same for reads of one count, without a Python loop.  Every builder returns its
reads with what it claims about them (exact counts, the network width of every wave of four, the sorted ranks of duplicates, how many
values pass a scale); tests/test_sets_cases.py re-derives each claim with the oracle alone, and tests/test_gpu_sets_edges.py asserts
from the engine's own offsets that the device reached the edge before it compares the sets.  Nothing here imports the engine: kinds
are the strings "kmer", "nthash", "minimizer", "syncmer".  Searches are seeded; the seed that hit is part of the claim."""
import numpy as np

U64 = np.uint64
FULL = 2**64 - 1
SMALL_CAP = 64     # sets.hip: per-sequence sets take k_sets_rows iff the batch's largest count is <= SMALL_CAP
SCAN_CHUNK = 2048  # sets_internal.hpp: numbers per block of the library's scan (SCAN_PER_THREAD * SCAN_BLOCK)
SCAN_TRIP = 1024   # sets_internal.hpp: block sums k_scan_top takes per trip (its s_carry crosses trips)
LADDER = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
_ACGT = np.frombuffer(b"ACGT", np.uint8)


# ---- the reference ----
def maxhash(scale):
    return FULL // scale if scale > 1 else FULL


def collection(sets):
    offs = np.zeros(len(sets) + 1, U64)
    if sets:
        offs[1:] = np.cumsum([len(s) for s in sets])
    vals = np.concatenate(sets).astype(U64) if sets and offs[-1] else np.zeros(0, U64)
    return offs, vals


def ref_sets(values_per_read, scale, whole):
    """-> (offsets[n_sets + 1], values): per read (or for all reads together) the values <= MaxUint64 / scale, ascending, each once"""
    mh = U64(maxhash(scale))
    per = []
    for v in values_per_read:
        v = np.asarray(v, U64)
        per.append(np.unique(v[v <= mh]))
    if whole:
        per = [np.unique(np.concatenate(per)) if per else np.zeros(0, U64)]
    return collection(per)


def ref_sets_rows(v2d, scale, whole, present=None):
    """ref_sets for reads of one count: v2d[i] are read i's values (present[i] false: the read has none).  Sort along axis 1, keep the
    first of every run that passes."""
    v = np.sort(np.asarray(v2d, U64), axis=1)
    keep = v <= U64(maxhash(scale))
    keep[:, 1:] &= v[:, 1:] != v[:, :-1]
    if present is not None:
        keep &= np.asarray(present, bool)[:, None]
    if whole:
        vals = np.unique(v[keep])
        return np.array([0, len(vals)], U64), vals
    offs = np.zeros(len(v) + 1, U64)
    offs[1:] = np.cumsum(keep.sum(1))
    return offs, v[keep]


def oracle_values(oracle, kind, pk, q):
    """Next*() values of the reference iterator / sketch over one read, from the CPU oracle (none where its constructor fails)"""
    try:
        if kind == "minimizer":
            return oracle.minimizer(q, pk["k"], pk["w"], False, closed=True)[0]
        if kind == "syncmer":
            return oracle.syncmer(q, pk["k"], pk["s"], False, closed=True)[0]
        if kind == "nthash":
            return oracle.nthash(q, pk["k"], True)[0]
        return oracle.kmer_codes(q, pk["k"], pk.get("canonical", True), False)
    except oracle.OracleError:
        return np.zeros(0, U64)


def values_of(oracle, case):
    return [np.asarray(oracle_values(oracle, case["kind"], case["pk"], q), U64) for q in case["reads"]]


def wave_widths(counts):
    """the network k_sets_rows takes for every wave of four consecutive reads: 64, 32 or 16 values per row"""
    c = np.asarray(counts, np.int64)
    c = np.concatenate([c, np.zeros(-len(c) % 4, np.int64)]).reshape(-1, 4).max(1)
    return np.where(c > 32, 64, np.where(c > 16, 32, 16))


def rand_read(rng, n):
    return _ACGT[rng.integers(0, 4, n)].tobytes().decode()


# ---- the count ladder ----
def ladder_waves():
    """waves of four counts: every ladder count at every row beside three short rows (so that one long row alone widens the network of
    its three neighbours), four equal rows, one loaded row beside three empty ones, and mixes across 16 / 32 / 48"""
    waves = []
    for c in LADDER:
        for p in range(4):
            w = [1, 2, 0]
            w.insert(p, c)
            waves.append(w)
    waves += [[c] * 4 for c in LADDER]
    for c in (33, 64, 17):
        for p in range(4):
            w = [0, 0, 0]
            w.insert(p, c)
            waves.append(w)
    return waves + [[16, 17, 15, 16], [32, 33, 31, 32], [48, 49, 47, 64], [63, 64, 1, 17], [16, 16, 16, 15], [32, 16, 32, 31]]


LADDER_TAILS = {0: [], 1: [64], 2: [33, 17], 3: [16, 49, 2]}  # n % 4 reads of a loaded last wave


def ladder_case(oracle, k, tail, extra65=False, seed=71):
    """KMER reads (ACGT only: count = L - k + 1) of ladder_waves()'s counts + LADDER_TAILS[tail]; extra65: one read of 65 values at
    index 5, which alone moves the whole batch to the general path.  distinct[i]: read i's number of distinct values."""
    rng = np.random.default_rng([seed, k, tail])
    counts = [c for w in ladder_waves() for c in w] + LADDER_TAILS[tail]
    if extra65:
        counts.insert(5, SMALL_CAP + 1)
    reads = []
    for i, c in enumerate(counts):
        reads.append(rand_read(rng, c + k - 1) if c else (rand_read(rng, k - 1) if i % 2 else ""))
    case = dict(kind="kmer", pk=dict(k=k), reads=reads, counts=np.array(counts, np.int64), widths=wave_widths(counts))
    case["distinct"] = np.array([len(np.unique(v)) for v in values_of(oracle, case)], np.int64)
    return case


# ---- duplicates at register boundaries ----
DUP_K = 5


def dup_boundary_case(oracle, seed=73):
    """KMER k = 5 reads of at most 64 values: for b in 16, 32, 48 one whose sorted values have v[b-1] == v[b] ("at") and one with
    v[b-1] != v[b] == v[b+1] ("after"), found by a seeded search over reads with a periodic part; poly-A (one value, c copies) and
    period-2 reads of 17, 33, 49 and 64 values.  facts: one dict per read."""
    k = DUP_K
    reads, facts = [], []
    for b in (16, 32, 48):
        for how in ("at", "after"):
            for s in range(20000):
                rng = np.random.default_rng([seed, b, how == "at", s])
                c = int(rng.integers(b + 2, SMALL_CAP + 1))
                p = int(rng.integers(2, 24))
                m = int(rng.integers(k, c + k))
                q = (rand_read(rng, p) * (m // p + 1))[:m] + rand_read(rng, c + k - 1 - m)
                v = np.sort(oracle_values(oracle, "kmer", dict(k=k), q))
                if len(v) == c and (v[b - 1] == v[b] if how == "at" else v[b - 1] != v[b] == v[b + 1]):
                    reads.append(q)
                    facts.append(dict(b=b, how=how, count=c, seed=s))
                    break
            else:
                raise RuntimeError("no read with a duplicate %s rank %d" % (how, b))
    for c in (17, 33, 49, 64):
        reads.append("A" * (c + k - 1))
        facts.append(dict(how="poly", count=c, distinct=1))
        reads.append(("AC" * 40)[:c + k - 1])
        facts.append(dict(how="period2", count=c, distinct=2))
    return dict(kind="kmer", pk=dict(k=k), reads=reads, facts=facts, counts=np.array([f["count"] for f in facts], np.int64))


# ---- filter boundaries ----
FILTER_K = 21
FILTER_PAIRS = sorted({(c, b) for c in (48, 64) for b in (0, 1, 15, 16, 17, 32, 48, c)})


def _filter_read(rng, gen, c):
    n = c + FILTER_K - 1
    if gen == "random":
        return rand_read(rng, n)
    if gen == "doubled":  # k-mer i + c/2 repeats k-mer i: every value twice
        return (rand_read(rng, c // 2) * 3)[:n]
    return (rand_read(rng, int(rng.integers(1, 5))) * n)[:n]  # "periodic": at most four values


def straddles(v_sorted, b):
    """a duplicate just below the cut and another just above it: ranks b-2 == b-1 pass, ranks b == b+1 are dropped"""
    v = v_sorted
    return 2 <= b <= len(v) - 2 and v[b - 2] == v[b - 1] and v[b] == v[b + 1]


def filter_case(oracle, seed=79):
    """ntHash k = 21 reads of c = 48 or 64 values with a scale in 2 .. 64 at which exactly b of the c values (duplicates counted) pass,
    for every (c, b) of FILTER_PAIRS -> one dict per pair: read, scale, c, b, how the read was made, the seed that hit, and whether
    duplicates straddle the cut.  Even b < c are searched among reads that hold every value twice, b == c among periodic reads
    (all of a random read's 48 values below MaxUint64 / 2 is one seed in 2^48)."""
    scales = np.arange(2, 65)
    mh = np.array([maxhash(int(s)) for s in scales], U64)
    out = []
    for c, b in FILTER_PAIRS:
        gen = "periodic" if b == c else "doubled" if b in (16, 32, 48) else "random"
        for s in range(100000):
            rng = np.random.default_rng([seed, c, b, s])
            q = _filter_read(rng, gen, c)
            v = np.sort(oracle_values(oracle, "nthash", dict(k=FILTER_K), q))
            if len(v) != c:
                continue
            hit = np.flatnonzero((v[None, :] <= mh[:, None]).sum(1) == b)
            if len(hit):
                out.append(dict(read=q, scale=int(scales[hit[0]]), c=c, b=b, gen=gen, seed=s, straddle=bool(straddles(v, b))))
                break
        else:
            raise RuntimeError("no read of %d values of which %d pass" % (c, b))
    return out


# ---- exact thresholds ----
def decode32(x):
    """the 32-mer whose 2-bit code (A, C, G, T = 0 .. 3, first base in the top bits) is x"""
    return "".join("ACGT"[(x >> (62 - 2 * i)) & 3] for i in range(32))


THRESHOLD_SCALES = (3, 2**31 - 1, 7, 5, 10, 11, 13, 1000)


def threshold_case(oracle, n_scales=3):
    """KMER k = 32 canonical: for three scales (3 and 2^31 - 1 among them) the 32-mers that decode m - 1, m and m + 1,
    m = MaxUint64 // scale, where the oracle yields exactly those codes (a code above its reverse complement's is not reachable: such
    a scale is passed over) -> per scale: three short reads (one value each) and their concatenation, a 96-base read of 65 values"""
    out = []
    for scale in THRESHOLD_SCALES:
        m = FULL // scale
        short = [decode32(x) for x in (m - 1, m, m + 1)]
        if all(list(oracle_values(oracle, "kmer", dict(k=32), q)) == [x] for q, x in zip(short, (m - 1, m, m + 1))):
            out.append(dict(kind="kmer", pk=dict(k=32), scale=scale, m=m, short=short, long="".join(short)))
        if len(out) == n_scales:
            return out
    raise RuntimeError("fewer than %d scales whose threshold codes are canonical" % n_scales)


# ---- the sentinel ----
def sentinel_case():
    """KMER k = 32, both strands (canonical = False): T x 32 has the codes ~0 and 0, the value filtered elements are replaced by"""
    rng = np.random.default_rng(83)
    reads = ["T" * 32, "T" * 40, "A" * 40, "T" * 33 + "ACGGTCA" + "A" * 20, rand_read(rng, 50), "", "A" * 32, "T" * 31]
    return dict(kind="kmer", pk=dict(k=32, canonical=False), reads=reads, holds_full=[True, True, True, True, False, False, True, False])


# ---- result layouts ----
LAYOUTS = {  # lengths, the kernel the plan must name, BSK_* switches
    "ring": ((200, 250, 290), "k_minimizer_ring", {}),
    "pkd": ((300, 340, 400), "k_minimizer_pkd", {}),
    "pk": ((150,), "k_minimizer_pk", {}),
    "wide": (tuple(range(64, 121)), " (over tiles)", {"BSK_TILE_MIN": "64"}),
}


def layout_case(oracle, name, seed=89):
    """minimizer batches of one length class, every read redrawn until it holds at most 64 values, with reads whose poly-A tail ties
    the window's keys (the packed kernels list them for the exact machine: stride 1 inside a unit of rows), reads too short for one
    window, empty reads, and n no multiple of 64 -- the construction of test_group_gather_layouts_and_mixed_groups"""
    lens, plan, env = LAYOUTS[name]
    pk = dict(k=15, w=8) if name == "wide" else dict(k=21, w=11)
    rng = np.random.default_rng([seed, len(name), lens[0]])
    n = 64 * 3 + 29 if name == "wide" else 64 * 37 + 29
    tail = "A" * (pk["k"] + pk["w"] + 4)

    def draw(i):
        while True:
            ln = int(rng.choice(lens))
            q = rand_read(rng, ln - len(tail)) + tail if i % 97 == 5 else rand_read(rng, ln)
            if len(oracle_values(oracle, "minimizer", pk, q)) <= SMALL_CAP:
                return q

    reads = [draw(i) for i in range(n)]
    for i in range(11, n, 131):
        reads[i] = reads[i][:17 if name != "wide" else 13]  # too short: no window
    reads[64], reads[65], reads[127] = "", "ACGT", ""
    if name == "pk":
        reads[199] = reads[263] = "A" * 80  # a homopolymer: 50 windows, one value
    return dict(kind="minimizer", pk=pk, reads=reads, plan=plan, env=env, tailed=list(range(5, n, 97)))


# ---- scan trips ----
def scan_reads_case(oracle, n=2 * SCAN_TRIP * SCAN_CHUNK + SCAN_CHUNK + 1, length=24, k=21, seed=97):
    """(a) n reads of `length` bases, read i = bases [i * step, i * step + length) of one random sequence (step = its number of k-mers),
    so that ONE oracle call over that sequence yields every read's ntHash values: v2d[i] = H[i * step : (i + 1) * step].  Reads at the
    scan's block and trip boundaries are empty.  -> data, offsets (for batch_from_arrays), v2d, present"""
    rng = np.random.default_rng(seed)
    step = length - k + 1
    s = _ACGT[rng.integers(0, 4, n * step + k - 1)]
    h = np.asarray(oracle.nthash(s, k, True)[0], U64)
    assert len(h) == n * step
    present = np.ones(n, bool)
    trip = SCAN_TRIP * SCAN_CHUNK
    empty = [0, 1, SCAN_CHUNK - 1, SCAN_CHUNK, trip - 1, trip, trip + 1, 2 * trip - 1, 2 * trip, 2 * trip + SCAN_CHUNK - 1]
    present[[e for e in empty if e < n]] = False
    windows = np.lib.stride_tricks.sliding_window_view(s, length)[::step][:n]
    data = np.ascontiguousarray(windows[present]).reshape(-1)
    offs = np.zeros(n + 1, U64)
    offs[1:] = np.cumsum(np.where(present, length, 0))
    return dict(kind="nthash", pk=dict(k=k), data=data, offsets=offs, v2d=h.reshape(n, step), present=present, n=n, step=step)


def scan_read(case, i):
    """read i of scan_reads_case as a string"""
    a, b = int(case["offsets"][i]), int(case["offsets"][i + 1])
    return case["data"][a:b].tobytes().decode()


def scan_values_case(n=16500, length=150, k=21, seed=101):
    """(b) n random reads of 150 bases: 130 ntHash values each, more than SCAN_TRIP * SCAN_CHUNK in total, every count above 64"""
    rng = np.random.default_rng(seed)
    data = _ACGT[rng.integers(0, 4, n * length)]
    offs = (np.arange(n + 1, dtype=U64) * U64(length))
    return dict(kind="nthash", pk=dict(k=k), data=data, offsets=offs, n=n, length=length, count=length - k + 1)


def scan_values_v2d(oracle, case):
    d, ln, k = case["data"], case["length"], case["pk"]["k"]
    return np.stack([np.asarray(oracle.nthash(d[i * ln:(i + 1) * ln], k, True)[0], U64) for i in range(case["n"])])
