"""One row per kernel instantiation of the default build (the build without EXPERIMENTS=1): the parameters, the BSK_* switches and the seeded
reads that make the planner choose it, and the kernel name `bsk_result_plan` must then report -- shared by tests/test_plan_atlas.py (CPU:
rows + UNREACHABLE equal the set the headers compile, and every row's reads have teeth) and tests/test_gpu_plan_atlas.py (GPU: the plan
name, then every read against the oracle).

A row COVERS the instantiations in `covers`.  The expected name is exact up to template arguments the table cannot know: a name that
ends in a comma ("k_minimizer_fast<15,") is a prefix, BSK_FAST_CAP follows it.  `suffixes` must follow the name, the other known suffixes
must not.  Names are spelled as `plan_name` (planner.hip) spells them, without blanks.

What the plan string cannot name:
  * the ASCII side launches k_minimizer_dense<W,false,true> and k_syncmer_fast<W,false,true>: the string only says " + ASCII side launch".
    The rows `min_side` / `syn_side` run a batch where a third of the reads carry N or IUPAC letters with every W; every read must equal
    the oracle and the digest must equal the run with BSK_NO_SIDE_DENSE (the general ASCII kernel in the side launch).  The NAME of the side
    kernel is not observable;
  * the list passes of the packed kernels (k_minimizer_dense<W,true>, k_syncmer_fast<W,true>): they run behind the planned kernel over the
    reads it listed for the exact machine -- every row below has such reads (a homopolymer, low-complexity reads) -- and are not part of
    the compiled set this table is held against.

Reads of a row (Row.reads): plain random reads of the row's lengths, every tenth a low-complexity read, read 1 a homopolymer, read 2 one
base shorter than the constructor accepts, read 3 empty, then one read of every length in `limits` -- the instantiation's own length limit
where the row reaches it (the longest read decides the plan; where one base more changes the plan, a row of its own with the other name
follows).  `mixed` rows put N / IUPAC letters into every third read.  Everything is seeded: both test modules build the same reads.

FALLBACK ROWS.  `min_dense_fallback<W>` and `pm_fallback<5,9>` hold a homopolymer as long as the longest read: it outgrows its per-read
slab, the call abandons k_minimizer_dense / k_prot_minimizer_fast and ends on k_minimizer_fast<W> / k_prot_minimizer, and launch.hip names
that final plan.  The other fallback -- a batch with more than a quarter of low-complexity reads abandons k_minimizer_pk / _ring / _pkd /
k_syncmer_pk / _pf and ends on k_minimizer_fast<W <= 13> / k_syncmer_fast<W> -- is tested in tests/test_gpu_unit_trips.py (the full segment:
tests/unit_trips.py, EDGES).  The list of reads a packed kernel leaves to the exact machine
is cut into one segment per workgroup of AT LEAST 1 024 reads (syn_pk_fixcap, planner.hip; list_append, kernels_generic.hpp), and the
call only falls back when a segment is full: one workgroup must list more than 1 024 reads, which a batch of a few hundred reads -- at
most 64 per workgroup -- cannot do whatever it holds; there BSK_UNIT_GRID=1 gives one workgroup 1 024 and 1 025 exact-tie reads.  The instantiations such a call ends on are rows of their own here, planned with
BSK_NO_RING + BSK_NO_DENSE + BSK_NO_PK (minimizers) and BSK_NO_PK (syncmers), and their reads hold the low-complexity share above.
"""
from __future__ import annotations

import random

AA = "ACDEFGHIKLMNPQRSTVWY"
IUPAC = "NRYKMSWn"
SUFFIXES = (" (length-binned units)", " + ASCII side launch", " (over tiles)")
BINNED, SIDE, TILES = SUFFIXES

# the limits the rows are sized by (tests/test_plan_atlas.py holds them against the headers)
PK_SHORT_BASES = 240        # pk_minimizer_short_bases(): 16 (PKNW - 1)
RING_SHORT_BASES = 176      # ring_minimizer_short_bases(): 16 (4 BSK_RING_NQ - 1)
SYN_SHORT_BASES = 224       # pk_syncmer_max_bases(false) = pf_syncmer_max_bases(false): 16 (PKNW - 2)
SYN_LONG_BASES = 480        # ... (true): 16 (32 - 2)
STREAM_BASES = 512          # 16 (BSK_NT_FAST_WORDS - 2)
SIM_BASES = {12: 160, 20: 288, 34: 512}  # k_simhash_fast<P, words>: 16 (words - 2)

# instantiations no switch combination plans: {name: one-line reason from the planner source}
UNREACHABLE = {}


def rand_seq(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def low_complexity(rng, n):
    """repeats and homopolymer runs: equal hashes inside a window, the case where an unstable buffer order could show"""
    unit = rand_seq(rng, rng.randint(1, 6))
    s = (unit * (n // len(unit) + 1))[:n]
    cut = rng.randint(0, n)
    return s[:cut] + rand_seq(rng, n - cut)


def fast_seq(rng, n, alpha="ACGT"):
    """plain random letters, a byte of the generator per letter (rand_seq costs a call per letter)"""
    if n <= 0:
        return ""
    m = len(alpha)
    return "".join(alpha[b % m] for b in rng.randbytes(n)) if m != 4 else bytes(alpha.encode()[b & 3] for b in rng.randbytes(n)).decode()


def hash_seed(*parts):
    v = 1469598103934665603
    for p in parts:
        for ch in str(p):
            v = ((v ^ ord(ch)) * 1099511628211) & ((1 << 64) - 1)
    return v


class Row:
    """kind: minimizer | syncmer | nthash | kmer | simhash | prot_hash | prot_minimizer; alphabet: dna | protein; p: the parameters
    (k, w, s, m, scale, canonical, circular, codon_table, frame); env: the BSK_* switches; name + suffixes: what the plan must say;
    covers: the instantiations the row stands for; lens: lengths of the plain reads; limits: lengths that must be present (the longest
    read of the batch is max(lens + limits)); mixed: every third read carries N / IUPAC letters; digest_env: switches of a second run
    whose digest must equal the first's; extra: reads appended as they are; lc_max: the longest homopolymer / low-complexity read (kernels
    with one slab per read -- k_minimizer_dense, k_prot_minimizer_fast -- are ABANDONED when a read selects more than its slab holds: their
    rows keep such reads within the slab, and the `fallback` rows do not)"""

    def __init__(self, rid, kind, p, name, covers, lens, limits=(), env=None, suffixes=(), alphabet="dna", mixed=False, digest_env=None, n=160,
                 extra=(), lc_max=None):
        self.lc_max = lc_max
        self.id, self.kind, self.p, self.name, self.covers = rid, kind, dict(p), name, tuple(covers)
        self.lens, self.limits, self.env, self.suffixes = tuple(lens), tuple(limits), dict(env or {}), tuple(suffixes)
        self.alphabet, self.mixed, self.digest_env, self.n, self.extra = alphabet, mixed, digest_env, n, tuple(extra)

    def __repr__(self):
        return "Row(%s)" % self.id

    @property
    def circular(self):
        return bool(self.p.get("circular"))

    def min_len(self):
        """the shortest sequence the reference's constructor accepts (non-circular calls)"""
        k, p = self.p["k"], self.p
        if self.kind == "minimizer":
            return k + p["w"] - 1                      # sketch.go:92
        if self.kind == "syncmer":
            return k if p["s"] == k else 2 * k - p["s"] - 1  # sketch.go:149
        if self.kind == "prot_hash":
            return 3 * k                               # iterator-protein.go:50: checked on the INPUT length, protein input too
        if self.kind == "prot_minimizer":
            return 3 * k + p["w"] - 1                  # sketch-protein.go:66,73
        return k

    def plain_indices(self):
        """reads that are plain random reads of the row's lengths (neither crafted nor low-complexity nor mixed)"""
        first = 4 + len(self.limits)
        return [i for i in range(first, self.n) if i % 10 and not (self.mixed and i % 3 == 2)]

    def limit_indices(self):
        return list(range(4, 4 + len(self.limits)))

    def reads(self):
        rng = random.Random(hash_seed("atlas", self.id))
        alpha = AA if self.alphabet == "protein" else "ACGT"
        seqs = [fast_seq(rng, rng.choice(self.lens), alpha) for _ in range(self.n)]
        for j in range(0, self.n, 10):  # every tenth read is low-complexity
            q = low_complexity(rng, min(len(seqs[j]), self.lc_max) if self.lc_max else len(seqs[j]))
            seqs[j] = q.replace("T", "W") if self.alphabet == "protein" else q
        seqs[1] = "A" * (min(max(self.lens + self.limits), self.lc_max) if self.lc_max else max(self.lens + self.limits))
        seqs[2] = fast_seq(rng, max(self.min_len() - 1, 0), alpha)
        seqs[3] = ""
        for j, ln in enumerate(self.limits):
            seqs[4 + j] = fast_seq(rng, ln, alpha)
        if self.mixed:  # about a third of the reads: one to three N / IUPAC letters each
            for j in range(2, self.n, 3):
                q = list(seqs[j])
                for _ in range(rng.randint(1, 3)):
                    if q:
                        q[rng.randrange(len(q))] = rng.choice(IUPAC)
                seqs[j] = "".join(q)
        return seqs + list(self.extra)


# ---- minimizers -------------------------------------------------------------------------------------------------------------------
MIN_K = 21
NO_RING, NO_DENSE, NO_PK, NO_PKD = {"BSK_NO_RING": "1"}, {"BSK_NO_DENSE": "1"}, {"BSK_NO_PK": "1"}, {"BSK_NO_PKD": "1"}
GENERIC = {"BSK_FORCE_GENERIC": "1"}
BIN = {"BSK_BIN_MIN": "64"}
NO_SIDE_DENSE = {"BSK_NO_SIDE_DENSE": "1"}


def _env(*ds):
    out = {}
    for d in ds:
        out.update(d)
    return out


def fast_tile_min(k, w):
    """tile_min_for (tiles.hip): windows only k_minimizer_fast takes (w >= 17) tile from 11 (w + 1) + k + w bases"""
    return 11 * (w + 1) + k + w


def slab_tuples(nwin, w):
    """tuples of a per-read slab (make_plan_enc: 2.6 / (w + 1) of the longest read's windows + 16, at most a tuple per window; before rounding
    up to whole 128-byte lines)"""
    return min(nwin, int(nwin * 2.6 / (w + 1.0)) + 16)


def _minimizer_rows():
    rows = []
    mp = lambda w, **kw: dict(k=MIN_K, w=w, **kw)
    for w in range(2, 14):
        pk_env = _env(NO_RING, NO_DENSE)  # (KT.MIN_CELLS "pk": barred from the unit-row and the per-read-slab kernels)
        rows.append(Row("min_pk<%d,false>" % w, "minimizer", mp(w), "k_minimizer_pk<%d,false>" % w, ["k_minimizer_pk<%d,false>" % w],
                        (100, 150, 200), (PK_SHORT_BASES - 1, PK_SHORT_BASES), pk_env))
        rows.append(Row("min_pk<%d,true>" % w, "minimizer", mp(w), "k_minimizer_pk<%d,true>" % w, ["k_minimizer_pk<%d,true>" % w],
                        (150, 200, 260), (PK_SHORT_BASES, PK_SHORT_BASES + 1), pk_env))
        ring_env = {"BSK_RING": "1"}
        rows.append(Row("min_ring<%d,false>" % w, "minimizer", mp(w), "k_minimizer_ring<%d,false>" % w, ["k_minimizer_ring<%d,false>" % w],
                        (100, 150, 170), (RING_SHORT_BASES - 1, RING_SHORT_BASES), ring_env))
        rows.append(Row("min_ring<%d,true>" % w, "minimizer", mp(w), "k_minimizer_ring<%d,true>" % w, ["k_minimizer_ring<%d,true>" % w],
                        (150, 200, 260), (RING_SHORT_BASES, RING_SHORT_BASES + 1), ring_env))
        rows.append(Row("min_pkd<%d>" % w, "minimizer", mp(w), "k_minimizer_pkd<%d>" % w, ["k_minimizer_pkd<%d>" % w], (300, 400, 450), (), NO_RING))
    for w in range(1, 17):
        env = _env(NO_RING, NO_PKD)
        lc = MIN_K + w - 2 + slab_tuples(400 - MIN_K - w + 2, w)  # a homopolymer selects every window: this one fills its slab to the last tuple
        rows.append(Row("min_dense<%d>" % w, "minimizer", mp(w), "k_minimizer_dense<%d>" % w, ["k_minimizer_dense<%d>" % w], (300, 400), (400,), env, lc_max=lc))
        rows.append(Row("min_side<%d>" % w, "minimizer", mp(w), "k_minimizer_dense<%d>" % w, ["k_minimizer_dense<%d,false,true>" % w], (300, 400), (400,), env,
                        suffixes=(SIDE,), mixed=True, digest_env=NO_SIDE_DENSE, lc_max=lc))
        if w >= 3:  # fallback, as production reaches it: a homopolymer of full length outgrows its slab, the call abandons k_minimizer_dense and re-plans
            rows.append(Row("min_dense_fallback<%d>" % w, "minimizer", mp(w), "k_minimizer_fast<%d," % w, [], (300, 400), (400,), env))
    for w in range(2, 33):
        env = _env(NO_RING, NO_DENSE, NO_PK)  # (w <= 13: what a call that abandons a packed kernel re-plans to)
        if w >= 17:  # beyond tile_min the batch is cut into tiles: the same instantiation over tiles
            tm = fast_tile_min(MIN_K, w)
            rows.append(Row("min_fast<%d>" % w, "minimizer", mp(w), "k_minimizer_fast<%d," % w, ["k_minimizer_fast<%d>" % w], (100, 150, 200), (tm - 1, tm), env))
            rows.append(Row("min_fast_tiles<%d>" % w, "minimizer", mp(w), "k_minimizer_fast<%d," % w, [], (150, 200, 2 * tm), (tm, tm + 1), env,
                            suffixes=(TILES,)))
        else:
            rows.append(Row("min_fast<%d>" % w, "minimizer", mp(w), "k_minimizer_fast<%d," % w, ["k_minimizer_fast<%d>" % w], (100, 150, 200), (), env))
    for w in range(4, 14):
        rows.append(Row("min_pft<%d>" % w, "minimizer", mp(w), "k_minimizer_pft<%d>" % w, ["k_minimizer_pft<%d>" % w], (300, 306, 312), (),
                        {"BSK_TILE_MIN": "40", "BSK_TILE_DENSE": "1"}, suffixes=(TILES,), n=96))
    # circular calls: the engine appends the first k - 1 bases, and the extended read is what the limits are held against
    pk_env, ext = _env(NO_RING, NO_DENSE), MIN_K - 1
    rows.append(Row("min_pk<11,false>_circular", "minimizer", mp(11, circular=True), "k_minimizer_pk<11,false>", [], (100, 150, 200), (PK_SHORT_BASES - ext - 1, PK_SHORT_BASES - ext), pk_env))
    rows.append(Row("min_pk<11,true>_circular", "minimizer", mp(11, circular=True), "k_minimizer_pk<11,true>", [], (100, 150, 200), (PK_SHORT_BASES - ext, PK_SHORT_BASES - ext + 1), pk_env))
    rows.append(Row("min_ring<11,false>_circular", "minimizer", mp(11, circular=True), "k_minimizer_ring<11,false>", [], (100, 130, 150), (RING_SHORT_BASES - ext - 1, RING_SHORT_BASES - ext),
                    {"BSK_RING": "1"}))
    rows.append(Row("min_ring<11,true>_circular", "minimizer", mp(11, circular=True), "k_minimizer_ring<11,true>", [], (100, 130, 150), (RING_SHORT_BASES - ext, RING_SHORT_BASES - ext + 1),
                    {"BSK_RING": "1"}))
    # ragged batches on the lock-step kernels run as length-binned units from 1 024 reads on: BSK_BIN_MIN bins these small ones too
    rows.append(Row("min_pk<11,false>_binned", "minimizer", mp(11), "k_minimizer_pk<11,false>", [], (60, 100, 150, 200), (PK_SHORT_BASES,), _env(pk_env, BIN), suffixes=(BINNED,)))
    rows.append(Row("min_ring<11,true>_binned", "minimizer", mp(11), "k_minimizer_ring<11,true>", [], (60, 150, 200, 260), (), _env({"BSK_RING": "1"}, BIN), suffixes=(BINNED,)))
    rows.append(Row("min_pkd<11>_binned", "minimizer", mp(11), "k_minimizer_pkd<11>", [], (100, 200, 300, 450), (), _env(NO_RING, BIN), suffixes=(BINNED,)))
    rows.append(Row("min_dense<5>_binned", "minimizer", mp(5), "k_minimizer_dense<5>", [], (100, 200, 300), (400,), _env(NO_RING, NO_PKD, BIN), suffixes=(BINNED,),
                    lc_max=MIN_K + 5 - 2 + slab_tuples(400 - MIN_K - 5 + 2, 5)))
    rows.append(Row("min_generic<0>", "minimizer", mp(11), "k_minimizer_generic<0>", ["k_minimizer_generic<0>"], (150, 300), (), GENERIC))
    rows.append(Row("min_generic<0>_w40", "minimizer", mp(40), "k_minimizer_generic<0>", [], (150, 300), ()))
    rows.append(Row("min_generic<1>", "minimizer", mp(40), "k_minimizer_generic<1>", ["k_minimizer_generic<1>"], (150, 300), (), mixed=True))
    rows.append(Row("min_generic<1>_forced", "minimizer", mp(11), "k_minimizer_generic<1>", [], (150, 300), (), GENERIC, mixed=True))
    return rows


# ---- syncmers (W = k - s) ---------------------------------------------------------------------------------------------------------
NO_SYN_PF = {"BSK_NO_SYN_PF": "1"}
SYN_S = 11
SYN_TILE_MIN = 448                         # PlannerTable::syn_tile_min_bases: longer reads run as tiles whatever the plan
SYN_PAIR_ROWS = {False: 23, True: 58}      # pk_syncmer_pair_rows
SYN_PF_MASK_ROWS = {False: 20, True: 32}   # pf_syncmer_mask_rows
SYN_PF_TUPLES = {False: 1024, True: 1792}  # pf_syncmer_unit_tuples


def syn_nwin(k, s, ln):
    return ln - 2 * k + s + 2


def syn_pk_fits(k, s, ln, lng):
    """make_plan_enc's rule for k_syncmer_pk / _pkl, restated to size the rows' reads: rows of a pair's staging column"""
    w = k - s
    rows = 2.0 * (syn_nwin(k, s, ln) * 1.5 / (w + 1.0) + 0.5) + 2.0
    want = rows + 0.12 * (rows - 2.0) if lng else rows
    return 4 <= w <= (24 if lng else 20) and ln <= (SYN_LONG_BASES if lng else SYN_SHORT_BASES) and want <= SYN_PAIR_ROWS[lng]


def syn_pf_fits(k, s, ln, lng, density=0):
    """... for k_syncmer_pf / _pfl: mask rows and expected selections per read against the emit list"""
    w = k - s
    dens = max(syn_nwin(k, s, ln), 0) * 1.5 / (w + 1.0)
    dmax = density if density else SYN_PF_TUPLES[lng] / 64.0 * 0.86
    ns = ln - s + 1 if ln >= s else 0
    return 8 <= w <= (24 if lng else 20) and ln <= (SYN_LONG_BASES if lng else SYN_SHORT_BASES) and k <= 64 and (ns + w - 1) // w <= SYN_PF_MASK_ROWS[lng] + 1 and dens <= dmax


def _longest(fits, lo, hi):
    """the longest length in [lo, hi] the rule takes (the rules are monotone in the length)"""
    best = None
    for ln in range(lo, hi + 1):
        if fits(ln):
            best = ln
    return best


def _syncmer_rows():
    rows = []
    sp = lambda k, s, **kw: dict(k=k, s=s, **kw)
    for w in range(4, 25):
        s, k = SYN_S, SYN_S + w
        base = s + 7 * w + 4  # (KT.build_syncmer_reads: windows enough for the fused and the staged kernels)
        lens = (base, base + w // 2, base + w - 1)
        if w <= 20:
            top = _longest(lambda ln: syn_pk_fits(k, s, ln, False), base, SYN_SHORT_BASES)
            rows.append(Row("syn_pk<%d>" % w, "syncmer", sp(k, s), "k_syncmer_pk<%d>" % w, ["k_syncmer_pk<%d>" % w], lens, (top - 1, top), NO_SYN_PF))
            # the kernel's own limit of 224 bases: a k large enough that such a read's pair still fits the 23-row column
            s2 = next(x for x in range(9, 400) if syn_pk_fits(x + w, x, SYN_SHORT_BASES, False))
            rows.append(Row("syn_pk_224<%d>" % w, "syncmer", sp(s2 + w, s2), "k_syncmer_pk<%d>" % w, [], (200, 210, 220), (SYN_SHORT_BASES - 1, SYN_SHORT_BASES), NO_SYN_PF))
            rows.append(Row("syn_pk_225<%d>" % w, "syncmer", sp(s2 + w, s2), "k_syncmer_pkl<%d>" % w, [], (200, 210, 220), (SYN_SHORT_BASES, SYN_SHORT_BASES + 1), NO_SYN_PF))
            # the long plan by density: more rows than the short column's 23, fewer than the long one's 58
            lo = _longest(lambda ln: syn_pk_fits(k, s, ln, False), base, SYN_SHORT_BASES) + 1
            hi = _longest(lambda ln: syn_pk_fits(k, s, ln, True), lo, SYN_LONG_BASES)
            rows.append(Row("syn_pkl<%d>" % w, "syncmer", sp(k, s), "k_syncmer_pkl<%d>" % w, ["k_syncmer_pkl<%d>" % w], (lo + 8, (lo + hi) // 2, hi - 4), (lo, hi), NO_SYN_PF))
        else:
            hi = _longest(lambda ln: syn_pk_fits(k, s, ln, True), base, SYN_TILE_MIN)
            rows.append(Row("syn_pkl<%d>" % w, "syncmer", sp(k, s), "k_syncmer_pkl<%d>" % w, ["k_syncmer_pkl<%d>" % w], lens, (hi - 1, hi), NO_SYN_PF))
        s3 = next(x for x in range(9, 900) if syn_pk_fits(x + w, x, SYN_LONG_BASES, True))
        rows.append(Row("syn_pkl_480<%d>" % w, "syncmer", sp(s3 + w, s3), "k_syncmer_pkl<%d>" % w, [], (440, 460, 470), (SYN_LONG_BASES - 1, SYN_LONG_BASES),
                        _env(NO_SYN_PF, {"BSK_NO_TILES": "1"})))  # (beyond 448 bases a batch is cut into tiles: the switch keeps it whole)
    for w in range(8, 25):
        s, k = SYN_S, SYN_S + w
        base = s + 7 * w + 4
        lens = (base, base + w // 2, base + w - 1)
        if w <= 20:
            top = _longest(lambda ln: syn_pf_fits(k, s, ln, False), base, SYN_SHORT_BASES)
            rows.append(Row("syn_pf<%d>" % w, "syncmer", sp(k, s), "k_syncmer_pf<%d>" % w, ["k_syncmer_pf<%d>" % w], lens, (top - 1, top)))
            # k_syncmer_pfl: reads beyond 224 bases whose expected selections still fit the emit list -- k = 64, the largest the emit hashes
            # (w = 8: even then 225-base reads expect 25.8 selections against 24.1, so BSK_PF_DENSITY plans it, as
            # test_syncmer_fused_emit_units_beyond_the_tuple_list does for k_syncmer_pf, and BSK_NO_TILES keeps the batch whole)
            kk, ss = 64, 64 - w
            env = {"BSK_PF_DENSITY": "40", "BSK_NO_TILES": "1"} if w == 8 else {}
            hi = _longest(lambda ln: syn_pf_fits(kk, ss, ln, True, 40 if w == 8 else 0), SYN_SHORT_BASES + 1, SYN_TILE_MIN if w > 8 else 250)
            rows.append(Row("syn_pfl<%d>" % w, "syncmer", sp(kk, ss), "k_syncmer_pfl<%d>" % w, ["k_syncmer_pfl<%d>" % w], (200, 215, SYN_SHORT_BASES + 1),
                            (SYN_SHORT_BASES + 1, hi), env))
            if syn_pf_fits(kk, ss, SYN_SHORT_BASES, False):  # (w >= 16) one base fewer than k_syncmer_pfl's shortest: the short kernel at its own limit
                rows.append(Row("syn_pf_224<%d>" % w, "syncmer", sp(kk, ss), "k_syncmer_pf<%d>" % w, [], (200, 215, 220), (SYN_SHORT_BASES - 1, SYN_SHORT_BASES)))
        else:
            hi = _longest(lambda ln: syn_pf_fits(k, s, ln, True), base, SYN_TILE_MIN)
            rows.append(Row("syn_pfl<%d>" % w, "syncmer", sp(k, s), "k_syncmer_pfl<%d>" % w, ["k_syncmer_pfl<%d>" % w], lens + (hi - 60,), (hi - 1, hi)))
    for w in range(2, 33):
        s, k = SYN_S, SYN_S + w
        env = NO_PK if w <= 24 else {}  # (w <= 24: what a call that abandons a packed kernel re-plans to; 25..32: the wide form, planned as it is)
        rows.append(Row("syn_fast<%d>" % w, "syncmer", sp(k, s), "k_syncmer_fast<%d>" % w, ["k_syncmer_fast<%d>" % w], (100, 150, 250), (), env))
        if w <= 24:
            rows.append(Row("syn_side<%d>" % w, "syncmer", sp(k, s), "k_syncmer_fast<%d>" % w, ["k_syncmer_fast<%d,false,true>" % w], (100, 150, 250), (), env,
                            suffixes=(SIDE,), mixed=True, digest_env=NO_SIDE_DENSE))
    rows.append(Row("syn_pf<20>_binned", "syncmer", sp(31, 11), "k_syncmer_pf<20>", [], (80, 120, 150, 170), (), BIN, suffixes=(BINNED,)))
    rows.append(Row("syn_pk<20>_binned", "syncmer", sp(31, 11), "k_syncmer_pk<20>", [], (80, 120, 150, 170), (), _env(NO_SYN_PF, BIN), suffixes=(BINNED,)))
    rows.append(Row("syn_pfl<22>_binned", "syncmer", sp(33, 11), "k_syncmer_pfl<22>", [], (80, 150, 250, 350), (), BIN, suffixes=(BINNED,)))
    rows.append(Row("syn_pkl<22>_binned", "syncmer", sp(33, 11), "k_syncmer_pkl<22>", [], (80, 150, 250, 350), (), _env(NO_SYN_PF, BIN), suffixes=(BINNED,)))
    rows.append(Row("syn_fast<20>_binned", "syncmer", sp(31, 11), "k_syncmer_fast<20>", [], (80, 150, 200, 250), (), _env(NO_PK, BIN), suffixes=(BINNED,)))
    rows.append(Row("syn_generic<0>", "syncmer", sp(31, 11), "k_syncmer<0>", ["k_syncmer<0>"], (150, 300), (), GENERIC))
    rows.append(Row("syn_generic<0>_w40", "syncmer", sp(51, 11), "k_syncmer<0>", [], (150, 300), ()))
    rows.append(Row("syn_generic<1>", "syncmer", sp(51, 11), "k_syncmer<1>", ["k_syncmer<1>"], (150, 300), (), mixed=True))
    rows.append(Row("syn_generic<1>_forced", "syncmer", sp(31, 11), "k_syncmer<1>", [], (150, 300), (), GENERIC, mixed=True))
    return rows


# ---- stream kinds -----------------------------------------------------------------------------------------------------------------
def _stream_rows():
    rows = []
    top = (STREAM_BASES - 1, STREAM_BASES)
    over = (STREAM_BASES, STREAM_BASES + 1)
    for canon in (False, True):
        m = int(canon)
        p = dict(k=21, canonical=canon)
        rows.append(Row("nt_fast<%d>" % m, "nthash", p, "k_nthash_fast<%d>" % m, ["k_nthash_fast<%d>" % m], (60, 150, 400), top))
        rows.append(Row("nt_fast<%d>_513" % m, "nthash", p, "k_nthash_fast<%d>" % m, [], (60, 150, 400), over, suffixes=(TILES,)))
        rows.append(Row("nt_fast<%d>_side" % m, "nthash", p, "k_nthash_fast<%d>" % m, [], (60, 150, 400), top, suffixes=(SIDE,), mixed=True))
    rows.append(Row("nt_stream<0>", "nthash", dict(k=21, canonical=True), "k_nthash_stream<0>", ["k_nthash_stream<0>"], (60, 150, 400), top, GENERIC))
    rows.append(Row("nt_stream<0>_513", "nthash", dict(k=21, canonical=True), "k_nthash_stream<0>", [], (60, 150, 400), over, {"BSK_NO_TILES": "1"}))
    rows.append(Row("nt_stream<1>", "nthash", dict(k=21, canonical=False), "k_nthash_stream<1>", ["k_nthash_stream<1>"], (60, 150, 400), top, GENERIC, mixed=True))
    rows.append(Row("kmer_fast<2>", "kmer", dict(k=21, canonical=True), "k_nthash_fast<2>", ["k_nthash_fast<2>"], (60, 150, 400), top))
    rows.append(Row("kmer_fast<2>_513", "kmer", dict(k=21, canonical=True), "k_nthash_fast<2>", [], (60, 150, 400), over, suffixes=(TILES,)))
    rows.append(Row("kmer_fast<3>", "kmer", dict(k=21, canonical=False), "k_nthash_fast<3>", ["k_nthash_fast<3>"], (60, 150, 400), top))
    rows.append(Row("kmer_fast<4>", "kmer", dict(k=21, canonical=False), "k_nthash_fast<4>", ["k_nthash_fast<4>"], (60, 150, 400), over, suffixes=(TILES,)))
    rows.append(Row("kmer<0>", "kmer", dict(k=21, canonical=True), "k_kmer<0>", ["k_kmer<0>"], (60, 150, 400), top, GENERIC))
    rows.append(Row("kmer<0>_two_strand", "kmer", dict(k=21, canonical=False), "k_kmer<0>", [], (60, 150, 400), top, GENERIC))
    rows.append(Row("kmer<1>", "kmer", dict(k=21, canonical=True), "k_kmer<1>", ["k_kmer<1>"], (60, 150, 400), top, GENERIC, mixed=True))
    # SimHash: nh = k - m + 1 counters' worth of planes (<= 31: five, <= 63: six), three LDS sizes by the longest read; the homopolymer of
    # every row drives a counter to nh (every m-mer of its k-mers has the same bits set)
    for planes, (k, m) in ((5, (35, 5)), (6, (67, 5))):  # nh = 31 / 63: every plane of a full counter is 1
        nh = k - m + 1
        for words in (12, 20, 34):
            lim = SIM_BASES[words]
            prev = {12: 100, 20: 160, 34: 288}[words]
            name = "k_simhash_fast<%d,%d>" % (planes, words)
            rows.append(Row("sim_fast<%d,%d>" % (planes, words), "simhash", dict(k=k, m=m, scale=nh, canonical=True), name, [name], (prev - 20, prev, lim - 30),
                            (lim - 1, lim), extra=("AC" * (lim // 2), ("ACG" * lim)[:lim])))
            if words != 34:  # one base beyond: the next LDS size
                nxt = "k_simhash_fast<%d,%d>" % (planes, 20 if words == 12 else 34)
                rows.append(Row("sim_fast<%d,%d>_beyond" % (planes, words), "simhash", dict(k=k, m=m, scale=1, canonical=False), nxt, [], (prev, lim - 30),
                                (lim, lim + 1), extra=("AC" * (lim // 2), ("ACG" * lim)[:lim + 1])))
            else:
                rows.append(Row("sim_fast<%d,34>_513" % planes, "simhash", dict(k=k, m=m, scale=1, canonical=False), name, [], (prev, lim - 30), (lim, lim + 1),
                                suffixes=(TILES,)))
    rows.append(Row("sim<0>", "simhash", dict(k=68, m=5, scale=64, canonical=True), "k_simhash<0>", ["k_simhash<0>"], (100, 150, 400), top))  # nh = 64: scalar counters
    rows.append(Row("sim<0>_forced", "simhash", dict(k=21, m=5, scale=5, canonical=True), "k_simhash<0>", [], (100, 150, 400), top, GENERIC))
    rows.append(Row("sim<1>", "simhash", dict(k=68, m=5, scale=1, canonical=False), "k_simhash<1>", ["k_simhash<1>"], (100, 150, 400), top, mixed=True))
    return rows


# ---- protein kinds ----------------------------------------------------------------------------------------------------------------
FRAMES = (1, 2, 3, -1, -2, -3)


def _protein_rows():
    rows = []
    for k in range(4, 17):
        rows.append(Row("ph_fast<%d,false>" % k, "prot_hash", dict(k=k), "k_prot_hash_fast<%d,false>" % k, ["k_prot_hash_fast<%d,false>" % k], (47, 300, 700),
                        (3 * k, 255, 256, 257, 256 + k - 1), alphabet="protein", n=100))
        rows.append(Row("ph_fast<%d,true>" % k, "prot_hash", dict(k=k, codon_table=1 + (k % 2) * 10, frame=FRAMES[k % 6]), "k_prot_hash_fast<%d,true>" % k,
                        ["k_prot_hash_fast<%d,true>" % k], (150, 900, 1500), (3 * k, 3 * k + 1, 3 * k + 2, 768, 771), n=100))
    rows.append(Row("ph_general_k3", "prot_hash", dict(k=3), "k_prot_hash", ["k_prot_hash"], (47, 300, 700), (), alphabet="protein", n=100))
    rows.append(Row("ph_general_k17", "prot_hash", dict(k=17), "k_prot_hash", [], (47, 300, 700), (), alphabet="protein", n=100))
    rows.append(Row("ph_general_dna_k17", "prot_hash", dict(k=17, codon_table=11, frame=-2), "k_prot_hash", [], (150, 900, 1500), (51, 52, 53), n=100))  # (translated first)
    rows.append(Row("ph_general_forced", "prot_hash", dict(k=9), "k_prot_hash", [], (47, 300, 700), (), GENERIC, alphabet="protein", n=100))
    for w in range(2, 9):
        for k in range(4, 17):
            name = "k_prot_minimizer_fast<%d,%d,false>" % (w, k)
            lc = k + w - 2 + slab_tuples(500 - k - w + 2, w)
            rows.append(Row("pm_fast<%d,%d,false>" % (w, k), "prot_minimizer", dict(k=k, w=w), name, [name], (100, 300, 500), (3 * k + w - 2, 3 * k + w - 1, 500), alphabet="protein", n=72,
                            lc_max=lc))
            name = "k_prot_minimizer_fast<%d,%d,true>" % (w, k)
            rows.append(Row("pm_fast<%d,%d,true>" % (w, k), "prot_minimizer", dict(k=k, w=w, codon_table=1 + (k % 2) * 10, frame=FRAMES[(w + k) % 6]), name, [name],
                            (300, 900, 1500), (3 * k, 3 * k + w - 1, 3 * (k + w) + 1, 901, 1500), n=72, lc_max=3 * (k + w - 2 + slab_tuples(500 - k - w + 2, w)) - 6))
    # fallback, as production reaches it: a homopolymer of full length outgrows its slab, the call abandons the register kernel and re-plans
    rows.append(Row("pm_fallback<5,9>", "prot_minimizer", dict(k=9, w=5), "k_prot_minimizer", [], (100, 300, 500), (500,), alphabet="protein", n=100))
    rows.append(Row("pm_general_w9", "prot_minimizer", dict(k=9, w=9), "k_prot_minimizer", ["k_prot_minimizer"], (100, 300, 500), (), alphabet="protein", n=100))
    rows.append(Row("pm_general_k17", "prot_minimizer", dict(k=17, w=5), "k_prot_minimizer", [], (100, 300, 500), (), alphabet="protein", n=100))
    rows.append(Row("pm_general_dna_k17", "prot_minimizer", dict(k=17, w=5, codon_table=1, frame=2), "k_prot_minimizer", [], (300, 900, 1500), (51, 55, 56, 66), n=100))  # (translated first)
    rows.append(Row("pm_general_dna_w9", "prot_minimizer", dict(k=5, w=9, codon_table=1, frame=-1), "k_prot_minimizer", [], (300, 900, 1500), (15, 23, 24, 39), n=100))
    rows.append(Row("pm_general_forced", "prot_minimizer", dict(k=9, w=5), "k_prot_minimizer", [], (100, 300, 500), (), GENERIC, alphabet="protein", n=100))
    return rows


ROWS = _minimizer_rows() + _syncmer_rows() + _stream_rows() + _protein_rows()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)


def covered():
    return {c for r in ROWS for c in r.covers}
