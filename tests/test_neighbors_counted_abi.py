"""CPU: the entries of the weighted sparse all-pairs comparison (bsk_sets_neighbors_counted, bsk_hits_weights_device,
bsk_hits_fetch_weights) -- declared with the contract's prototypes between bsk_hits_from_host and the neighbours block, bound by
bio_amd._lib, called from the Go shim and the C++ owners, exported by the library, their argument checks as far as they run without a
device, and the arithmetic of Hits.cosine / angular_similarity / weighted_jaccard / bray_curtis."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import compare_counted_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "bsk_sets_neighbors_counted": "int bsk_sets_neighbors_counted(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, uint64_t limit, "
                                  "const struct bsk_neighbor_params *np, bsk_hits **hits);",
    "bsk_hits_weights_device": "int bsk_hits_weights_device(const bsk_hits *h, const uint64_t **dot, const uint64_t **min_sum);",
    "bsk_hits_fetch_weights": "int bsk_hits_fetch_weights(bsk_ctx *ctx, const bsk_hits *h, uint64_t first, uint64_t count, uint64_t *dot, uint64_t *min_sum, uint64_t hit_cap);",
}
ARITY = dict(bsk_sets_neighbors_counted=6, bsk_hits_weights_device=3, bsk_hits_fetch_weights=7)


def _norm(s):
    s = re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    return re.sub(r"\s+", " ", s).replace("( ", "(").replace(" )", ")").replace(" ;", ";").replace(" ,", ",").strip()


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_header_declares_the_entries():
    raw = _read("include", "biosketch.h")
    hdr = _norm(raw)
    for name, proto in ENTRIES.items():
        assert _norm(proto) in hdr, name
    assert "#define BSK_ABI_VERSION 1" in hdr
    # after bsk_hits_from_host, before the neighbours block (which still closes the header), the params struct declared forward
    order = ["int bsk_hits_from_host(", "struct bsk_neighbor_params;", "int bsk_sets_neighbors_counted(", "int bsk_hits_weights_device(", "int bsk_hits_fetch_weights(",
             "enum { BSK_NEIGHBORS_UPPER", "typedef struct bsk_neighbor_params {", "int bsk_sets_neighbors("]
    at = [hdr.index(x) for x in order]
    assert at == sorted(at)
    assert hdr.count("BSK_NEIGHBORS_UPPER =") == 1 and hdr.count("typedef struct bsk_neighbor_params") == 1  # no new flag, no new struct
    start, end = raw.index("/* ---- weighted sparse all-pairs comparison"), raw.index("/* ---- sparse all-pairs comparison")
    assert raw.index("int bsk_hits_from_host(") < start < end
    block = raw[start:end]
    for said in ("defined in the block below", "bit-identical", "payload", "do not take part in the rule", "dot[n_hits]", "min_sum[n_hits]", "bsk_sets_compare_counted",
                 "saturating", "2^64-1", "exact sum", "An uncounted operand counts 1", "dot == min_sum == shared", "2^32", "NO limit on cells", "BSK_NEIGHBORS_UPPER",
                 "never run", "The result slot", "null,", "flag, fraction, foreign context", "bsk_index_search", "bsk_hits_top", "hits sink", "bsk_hits_from_host",
                 "unweighted bsk_sets_neighbors", "only grow", "neither totals nor weights", "_cluster", "both NULL for hits without weights", "bsk_hits_fetch_totals",
                 "BSK_ERR_ARG for hits without weights", "k_cmp_tile_nb_w", "tiles=", "skipped=", "rounds=", "runs="):
        assert said in block, said
    slot = raw[raw.index("/* The result slot."):raw.index("int bsk_result_sets_reuse(")]
    assert "_neighbors_counted" in slot
    route = raw[raw.index("/* ---- sparse all-pairs comparison"):]
    assert "bsk_sets_neighbors_counted" in route[route.index("Which route"):]


def test_python_binds_go_and_cpp_call_them():
    from bio_amd import _lib
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    go, hpp = _read("bindings", "go", "sketches", "compare.go"), _read("bio_amd", "csrc", "sketches.hpp")
    for name in ENTRIES:
        assert name in bound and len(bound[name][1]) == ARITY[name] and bound[name][0] is C.c_int, name
        assert f"C.{name}(" in go, name
        assert name + "(" in hpp, name
    assert bound["bsk_sets_neighbors_counted"][1] == bound["bsk_sets_neighbors"][1] and bound["bsk_sets_neighbors_counted"][1][3] is C.c_uint64
    fw = bound["bsk_hits_fetch_weights"][1]
    assert fw[2] is C.c_uint64 and fw[3] is C.c_uint64 and fw[6] is C.c_uint64 and fw == bound["bsk_compare_fetch_weights"][1]
    for m in ("func (a *Sets) NeighborsCounted(b *Sets, limit uint64, p NeighborParams, reuse *Hits) (*Hits, error)", "func (h *Hits) Weights() (dot, minSum unsafe.Pointer)",
              "func (h *Hits) FetchWeights(first, count uint64) (dot, minSum []uint64, err error)"):
        assert m in go, m
    assert go.count("type NeighborParams struct") == 1
    for m in ("DeviceSets::neighbors_counted(", "weights_device()", "fetch_weights("):
        assert m in hpp, m
    from bio_amd import sketches as S
    sig, plain = inspect.signature(S.Sets.neighbors_counted).parameters, inspect.signature(S.Sets.neighbors).parameters
    assert list(sig) == ["self", "other", "limit", "min_shared", "min_jaccard", "upper", "reuse"] == list(plain)
    assert [sig[k].default for k in list(sig)[1:]] == [None, 0, 1, None, False, None] == [plain[k].default for k in list(plain)[1:]]
    assert isinstance(S.Hits.dot, property) and isinstance(S.Hits.min_sum, property)
    for m in ("has_weights", "fetch_weights", "cosine", "angular_similarity", "weighted_jaccard", "bray_curtis"):
        assert callable(getattr(S.Hits, m)), m
    assert "operands" in inspect.signature(S.Hits._bind).parameters and inspect.signature(S.Hits._bind).parameters["operands"].default is None
    assert S.Hits._weights is None and S.Hits._norms is None and S.Hits._operands is None  # class-level defaults: subclasses that set _host alone keep working


def test_the_kernel_lives_where_the_build_expects_it():
    mk = _read("bio_amd", "csrc", "Makefile")
    assert re.search(r"^test_neighbors_counted:.*tests/cpp/test_neighbors_counted\.cpp.*sketches\.hpp.*libbiosketch\.so", mk, re.M)
    assert re.search(r"^\trm -f .*\btest_neighbors_counted\b", mk, re.M)
    assert '"test_neighbors_counted"' in _read("__graft_entry__.py")
    assert "bio_amd/csrc/test_neighbors_counted" in _read(".gitignore").split()
    src = _read("bio_amd", "csrc", "compare.hip")
    assert "void k_cmp_tile_nb_w(" in src and "void k_nb_place_w(" in src and "SLOT_NB_WEIGHTS" in src and "->cus" not in src
    assert re.search(r"static_assert\(.*160 \* 1024 / CMP_W_BLOCKS_PER_CU", src)  # the LDS total, stated against a third of a CU's
    assert "capped_grid(ctx, ntiles, weighted ? CMP_W_BLOCKS_PER_CU : CMP_BLOCKS_PER_CU)" in src
    assert src.count("int neighbors_impl(") == 1  # one host path with a flag, not a copy
    types = _read("bio_amd", "csrc", "host_types.hpp")
    slots = {k: int(v) for k, v in re.findall(r"\b(SLOT_\w+|POOL_SLOTS) = (\d+)", types)}
    assert slots["SLOT_NB_WEIGHTS"] < slots["POOL_SLOTS"] and list(slots.values()).count(slots["SLOT_NB_WEIGHTS"]) == 1
    internal = _read("bio_amd", "csrc", "search_internal.hpp")
    for field in ("*dot", "*msum", "c_dot", "c_msum", "bool has_weights = false"):
        assert field in internal, field


def test_whoever_clears_the_totals_clears_the_weights():
    """every place that writes hits without totals also leaves them without weights: has_weights is cleared beside has_total, line for line"""
    for path in (("bio_amd", "csrc", "search.hip"), ("bio_amd", "csrc", "compare.hip")):
        lines = _read(*path).splitlines()
        cleared = [k for k, ln in enumerate(lines) if re.search(r"\bres->has_total = false;", ln)]
        assert cleared, path
        for k in cleared:
            assert re.search(r"\bres->has_weights = false;", lines[k + 1]), (path, k + 1, lines[k])
    search = _read("bio_amd", "csrc", "search.hip")
    assert len(re.findall(r"res->has_total = false;", search)) == 3  # bsk_hits_from_host, the search (and through it the pipeline's sink), bsk_hits_top
    assert "hipFree(h->dot)" in search and "hipFree(h->msum)" in search
    assert "has_weights" not in _read("bio_amd", "csrc", "pipeline.cpp")  # the sink goes through bsk_index_search and bsk_hits_top


@pytest.fixture(scope="module")
def lib():
    from bio_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_library_exports_them(lib):
    from bio_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (bsk_\w+)", out))
    assert set(ENTRIES) <= exported
    assert not [s for s in re.findall(r" [TW] (\S*(?:neighbors_impl|k_cmp_tile_nb_w|k_nb_place_w|NbRule)\S*)", out)]  # the helpers stay inside the library
    declared = set(re.findall(r"\b(bsk_\w+)\(", _norm(_read("include", "biosketch.h"))))
    assert exported <= declared, exported - declared


def test_null_and_bad_arguments_without_a_device(lib):
    from bio_amd import _lib as L
    fake = C.create_string_buffer(1024)  # zeroed: a bsk_sets / bsk_hits of no context and nothing in it -- every case below fails its checks first
    fp = C.addressof(fake)
    hits = C.c_void_p(4321)
    for a, b in ((None, None), (fp, None), (None, fp), (fp, fp)):
        assert lib.bsk_sets_neighbors_counted(None, a, b, 0, None, C.byref(hits)) == L.ERR_ARG and hits.value == 4321  # an argument error leaves *hits
    assert lib.bsk_sets_neighbors_counted(None, fp, fp, 7, None, None) == L.ERR_ARG
    for bad in (L.NeighborParams(1, 2, 0, 0), L.NeighborParams(1, 1 | 4, 0, 0), L.NeighborParams(1, 0x80000000, 0, 0), L.NeighborParams(1, 0, 3, 2),
                L.NeighborParams(0, 1, 0xFFFFFFFF, 0xFFFFFFFE)):
        assert lib.bsk_sets_neighbors_counted(None, fp, fp, 0, C.byref(bad), C.byref(hits)) == L.ERR_ARG and hits.value == 4321
    d, m = C.c_void_p(55), C.c_void_p(66)
    assert lib.bsk_hits_weights_device(None, C.byref(d), C.byref(m)) == L.ERR_ARG and (d.value, m.value) == (55, 66)
    assert lib.bsk_hits_weights_device(fp, C.byref(d), C.byref(m)) == L.OK and d.value is None and m.value is None  # hits without weights: NULLs
    d = C.c_void_p(55)
    assert lib.bsk_hits_weights_device(fp, C.byref(d), None) == L.OK and d.value is None and lib.bsk_hits_weights_device(fp, None, None) == L.OK
    ww = np.full(4, 7, np.uint64)
    assert lib.bsk_hits_fetch_weights(None, fp, 0, 0, ww.ctypes.data, ww.ctypes.data, 4) == L.ERR_ARG
    assert lib.bsk_hits_fetch_weights(None, None, 0, 0, None, None, 0) == L.ERR_ARG and list(ww) == [7] * 4


def test_the_order_of_the_checks():
    """null, flag, fraction, foreign context, all before the slot is taken; the limits inside it -- read from the source, as for bsk_sets_neighbors"""
    src = _read("bio_amd", "csrc", "compare.hip")
    body = src[src.index('extern "C" int bsk_sets_neighbors_counted('):]
    body = body[:body.index('extern "C" int bsk_hits_weights_device(')]
    at = [body.index(x) for x in ("null argument", "unknown flag", "jaccard_num > jaccard_den", "another context", "take_over(", "2^32 values or more", "2^32 sets or more",
                                  "neighbors_impl(ctx, a, b, limit, rule, res, reused, weighted)")]
    assert at == sorted(at) and "neighbors_entry(ctx, a, b, limit, np, hits, true)" in body[:at[0]]
    # one helper serves both entries: every message exists once per prefix, chosen by the flag
    said = re.findall(r'weighted \? "bsk_sets_neighbors_counted: ([^"]*)" : "bsk_sets_neighbors: ([^"]*)"', body)
    assert len(said) == 6 and all(x == y for x, y in said) and len(re.findall(r'"bsk_sets_neighbors\w*: ', body)) == 12
    fetch = src[src.index('extern "C" int bsk_hits_fetch_weights('):]
    fetch = fetch[:fetch.index('extern "C" int bsk_hits_totals_device(')]
    at = [fetch.index(x) for x in ("null argument", "another context", "carry no weights", "range outside the hits", "hipSetDevice", "hit_cap too small")]
    assert at == sorted(at)


class Fixed:
    """Hits with arrays put in by hand (no device): built in make() so that the subclass exists only where bio_amd imports"""

    @staticmethod
    def make(offsets, target, shared, total, dot, ms, qa, qb, ta, tb):
        from bio_amd import sketches as S

        class _Fixed(S.Hits):
            def __init__(self):
                self.eng, self.h = None, None
                self._host = (np.array(offsets, np.uint64), np.array(target, np.uint32), np.array(shared, np.uint32))
                self._totals = np.array(total, np.uint32)
                if dot is not None:
                    self._weights = (np.array(dot, np.uint64), np.array(ms, np.uint64))
                    self._norms = tuple(np.array(x, np.uint64) for x in (qa, qb, ta, tb))

        return _Fixed()


def test_python_mirror_arithmetic():
    """Hits.cosine and its kin on hand-filled arrays against the references of compare_counted_cases: per hit what Compare gives per cell,
    a saturated dot or norm -> NaN, a zero norm -> 0.0"""
    top = WC.MAX
    # 3 x 3 cells, six of them hits; row 1 has a zero norm, column 2 a saturated one, hit (2, 0) a saturated dot
    dot = np.array([[12, 0, 5], [0, 0, 0], [top, 7, 9]], np.uint64)
    ms = np.array([[3, 0, 2], [0, 0, 0], [40, 4, 6]], np.uint64)
    qa, qb = np.array([30, 0, 1 << 62], np.uint64), np.array([89, 9, top], np.uint64)
    ta, tb = np.array([10, 0, 1 << 40], np.uint64), np.array([15, 3, 1 << 41], np.uint64)
    offsets, target = [0, 2, 3, 6], [0, 2, 1, 0, 1, 2]
    i, j = np.array([0, 0, 1, 2, 2, 2]), np.array(target)
    h = Fixed.make(offsets, target, [2, 1, 1, 3, 1, 2], [5, 4, 4, 6, 6, 6], dot[i, j], ms[i, j], qa, qb, ta, tb)
    assert h.has_weights() and h.dot.tolist() == dot[i, j].tolist() and h.min_sum.tolist() == ms[i, j].tolist() and h.query().tolist() == i.tolist()
    cos, want = h.cosine(), WC.ref_cosine(dot, qa, qb)[i, j]
    assert cos.dtype == np.float64 and np.isnan(cos).tolist() == [False, True, False, True, False, True] == np.isnan(want).tolist()
    ok = ~np.isnan(want)
    assert cos[ok] == pytest.approx(want[ok], rel=1e-15) and cos[0] == 12 / (np.sqrt(30.0) * np.sqrt(89.0)) and cos[2] == 0.0  # (1, 1): a zero norm
    ang, want = h.angular_similarity(), WC.ref_angular(WC.ref_cosine(dot, qa, qb))[i, j]
    assert np.isnan(ang).tolist() == np.isnan(want).tolist() and ang[ok] == pytest.approx(want[ok], rel=1e-15) and ang[2] == 0.0
    assert h.weighted_jaccard() == pytest.approx(WC.ref_weighted_jaccard(ms, ta, tb)[i, j], rel=1e-15) and h.weighted_jaccard()[0] == 3 / 22
    assert h.bray_curtis() == pytest.approx(WC.ref_bray_curtis(ms, ta, tb)[i, j], rel=1e-15) and h.bray_curtis()[0] == 1 - 6 / 25
    assert h.weighted_jaccard()[2] == 0.0 and h.bray_curtis()[2] == 1.0  # hit (1, 1): nothing in common with an empty set
    # the dense mirror on the same numbers: the same formula, cell for cell
    from bio_amd import sketches as S

    class Dense(S.Compare):
        def __init__(self):
            self.eng, self.h, self._host = None, None, None
            self._whost, self._norms = (dot, ms), (qa, qb, ta, tb)

        def info(self):
            return dict(n_a=3, n_b=3, limit=0)

    d = Dense()
    for name in ("cosine", "angular_similarity", "weighted_jaccard", "bray_curtis"):
        assert np.array_equal(getattr(h, name)(), getattr(d, name)()[i, j], equal_nan=True), name
    # without weights: None, and the formulas raise
    plain = Fixed.make(offsets, target, [2, 1, 1, 3, 1, 2], [5, 4, 4, 6, 6, 6], None, None, None, None, None, None)
    assert not plain.has_weights() and plain.dot is None and plain.min_sum is None and plain.has_totals()
    for name in ("cosine", "angular_similarity", "weighted_jaccard", "bray_curtis"):
        with pytest.raises(ValueError):
            getattr(plain, name)()
    # the thresholds of neighbors_counted are those of neighbors: a bad fraction raises before any call

    class NoCall(S.Sets):
        def __init__(self):
            self.eng, self.h = None, None

    for x in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            NoCall().neighbors_counted(min_jaccard=x)
