"""CPU: the entries of the sparse all-pairs comparison (bsk_sets_neighbors, bsk_hits_totals_device, bsk_hits_fetch_totals) -- declared with
the contract's prototypes after bsk_sets_sumsq, bound by bio_amd._lib, called from the Go shim and the C++ owners, exported by the library,
their argument checks as far as they run without a device, and the arithmetic of Hits.jaccard / mash_distance."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "bsk_sets_neighbors": "int bsk_sets_neighbors(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, uint64_t limit, "
                          "const bsk_neighbor_params *np, bsk_hits **hits);",
    "bsk_hits_totals_device": "int bsk_hits_totals_device(const bsk_hits *h, const uint32_t **total);",
    "bsk_hits_fetch_totals": "int bsk_hits_fetch_totals(bsk_ctx *ctx, const bsk_hits *h, uint64_t first, uint64_t count, uint32_t *total, uint64_t hit_cap);",
}
ARITY = dict(bsk_sets_neighbors=6, bsk_hits_totals_device=2, bsk_hits_fetch_totals=6)


def _norm(s):
    s = re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    return re.sub(r"\s+", " ", s).replace("( ", "(").replace(" )", ")").replace(" ;", ";").replace(" ,", ",").strip()


def test_header_declares_the_entries():
    raw = open(os.path.join(ROOT, "include", "biosketch.h")).read()
    hdr = _norm(raw)
    for name, proto in ENTRIES.items():
        assert _norm(proto) in hdr, name
    assert "enum { BSK_NEIGHBORS_UPPER = 1 };" in hdr and "#define BSK_ABI_VERSION 1" in hdr
    assert _norm("typedef struct bsk_neighbor_params { uint32_t min_shared; uint32_t flags; uint32_t jaccard_num; uint32_t jaccard_den; } bsk_neighbor_params;") in hdr
    # the block follows bsk_sets_sumsq and closes the header
    assert hdr.index("int bsk_sets_sumsq(") < hdr.index("enum { BSK_NEIGHBORS_UPPER") < hdr.index("typedef struct bsk_neighbor_params") < hdr.index("int bsk_sets_neighbors(")
    assert hdr.index("int bsk_sets_neighbors(") < hdr.index("int bsk_hits_totals_device(") < hdr.index("int bsk_hits_fetch_totals(") < hdr.rindex("#ifdef __cplusplus")
    assert not re.search(r"\bint bsk_\w+\(", hdr[hdr.index("int bsk_hits_fetch_totals(") + 10:])
    block = raw[raw.index("/* ---- sparse all-pairs comparison"):]
    for said in ("shared >= max(min_shared, 1)", "jaccard_den == 0", "j > i", "NO limit on cells", "2^32", "bsk_hits_top", "carries no", "total == limit",
                 "bit-identical", "k_cmp_tile_nb", "tiles=", "skipped=", "rounds=", "runs=", "Which route", "bsk_index_search", "bsk_sets_compare", "The result slot"):
        assert said in block, said


def test_python_binds_go_and_cpp_call_them():
    from bio_amd import _lib
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    go = open(os.path.join(ROOT, "bindings", "go", "sketches", "compare.go")).read()
    hpp = open(os.path.join(ROOT, "bio_amd", "csrc", "sketches.hpp")).read()
    for name in ENTRIES:
        assert name in bound and len(bound[name][1]) == ARITY[name] and bound[name][0] is C.c_int, name
        assert f"C.{name}(" in go, name
        assert name + "(" in hpp, name
    assert bound["bsk_sets_neighbors"][1][3] is C.c_uint64
    assert bound["bsk_hits_fetch_totals"][1][2] is C.c_uint64 and bound["bsk_hits_fetch_totals"][1][3] is C.c_uint64 and bound["bsk_hits_fetch_totals"][1][5] is C.c_uint64
    assert [f for f, _ in _lib.NeighborParams._fields_] == ["min_shared", "flags", "jaccard_num", "jaccard_den"]
    assert all(t is C.c_uint32 for _, t in _lib.NeighborParams._fields_) and C.sizeof(_lib.NeighborParams) == 16 and _lib.NEIGHBORS_UPPER == 1
    for m in ("func (a *Sets) Neighbors(b *Sets, limit uint64, p NeighborParams, reuse *Hits) (*Hits, error)", "type NeighborParams struct",
              "func (h *Hits) Totals(", "func (h *Hits) FetchTotals(", "C.BSK_NEIGHBORS_UPPER"):
        assert m in go, m
    for m in ("DeviceSets::neighbors(", "totals_device()", "fetch_totals("):
        assert m in hpp, m
    from bio_amd import sketches as S
    sig = inspect.signature(S.Sets.neighbors).parameters
    assert list(sig) == ["self", "other", "limit", "min_shared", "min_jaccard", "upper", "reuse"]
    assert [sig[k].default for k in list(sig)[1:]] == [None, 0, 1, None, False, None]
    assert isinstance(S.Hits.total, property) and list(inspect.signature(S.Hits.mash_distance).parameters) == ["self", "k"]


def test_the_kernel_lives_where_the_build_expects_it():
    mk = open(os.path.join(ROOT, "bio_amd", "csrc", "Makefile")).read()
    assert re.search(r"compare\.o:.*search_internal\.hpp", mk) and re.search(r"^test_neighbors:.*tests/cpp/test_neighbors\.cpp", mk, re.M)
    assert re.search(r"^\trm -f .*\btest_neighbors\b", mk, re.M)
    assert '"test_neighbors"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    src = open(os.path.join(ROOT, "bio_amd", "csrc", "compare.hip")).read()
    assert "void k_cmp_tile_nb(" in src and "sets_sort_segments_u64(" in src and "scan_counts(" in src
    assert "struct bsk_hits {" in open(os.path.join(ROOT, "bio_amd", "csrc", "search_internal.hpp")).read()
    assert "struct bsk_hits {" not in open(os.path.join(ROOT, "bio_amd", "csrc", "search.hip")).read()
    assert "BSK_NB_ROOM" in open(os.path.join(ROOT, "bio_amd", "csrc", "biosketch.hip")).read()


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
    assert not [s for s in re.findall(r" [TW] (\S*(?:neighbors_impl|k_cmp_tile_nb|k_nb_keys|k_nb_place|NbRule)\S*)", out)]  # the helpers stay inside the library
    declared = set(re.findall(r"\b(bsk_\w+)\(", _norm(open(os.path.join(ROOT, "include", "biosketch.h")).read())))
    assert exported <= declared, exported - declared  # the header's entries and no more


def test_null_and_bad_arguments_without_a_device(lib):
    from bio_amd import _lib as L
    fake = C.create_string_buffer(1024)  # zeroed: a bsk_sets / bsk_hits of no context and nothing in it -- every case below fails its checks first
    fp = C.addressof(fake)
    hits = C.c_void_p(4321)
    for a, b in ((None, None), (fp, None), (None, fp), (fp, fp)):
        assert lib.bsk_sets_neighbors(None, a, b, 0, None, C.byref(hits)) == L.ERR_ARG and hits.value == 4321  # an argument error leaves *hits
    assert lib.bsk_sets_neighbors(None, fp, fp, 7, None, None) == L.ERR_ARG
    for bad in (L.NeighborParams(1, 2, 0, 0), L.NeighborParams(1, 1 | 4, 0, 0), L.NeighborParams(1, 0x80000000, 0, 0), L.NeighborParams(1, 0, 3, 2),
                L.NeighborParams(0, 1, 0xFFFFFFFF, 0xFFFFFFFE)):
        assert lib.bsk_sets_neighbors(None, fp, fp, 0, C.byref(bad), C.byref(hits)) == L.ERR_ARG and hits.value == 4321
    t = C.c_void_p(55)
    assert lib.bsk_hits_totals_device(None, C.byref(t)) == L.ERR_ARG and t.value == 55
    assert lib.bsk_hits_totals_device(fp, C.byref(t)) == L.OK and t.value is None  # hits without totals: NULL
    assert lib.bsk_hits_totals_device(fp, None) == L.OK
    tt = np.full(4, 7, np.uint32)
    assert lib.bsk_hits_fetch_totals(None, fp, 0, 0, tt.ctypes.data, 4) == L.ERR_ARG
    assert lib.bsk_hits_fetch_totals(None, None, 0, 0, None, 0) == L.ERR_ARG and list(tt) == [7] * 4


def test_the_rule_checks_need_a_context_to_tell_them_apart():
    """the flag and fraction checks come before the context checks: with a fake context-less ctx they cannot be reached, so the order is read from the source"""
    src = open(os.path.join(ROOT, "bio_amd", "csrc", "compare.hip")).read()
    body = src[src.index('extern "C" int bsk_sets_neighbors('):]
    body = body[:body.index("take_over(")]
    assert body.index("null argument") < body.index("unknown flag") < body.index("jaccard_num > jaccard_den") < body.index("another context")


def test_python_mirror_arithmetic():
    """Hits.jaccard / mash_distance on arrays put in by hand (no device): with totals shared / total, without them the sizes' Jaccard"""
    from bio_amd import sketches as S

    class Fixed(S.Hits):
        def __init__(self, offsets, target, shared, total, qsizes, tsizes):
            self.eng, self.h = None, None
            self._host = (np.array(offsets, np.uint64), np.array(target, np.uint32), np.array(shared, np.uint32))
            self._totals = None if total is None else np.array(total, np.uint32)
            self.query_sizes, self.target_sizes = np.array(qsizes, np.uint64), np.array(tsizes, np.uint64)

    h = Fixed([0, 2, 2, 3], [0, 2, 1], [4, 1, 2], [4, 3, 4], [4, 0, 3], [4, 3, 2])
    assert h.has_totals() and h.total.tolist() == [4, 3, 4] and h.query().tolist() == [0, 0, 2]
    j = h.jaccard()
    assert j.dtype == np.float64 and j.tolist() == [1.0, 1 / 3, 0.5]
    d = h.mash_distance(21)
    assert d[0] == 0.0 and d[1] == pytest.approx(-np.log(2 * (1 / 3) / (1 + 1 / 3)) / 21, rel=1e-15) and d[2] == pytest.approx(-np.log(2 * 0.5 / 1.5) / 21, rel=1e-15)

    class Dense(S.Compare):  # Compare.mash_distance on the same cells: the same formula, cell for cell
        def __init__(self, shared, total):
            self.h, self._host = None, (np.array(shared, np.uint32), np.array(total, np.uint32))

    assert np.array_equal(d, Dense([[4, 1, 2]], [[4, 3, 4]]).mash_distance(21)[0])
    plain = Fixed([0, 2, 2, 3], [0, 2, 1], [4, 1, 2], None, [4, 0, 3], [4, 3, 2])
    assert not plain.has_totals() and plain.total is None
    assert plain.jaccard().tolist() == [4 / (4 + 4 - 4), 1 / (4 + 2 - 1), 2 / (3 + 3 - 2)]
    assert plain.mash_distance(21)[0] == 0.0
    # min_jaccard: a float is turned into (ceil(x * 2^30), 2^30); outside 0..1 raises before any call
    class NoCall(S.Sets):
        def __init__(self):
            self.eng, self.h = None, None
    for x in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            NoCall().neighbors(min_jaccard=x)
