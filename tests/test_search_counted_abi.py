"""CPU: the entries of the weighted containment search (bsk_index_build_counted, bsk_index_counted, bsk_index_fetch_norms,
bsk_index_search_counted) -- declared with the contract's prototypes between bsk_sets_sumsq and the window-sets block, bound by
bio_amd._lib, called from the Go shim and the C++ owners, exported by the library, the order of their checks read from the source, their
argument checks as far as they run without a device, and the arithmetic of Hits.weighted_containment."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import search_counted_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "bsk_index_build_counted": "int bsk_index_build_counted(bsk_ctx *ctx, const bsk_sets *targets, bsk_index **out);",
    "bsk_index_counted": "int bsk_index_counted(const bsk_index *ix, int *counted);",
    "bsk_index_fetch_norms": "int bsk_index_fetch_norms(bsk_ctx *ctx, const bsk_index *ix, uint64_t first, uint64_t count, uint64_t *sumsq, uint64_t *totals);",
    "bsk_index_search_counted": "int bsk_index_search_counted(bsk_ctx *ctx, const bsk_index *ix, const bsk_sets *queries, const bsk_search_params *sp, bsk_hits **hits);",
}
ARITY = dict(bsk_index_build_counted=3, bsk_index_counted=2, bsk_index_fetch_norms=6, bsk_index_search_counted=5)
KERNELS = ("k_ix_ord", "k_ix_gather", "k_sw_row", "k_sw_chunk", "k_sw_finish")


def _norm(s):
    s = re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    return re.sub(r"\s+", " ", s).replace("( ", "(").replace(" )", ")").replace(" ;", ";").replace(" ,", ",").strip()


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_header_declares_the_entries_in_their_place():
    raw = _read("include", "biosketch.h")
    hdr = _norm(raw)
    for name, proto in ENTRIES.items():
        assert _norm(proto) in hdr, name
        assert not any(x in name for x in ("windows", "fold", "members", "cluster")), name  # other tests pick exports by these substrings
    assert "#define BSK_ABI_VERSION 1" in hdr
    order = ["int bsk_sets_sumsq(", "int bsk_index_build_counted(", "int bsk_index_counted(", "int bsk_index_fetch_norms(", "int bsk_index_search_counted(",
             "enum { BSK_WINDOWS_COUNTED", "int bsk_hits_fold(", "int bsk_hits_cluster(", "int bsk_sets_neighbors_counted(", "enum { BSK_NEIGHBORS_UPPER", "int bsk_sets_neighbors(",
             "int bsk_hits_fetch_totals("]
    at = [hdr.index(x) for x in order]
    assert at == sorted(at)
    assert "bsk_" not in _norm(raw[raw.index("int bsk_hits_fetch_totals("):]).split(";", 1)[1] and raw.index("/* ---- sparse all-pairs comparison") > raw.index("/* ---- weighted sparse all-pairs comparison")  # the neighbours block closes the header
    a, b = raw.index("/* ---- weighted containment search"), raw.index("/* ---- window sets and folded hits")
    assert raw.index("int bsk_sets_sumsq(") < a < b
    block = raw[a:b]
    for said in ("V = q & t", "cq(v) * ct(v)", "2^64-1", "min(cq(v), ct(v))", "exact", "bsk_sets_compare_counted", "bsk_sets_neighbors_counted with limit == 0",
                 "dot == min_sum == shared", "1 for uncounted queries", "1 for an index without counts", "post_cnt[n_postings]", "as bsk_sets_sumsq", "as bsk_sets_totals",
                 "owns copies", "bit-identical to bsk_index_build", "device_bytes grows", "exactly what bsk_index_build", "only writes its slot", "itself is", "unchanged",
                 "either out array may be NULL", "rules of bsk_sets_totals", "reports |t| for both", "bit-identical to bsk_index_search", "thresholds", "read shared only",
                 "payload", "no totals and no members", "four combinations", "null, foreign context, reserved, covers", "2^32 limits", "The result slot", "k_sw_row", "k_sw_chunk",
                 "512 hits", "256 query values", "bit-identical from call to call", "; weights:", "large queries is the search's", "bsk_index_attach", "copies them to another device",
                 "hits sink", "bsk_hits_top", "bsk_hits_fold", "keeps the arrays", "thresholds on the weighted measures", "a weighted hits sink", "share of the query's k-mer mass"):
        assert said in block, said
    assert str(W.SW_ROW) + " hits" in block and str(W.SW_CHUNK) + " query values" in block  # the header states the caps the source has
    slot = raw[raw.index("/* The result slot."):raw.index("int bsk_result_sets_reuse(")]
    assert "bsk_index_search_counted" in slot


def test_python_binds_go_and_cpp_call_them():
    from bio_amd import _lib
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    go, hpp = _read("bindings", "go", "sketches", "search.go"), _read("bio_amd", "csrc", "sketches.hpp")
    for name in ENTRIES:
        assert name in bound and len(bound[name][1]) == ARITY[name] and bound[name][0] is C.c_int, name
        assert f"C.{name}(" in go, name
        assert name + "(" in hpp, name
    assert bound["bsk_index_build_counted"][1] == bound["bsk_index_build"][1] and bound["bsk_index_search_counted"][1] == bound["bsk_index_search"][1]
    fn = bound["bsk_index_fetch_norms"][1]
    assert fn[2] is C.c_uint64 and fn[3] is C.c_uint64
    for m in ("func (s *Sets) BuildIndexCounted() (*Index, error)", "func (ix *Index) Counted() bool", "func (ix *Index) Norms(first, count uint64) (sumsq, totals []uint64, err error)",
              "func (ix *Index) SearchCounted(q *Sets, p SearchParams, into *Hits) (*Hits, error)"):
        assert m in go, m
    for m in ("int build_counted(Engine &e, const DeviceSets &targets)", "bool counted() const", "int fetch_norms(Engine &e, std::vector<uint64_t> &sumsq, std::vector<uint64_t> &totals) const",
              "int search_counted(Engine &e, const DeviceSets &queries, const bsk_search_params &sp, SearchHits &into) const"):
        assert m in hpp, m
    from bio_amd import sketches as S
    sig, plain = inspect.signature(S.Index.search_counted).parameters, inspect.signature(S.Index.search).parameters
    assert list(sig) == ["self", "queries", "min_shared", "min_query_cov", "min_target_cov", "reuse"] == list(plain)
    assert [sig[k].default for k in list(sig)[2:]] == [1, 0.0, 0.0, None] == [plain[k].default for k in list(plain)[2:]]
    assert list(inspect.signature(S.Sets.index).parameters) == ["self"] == list(inspect.signature(S.Sets.index_counted).parameters)
    assert isinstance(S.Index.counted, property) and callable(S.Index.norms) and callable(S.Hits.weighted_containment)
    assert S.Hits._plain_targets is None  # class-level default: hits of any other origin


def test_the_kernels_live_where_the_build_expects_them():
    mk = _read("bio_amd", "csrc", "Makefile")
    assert re.search(r"^test_search_counted:.*tests/cpp/test_search_counted\.cpp.*sketches\.hpp.*libbiosketch\.so", mk, re.M)
    assert re.search(r"^\trm -f .*\btest_search_counted\b", mk, re.M)
    assert '"test_search_counted"' in _read("__graft_entry__.py")
    assert "bio_amd/csrc/test_search_counted" in _read(".gitignore").split()
    src = _read("bio_amd", "csrc", "search.hip")
    code = re.sub(r"//.*", "", src)
    for k in KERNELS:
        assert f"void {k}(" in code, k
    assert "->cus" not in code and "asm" not in code
    assert len(re.findall(r"rocprim::radix_sort_pairs\(", code)) == 2 and "radix_sort_pairs<" not in code  # the one instantiation, its size query and its run
    # every launch of the new kernels goes through grid_for
    for k in KERNELS:
        launches = re.findall(r"hipLaunchKernelGGL\(%s, dim3\(([^;]*?)\), dim3\(" % k, code)
        assert launches and all(x.startswith("grid_for(ctx, ") for x in launches), (k, launches)
    # the search itself is run as it is: one implementation, and the payload pass adds no fourth place that clears the totals
    assert code.count("static int search_impl(") == 2 and code.count("search_impl(ctx, ix, queries, sp, res)") == 1 and code.count("static int weights_impl(") == 2
    assert len(re.findall(r"res->has_total = false;", src)) == 3 and len(re.findall(r"res->has_weights = true;", src)) == 1
    types = _read("bio_amd", "csrc", "host_types.hpp")
    slots = {k: int(v) for k, v in re.findall(r"\b(SLOT_\w+|POOL_SLOTS) = (\d+)", types)}
    mine = [slots["SLOT_SW_QUERY"], slots["SLOT_SW_FLAGS"]]
    assert len(set(mine)) == 2 and all(v < slots["POOL_SLOTS"] for v in mine)
    assert not [k for k, v in slots.items() if v in mine and not k.startswith("SLOT_SW_")]  # shared with nobody
    assert "SLOT_SW_QUERY" in src and "SLOT_SW_FLAGS" in src
    caps = W.read_caps()
    assert {"SW_ROW", "SW_WAVES", "SW_CHUNK"} <= set(caps) and caps["SW_ROW"] * 20 * caps["SW_WAVES"] <= 64 * 1024  # the rows of a workgroup: 20 bytes a hit


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
    assert not [s for s in re.findall(r" [TW] (\S*(?:weights_impl|search_entry|_ZL?\d*index_build|k_sw_|k_ix_|SwRow|sets_totals_device|sets_sumsq_device)\S*)", out)]  # the helpers stay inside
    declared = set(re.findall(r"\b(bsk_\w+)\(", _norm(_read("include", "biosketch.h"))))
    assert exported <= declared, exported - declared


def test_null_and_bad_arguments_without_a_device(lib):
    from bio_amd import _lib as L
    fake = C.create_string_buffer(1024)  # zeroed: an object of no context and nothing in it -- every case below fails its checks first
    fp = C.addressof(fake)
    out = C.c_void_p(1234)
    assert lib.bsk_index_build_counted(None, None, C.byref(out)) == L.ERR_ARG and out.value is None  # only writes its slot: NULL on every error
    out = C.c_void_p(1234)
    assert lib.bsk_index_build_counted(None, fp, C.byref(out)) == L.ERR_ARG and out.value is None
    assert lib.bsk_index_build_counted(None, fp, None) == L.ERR_ARG
    k = C.c_int(7)
    assert lib.bsk_index_counted(None, C.byref(k)) == L.ERR_ARG and k.value == 7 and lib.bsk_index_counted(fp, None) == L.ERR_ARG
    assert lib.bsk_index_counted(fp, C.byref(k)) == L.OK and k.value == 0  # a zeroed index keeps no counts
    nn = np.full(4, 7, np.uint64)
    assert lib.bsk_index_fetch_norms(None, fp, 0, 0, nn.ctypes.data, nn.ctypes.data) == L.ERR_ARG
    assert lib.bsk_index_fetch_norms(None, None, 0, 0, None, None) == L.ERR_ARG and list(nn) == [7] * 4
    hits = C.c_void_p(4321)
    sp = L.SearchParams(1, 0, 0.0, 0.0)
    for ix, q in ((None, None), (fp, None), (None, fp), (fp, fp)):
        assert lib.bsk_index_search_counted(None, ix, q, C.byref(sp), C.byref(hits)) == L.ERR_ARG and hits.value == 4321  # an argument error leaves *hits
    assert lib.bsk_index_search_counted(None, fp, fp, None, C.byref(hits)) == L.ERR_ARG and lib.bsk_index_search_counted(None, fp, fp, C.byref(sp), None) == L.ERR_ARG


def test_the_order_of_the_checks():
    """null, foreign context, reserved, covers, the 2^32 limits, all before the slot is taken, under the entry's own name -- read from the
    source, where one helper serves bsk_index_search and bsk_index_search_counted; and the build's, and the norms'"""
    src = _read("bio_amd", "csrc", "search.hip")
    body = src[src.index("static int search_entry("):src.index("struct SearchCarve {")]
    at = [body.index(x) for x in ("null argument", "belong to another context", "reserved != 0", "a cover outside 0..1", "2^32 query sets or query values", "take_over(",
                                  "search_impl(ctx, ix, queries, sp, res)", "weights_impl(ctx, ix, queries, res)")]
    assert at == sorted(at)
    said = re.findall(r'weighted \? "bsk_index_search_counted: ([^"]*)"\s*: "bsk_index_search: ([^"]*)"', body)
    assert len(said) == 5 and all(x == y for x, y in said)
    assert "return search_entry(ctx, ix, queries, sp, hits, true);" in body and "return search_entry(ctx, ix, queries, sp, hits, false);" in body
    build = src[src.index("static int index_build("):src.index('extern "C" int bsk_index_counted(')]
    at = [build.index(x) for x in ("if (out) *out = nullptr;", "null argument", "belong to another context", "2^32 targets or postings", "hipSetDevice", "k_ix_gather", "*out = hold.release();")]
    assert at == sorted(at)
    said = re.findall(r'keep_counts \? "bsk_index_build_counted: ([^"]*)" : "bsk_index_build: ([^"]*)"', build)
    assert len(said) == 3 and all(x == y for x, y in said)
    assert "const bool counted = keep_counts && targets->counted;" in build  # uncounted sets: an index without counts from either entry
    norms = src[src.index('extern "C" int bsk_index_fetch_norms('):src.index("// bsk_index_search and bsk_index_search_counted")]
    at = [norms.index(x) for x in ("null argument", "another context", "range outside the targets", "hipSetDevice")]
    assert at == sorted(at)
    attach = src[src.index('extern "C" int bsk_index_attach('):src.index("static int index_build(")]
    for arr in ("post_cnt", "tsumsq", "ttotal"):
        assert f"hipMemcpyPeer(d->{arr}, d->device, src->{arr}, src->device" in attach and f"hipFree(a->{arr})" in src, arr


class Fixed:
    """Hits with arrays put in by hand (no device)"""

    @staticmethod
    def make(offsets, target, shared, dot, ms, norms, plain_targets):
        from bio_amd import sketches as S

        class _Fixed(S.Hits):
            def __init__(self):
                self.eng, self.h = None, None
                self._host = (np.array(offsets, np.uint64), np.array(target, np.uint32), np.array(shared, np.uint32))
                if dot is not None:
                    self._weights = (np.array(dot, np.uint64), np.array(ms, np.uint64))
                self._norms = None if norms is None else tuple(np.array(x, np.uint64) for x in norms)
                self._plain_targets = plain_targets

        return _Fixed()


def test_weighted_containment_arithmetic():
    """dot / totals_q per hit against an index without counts; NaN for a saturated dot, 0.0 for an empty query's total; refused for a
    counted index, for hits of another origin and for hits without weights"""
    norms = ([30, 0, 9], [3, 2, 5], [10, 0, 1 << 40], [3, 2, 5])  # sumsq_q, sumsq_t (= sizes), totals_q, totals_t (= sizes)
    h = Fixed.make([0, 2, 3, 5], [0, 2, 1, 0, 1], [2, 1, 1, 3, 1], [7, 10, 0, W.MAX, 1 << 39], [2, 1, 0, 3, 1], norms, True)
    wc = h.weighted_containment()
    assert wc.dtype == np.float64 and wc[:3].tolist() == [0.7, 1.0, 0.0] and np.isnan(wc[3]) and wc[4] == 0.5
    assert h.cosine()[0] == 7 / (np.sqrt(30.0) * np.sqrt(3.0)) and h.bray_curtis()[0] == 1 - 4 / 13  # the other formulas read the same bound norms
    with pytest.raises(ValueError):
        Fixed.make([0, 1], [0], [1], [4], [1], norms, False).weighted_containment()  # a counted index: dot is a product
    with pytest.raises(ValueError):
        Fixed.make([0, 1], [0], [1], [4], [1], norms, None).weighted_containment()  # Sets.neighbors_counted and the like
    with pytest.raises(ValueError):
        Fixed.make([0, 1], [0], [1], None, None, norms, True).weighted_containment()  # no weights
