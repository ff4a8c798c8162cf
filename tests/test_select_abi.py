"""CPU: the entries that select hits by a measure (bsk_hits_filter, bsk_hits_top_by) -- declared with the contract's prototypes between the
folded hits and the clusters block, bound by bio_amd._lib, called from the Go shim and the C++ owners, exported by the library and nothing
else with them, built where the build expects them, and their argument checks as far as they run without a device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "bsk_hits_filter": "int bsk_hits_filter(bsk_ctx *ctx, const bsk_hits *h, const bsk_measure *m, const bsk_filter_params *fp, bsk_hits **out);",
    "bsk_hits_top_by": "int bsk_hits_top_by(bsk_ctx *ctx, const bsk_hits *h, const bsk_measure *m, uint32_t n, bsk_hits **top);",
}
ARITY = dict(bsk_hits_filter=5, bsk_hits_top_by=5)
KINDS = ("SHARED", "MEMBERS", "DOT", "MIN_SUM", "QUERY_COV", "TARGET_COV", "JACCARD", "COSINE", "WEIGHTED_JACCARD", "BC_SIMILARITY", "QUERY_MASS")
KERNELS = ("k_sel_check", "k_sel_place", "k_sel_offsets", "k_tb_classes", "k_tb_group", "k_tb_lds", "k_tb_global")


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


def _norm(s):
    s = re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    return re.sub(r"\s+", " ", s).replace("( ", "(").replace(" )", ")").replace(" ;", ";").replace(" ,", ",").strip()


def test_header_declares_the_entries_in_their_place():
    raw = _read("include", "biosketch.h")
    hdr = _norm(raw)
    for name, proto in ENTRIES.items():
        assert _norm(proto) in hdr, name
    assert _norm("enum { " + ", ".join("BSK_MEASURE_" + k + (" = 0" if k == "SHARED" else "") for k in KINDS) + " };") in hdr and "#define BSK_ABI_VERSION 1" in hdr
    assert _norm("typedef struct bsk_measure { uint32_t kind, flags; const uint64_t *qnorm; uint64_t n_qnorm; const uint64_t *tnorm; uint64_t n_tnorm; } bsk_measure;") in hdr
    assert _norm("typedef struct bsk_filter_params { uint64_t min_num, min_den; } bsk_filter_params;") in hdr
    order = ["int bsk_hits_fetch_members(", "enum { BSK_MEASURE_SHARED", "typedef struct bsk_measure", "typedef struct bsk_filter_params", "int bsk_hits_filter(",
             "int bsk_hits_top_by(", "enum { BSK_CLUSTER_COMPONENTS", "enum { BSK_NEIGHBORS_UPPER", "int bsk_hits_fetch_totals("]
    at = [hdr.index(x) for x in order]
    assert at == sorted(at)
    a, b = raw.index("/* ---- hits selected by a measure"), raw.index("/* ---- clusters of a neighbour graph")
    assert raw.index("/* ---- window sets and folded hits") < a < b < raw.index("/* ---- sparse all-pairs comparison")  # the neighbours block still closes the header
    block = raw[a:b]
    for said in ("exact fraction N/D", "Q = qnorm[q] and T = tnorm[t]", "total[i] where h has totals, else Q + T - shared", "N = dot * dot", "D = Q * T", "Q + T - min_sum",
                 "N = 2 * min_sum", "squared cosine", "1 - Bray-Curtis", "2^64-1", "more than 64 bits", "256 bits", "wide_uint.hpp", "no rounding", "not retained",
                 "keep the slot", "unknown kind", "flag bit", "n_qnorm != n_queries", "*out == h", "another context", "k_sel_check", "before the object is taken over",
                 "target >= n_tnorm", "D <= 0", "BSK_ERR_UNSUPPORTED", "release it", "need not have ascending rows", "N * min_den >= min_num * D",
                 "N * min_den^2 >= min_num^2 * D", "min_den == 0", "Rows keep their order", "k_sel_offsets", "k_sel_place", "No atomics on the output", "bit-identical",
                 "kept=", "N_a * D_b > N_b * D_a", "ascending target", "best first", "n == 0", "bit-identical to", "bsk_hits_top(h, n)", "k_tb_group", "k_tb_lds", "k_tb_global",
                 "__syncthreads()", "filter first", "n_large_queries is the count of the global path", "still drops the payloads"):
        assert said in block, said
    slot = raw[raw.index("/* The result slot."):raw.index("int bsk_result_sets_reuse(")]
    assert "bsk_hits_filter" in slot and "bsk_hits_top_by" in slot


def test_python_binds_go_and_cpp_call_them():
    from bio_amd import _lib
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    go = _read("bindings", "go", "sketches", "select.go")
    hpp = _read("bio_amd", "csrc", "sketches.hpp")
    for name in ENTRIES:
        assert name in bound and len(bound[name][1]) == ARITY[name] and bound[name][0] is C.c_int, name
        assert f"C.{name}(" in go, name
        assert name + "(" in hpp, name
    assert [f for f, _ in _lib.Measure._fields_] == ["kind", "flags", "qnorm", "n_qnorm", "tnorm", "n_tnorm"] and C.sizeof(_lib.Measure) == 40
    assert [(f, t) for f, t in _lib.FilterParams._fields_] == [("min_num", C.c_uint64), ("min_den", C.c_uint64)] and C.sizeof(_lib.FilterParams) == 16
    assert bound["bsk_hits_top_by"][1][3] is C.c_uint32
    assert [getattr(_lib, "MEASURE_" + k) for k in KINDS] == list(range(11))
    for m in ("type Measure struct", "func (h *Hits) Filter(m Measure, minNum, minDen uint64, reuse *Hits) (*Hits, error)",
              "func (h *Hits) TopBy(m Measure, n uint32, reuse *Hits) (*Hits, error)", "C.BSK_MEASURE_COSINE", "C.BSK_MEASURE_QUERY_MASS"):
        assert m in go, m
    for m in ("int filter(Engine &e, const bsk_measure &m, uint64_t min_num, uint64_t min_den", "int top_by(Engine &e, const bsk_measure &m, uint32_t n"):
        assert m in hpp, m
    from bio_amd import sketches as S
    sig = inspect.signature(S.Hits.filter).parameters
    assert list(sig) == ["self", "measure", "at_least", "qnorm", "tnorm", "reuse"] and all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY and sig[k].default is None
                                                                                          for k in ("qnorm", "tnorm", "reuse"))
    sig = inspect.signature(S.Hits.top_by).parameters
    assert list(sig) == ["self", "n", "measure", "qnorm", "tnorm", "reuse"] and all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("qnorm", "tnorm", "reuse"))
    assert sorted(S.Hits._MEASURES) == sorted(["shared", "members", "dot", "min_sum", "query_cov", "target_cov", "jaccard", "cosine", "weighted_jaccard",
                                               "bray_curtis_similarity", "weighted_containment"])
    assert sorted(v[0] for v in S.Hits._MEASURES.values()) == list(range(11))


def test_the_threshold_is_taken_exactly():
    from fractions import Fraction
    from bio_amd import sketches as S
    f = S.Hits._at_least
    assert f(3) == (3, 1) and f(Fraction(9, 10)) == (9, 10) and f((7, 8)) == (7, 8) and f(0.5) == (1, 2) and f(np.uint32(4)) == (4, 1)
    assert f(0.9) == (0.9).as_integer_ratio() and Fraction(*f(0.9)) != Fraction(9, 10)  # the float itself, not the decimal it was written as
    assert f(-1) == (0, 1) and f((2**64 - 1, 2**64 - 1)) == (2**64 - 1, 2**64 - 1)
    for bad in (Fraction(2**64, 3), (1, 2**64), 1e-30, float("nan"), float("inf"), (1, 0)):
        with pytest.raises(ValueError):
            f(bad)


def test_the_kernels_live_where_the_build_expects_them():
    mk = _read("bio_amd", "csrc", "Makefile")
    assert re.search(r"^OBJS =.*\bselect\.o\b", mk, re.M) and re.search(r"^HDRS =(.|\\\n)*\bwide_uint\.hpp\b", mk, re.M)
    assert re.search(r"select\.o:.*sets_internal\.hpp.*search_internal\.hpp.*wide_uint\.hpp", mk)
    assert re.search(r"^test_select:.*tests/cpp/test_select\.cpp.*sketches\.hpp.*libbiosketch\.so", mk, re.M) and re.search(r"^\trm -f .*\btest_select\b", mk, re.M)
    assert '"test_select"' in _read("__graft_entry__.py")
    assert "bio_amd/csrc/test_select" in _read(".gitignore").split()
    src = _read("bio_amd", "csrc", "select.hip")
    for k in KERNELS:
        assert f"void {k}(" in src, k
    code = re.sub(r"//.*", "", src)
    assert "scan_counts(" in code and "rocprim" not in code and "asm" not in code and "->cus" not in code  # the library's scan, no new instantiation, grids through the helper
    for banned in ("atomicCAS", "atomicExch", "while (", "__threadfence", "volatile", "double", "float", "hipMalloc", "<<<"):
        assert banned not in code, banned  # bounded loops, integers, pooled memory, no retry and no wait on another workgroup
    assert len(re.findall(r"hipLaunchKernelGGL\(", code)) == len(re.findall(r"hipLaunchKernelGGL\([^;]*?(?:grid_for|sel_grid)\(ctx", code))  # every grid is capped
    wide = re.sub(r"//.*", "", _read("bio_amd", "csrc", "wide_uint.hpp"))
    assert "unsigned __int128" in wide and "w[4]" in wide and "double" not in wide and "float" not in wide and "hip_runtime" not in wide  # the host compiler takes it too
    # search.hip, fold.hip and cluster.hip know nothing of the selection; bsk_hits_top still drops the payloads
    for fn in ("search.hip", "fold.hip", "cluster.hip"):
        assert "bsk_hits_filter" not in _read("bio_amd", "csrc", fn) and "top_by" not in _read("bio_amd", "csrc", fn)
    assert "res->has_total = false;  // the n best carry no totals" in _read("bio_amd", "csrc", "search.hip")
    slots = {k: int(v) for k, v in re.findall(r"\b(SLOT_\w+|POOL_SLOTS) = (\d+)", _read("bio_amd", "csrc", "host_types.hpp"))}
    mine = [slots[k] for k in ("SLOT_SELECT_WORK", "SLOT_SELECT_NORMS", "SLOT_SELECT_INDEX")]
    assert len(set(mine)) == 3 and all(v < slots["POOL_SLOTS"] for v in mine)
    assert not [k for k, v in slots.items() if v in mine and not k.startswith("SLOT_SELECT_")]  # shared with nobody


def test_the_checks_come_in_the_contracts_order():
    """without a context the argument checks cannot be told apart, so their order is read from the source: nothing touches the device before
    them, and the pass that refuses a target beyond the norms and a denominator that is not positive runs before the slot is taken over"""
    src = _read("bio_amd", "csrc", "select.hip")
    args = src[src.index("int sel_check_args("):src.index("struct SelScratch")]
    at = [args.index(x) for x in ("null argument", "unknown measure", "unknown flag", "another context", "holds h itself", "needs hits with members", "needs hits with weights",
                                  "needs qnorm", "needs tnorm", "n_qnorm != n_queries", "BSK_ERR_UNSUPPORTED")]
    assert at == sorted(at) and "hip" not in args
    body = src[src.index('extern "C" int bsk_hits_filter('):src.index('extern "C" int bsk_hits_top_by(')]
    at = [body.index(x) for x in ("sel_check_args(", "min_den == 0", "hipSetDevice", "sel_prepare(", "k_sel_check<true>", "scan_counts(", "read_back(", "sel_refuse(", "take_over(")]
    assert at == sorted(at)
    body = src[src.index('extern "C" int bsk_hits_top_by('):]
    at = [body.index(x) for x in ("sel_check_args(", "n == 0", "hipSetDevice", "sel_prepare(", "k_sel_check<false>", "read_back(", "sel_refuse(", "take_over(")]
    assert at == sorted(at)


@pytest.fixture(scope="module")
def lib():
    from bio_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_library_exports_them_and_nothing_else(lib):
    from bio_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (bsk_\w+)", out))
    assert set(ENTRIES) <= exported
    hidden = "|".join(KERNELS + ("filter_impl", "top_by_impl", "sel_prepare", "sel_check_args", "SelScratch", "SelMeasure", "SelRule", "wide_mul", "wide_cmp", "tb_sort"))
    assert not re.findall(r" [TW] (\S*(?:%s)\S*)" % hidden, out)  # the helpers stay inside the library
    declared = set(re.findall(r"\b(bsk_\w+)\(", _norm(_read("include", "biosketch.h"))))
    assert exported <= declared, exported - declared  # the header's entries and no more
    assert {s for s in exported if "filter" in s and "counts" not in s or "top_by" in s} == set(ENTRIES)


def test_null_and_bad_arguments_without_a_device(lib):
    from bio_amd import _lib as L
    fake = C.create_string_buffer(2048)  # zeroed: hits of no context and nothing in them -- every case below fails its checks first
    fp = C.addressof(fake)
    out = C.c_void_p(4321)
    norms = np.full(4, 7, np.uint64)
    m = L.Measure(L.MEASURE_SHARED, 0, None, 0, None, 0)
    rule, rule0 = L.FilterParams(1, 2), L.FilterParams(1, 0)
    for ctx, h, mm in ((None, None, m), (None, fp, m), (None, fp, None)):
        ref = C.byref(mm) if mm is not None else None
        assert lib.bsk_hits_filter(ctx, h, ref, C.byref(rule), C.byref(out)) == L.ERR_ARG and out.value == 4321
        assert lib.bsk_hits_top_by(ctx, h, ref, 3, C.byref(out)) == L.ERR_ARG and out.value == 4321
    assert lib.bsk_hits_filter(None, fp, C.byref(m), None, C.byref(out)) == L.ERR_ARG and out.value == 4321
    assert lib.bsk_hits_filter(None, fp, C.byref(m), C.byref(rule), None) == L.ERR_ARG and lib.bsk_hits_top_by(None, fp, C.byref(m), 3, None) == L.ERR_ARG
    for bad in (L.Measure(11, 0, None, 0, None, 0), L.Measure(0xFFFFFFFF, 0, None, 0, None, 0), L.Measure(L.MEASURE_SHARED, 1, None, 0, None, 0),
                L.Measure(L.MEASURE_COSINE, 0, norms.ctypes.data, 4, norms.ctypes.data, 4), L.Measure(L.MEASURE_QUERY_COV, 0, None, 0, None, 0)):
        assert lib.bsk_hits_filter(None, fp, C.byref(bad), C.byref(rule), C.byref(out)) == L.ERR_ARG and out.value == 4321
        assert lib.bsk_hits_top_by(None, fp, C.byref(bad), 3, C.byref(out)) == L.ERR_ARG and out.value == 4321
    assert lib.bsk_hits_filter(None, fp, C.byref(m), C.byref(rule0), C.byref(out)) == L.ERR_ARG and out.value == 4321
    assert lib.bsk_hits_top_by(None, fp, C.byref(m), 0, C.byref(out)) == L.ERR_ARG and out.value == 4321
    assert list(norms) == [7] * 4
