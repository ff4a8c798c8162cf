"""CPU: the containment-search entries of include/biosketch.h -- declared with the contract's signatures, bound by bio_amd._lib, called
from the Go shim -- and their argument checks, as far as they run without a device."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "bsk_sets_from_host": "int bsk_sets_from_host(bsk_ctx *ctx, const uint64_t *offsets, uint64_t n_sets, const uint64_t *values, bsk_sets **out);",
    "bsk_index_build": "int bsk_index_build(bsk_ctx *ctx, const bsk_sets *targets, bsk_index **out);",
    "bsk_index_info": "int bsk_index_info(const bsk_index *ix, uint64_t *n_targets, uint64_t *n_postings, uint64_t *n_distinct, uint64_t *max_bucket, "
                      "uint64_t *device_bytes);",
    "bsk_index_release": "void bsk_index_release(bsk_index *ix);",
    "bsk_index_search": "int bsk_index_search(bsk_ctx *ctx, const bsk_index *ix, const bsk_sets *queries, const bsk_search_params *sp, bsk_hits **hits);",
    "bsk_hits_info": "int bsk_hits_info(const bsk_hits *h, uint64_t *n_queries, uint64_t *n_hits);",
    "bsk_hits_plan": "int bsk_hits_plan(const bsk_hits *h, const char **plan, uint64_t *n_large_queries);",
    "bsk_hits_fetch": "int bsk_hits_fetch(bsk_ctx *ctx, const bsk_hits *h, uint64_t first, uint64_t count, uint64_t *offsets, uint32_t *target, "
                      "uint32_t *shared, uint64_t hit_cap);",
    "bsk_hits_device": "int bsk_hits_device(const bsk_hits *h, const uint64_t **offsets, const uint32_t **target, const uint32_t **shared);",
    "bsk_hits_release": "void bsk_hits_release(bsk_hits *h);",
}


def _norm(s):
    s = re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    return re.sub(r"\s+", " ", s).replace("( ", "(").replace(" )", ")").replace(" ;", ";").replace(" ,", ",").strip()


def _header():
    return _norm(open(os.path.join(ROOT, "include", "biosketch.h")).read())


def test_header_declares_the_search_entries():
    hdr = _header()
    for name, proto in ENTRIES.items():
        assert _norm(proto) in hdr, name
    body = re.search(r"typedef struct bsk_search_params \{(.*?)\} bsk_search_params;", hdr).group(1)
    assert re.findall(r"(\w+) (\w+);", body) == [("uint32_t", "min_shared"), ("uint32_t", "reserved"), ("double", "min_query_cov"),
                                                 ("double", "min_target_cov")]
    assert "#define BSK_ABI_VERSION 1" in hdr


def test_python_binds_and_go_calls_them():
    from bio_amd import _lib
    bound = {n for n, _, _ in _lib.SYMBOLS}
    go = "".join(open(f).read() for f in glob.glob(os.path.join(ROOT, "bindings", "go", "sketches", "*.go")))
    for name in ENTRIES:
        assert name in bound, name
        assert f"C.{name}(" in go, name
    assert C.sizeof(_lib.SearchParams) == 24
    from bio_amd import sketches as S
    for cls, attrs in ((S.Sets, ("index", "fetch", "device", "info")), (S.Index, ("search", "info")),
                       (S.Hits, ("offsets", "target", "shared", "containment", "jaccard", "plan")),
                       (S.BatchResult, ("device_sets",)), (S.Engine, ("sets_from_arrays",))):
        for a in attrs:
            assert hasattr(cls, a), (cls, a)


@pytest.fixture(scope="module")
def lib():
    from bio_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_null_and_bad_arguments_without_a_context(lib):
    from bio_amd import _lib as L
    out = C.c_void_p(1234)
    assert lib.bsk_index_build(None, None, C.byref(out)) == L.ERR_ARG and out.value is None
    lib.bsk_hits_release(None)
    lib.bsk_index_release(None)
    offs = np.array([0, 2], np.uint64)
    for vals in (np.array([5, 3], np.uint64), np.array([5, 5], np.uint64), np.array([3, 5], np.uint64)):
        out = C.c_void_p()
        assert lib.bsk_sets_from_host(None, offs.ctypes.data, 1, vals.ctypes.data, C.byref(out)) == L.ERR_ARG and not out.value
    assert lib.bsk_sets_from_host(None, None, 0, None, C.byref(out)) == L.ERR_ARG
    sp = L.SearchParams(1, 0, 0.0, 0.0)
    hits = C.c_void_p()
    assert lib.bsk_index_search(None, None, None, C.byref(sp), C.byref(hits)) == L.ERR_ARG and not hits.value
    assert lib.bsk_index_search(None, None, None, None, None) == L.ERR_ARG
    u = C.c_uint64()
    assert lib.bsk_index_info(None, C.byref(u), None, None, None, None) == L.ERR_ARG
    assert lib.bsk_hits_info(None, C.byref(u), C.byref(u)) == L.ERR_ARG
    assert lib.bsk_hits_plan(None, None, C.byref(u)) == L.ERR_ARG
    assert lib.bsk_hits_device(None, None, None, None) == L.ERR_ARG
    o = np.zeros(2, np.uint64)
    assert lib.bsk_hits_fetch(None, None, 0, 1, o.ctypes.data, None, None, 0) == L.ERR_ARG
