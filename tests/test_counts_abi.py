"""CPU: the counted-sets entries of include/biosketch.h -- declared with the contract's prototypes, bound by bio_amd._lib, called from the
Go shim and the C++ owners, exported by the library, and their argument checks as far as they run without a device."""
import ctypes as C
import glob
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "bsk_result_sets_counted": "int bsk_result_sets_counted(bsk_ctx *ctx, const bsk_result *r, int scope, int scale, bsk_sets **sets);",
    "bsk_sets_counts_device": "int bsk_sets_counts_device(const bsk_sets *s, const uint32_t **counts);",
    "bsk_sets_fetch_counts": "int bsk_sets_fetch_counts(bsk_ctx *ctx, const bsk_sets *s, uint64_t first, uint64_t count, uint32_t *counts, uint64_t count_cap);",
    "bsk_sets_from_host_counted": "int bsk_sets_from_host_counted(bsk_ctx *ctx, const uint64_t *offsets, uint64_t n_sets, const uint64_t *values, "
                                  "const uint32_t *counts, bsk_sets **out);",
    "bsk_sets_op_counted": "int bsk_sets_op_counted(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, int op, bsk_sets **out);",
    "bsk_sets_filter_counts": "int bsk_sets_filter_counts(bsk_ctx *ctx, const bsk_sets *s, uint32_t min_count, uint32_t max_count, bsk_sets **out);",
    "bsk_sets_totals": "int bsk_sets_totals(bsk_ctx *ctx, const bsk_sets *s, uint64_t first, uint64_t count, uint64_t *totals);",
}
ARITY = dict(bsk_result_sets_counted=5, bsk_sets_counts_device=2, bsk_sets_fetch_counts=6, bsk_sets_from_host_counted=6, bsk_sets_op_counted=5,
             bsk_sets_filter_counts=5, bsk_sets_totals=5)


def _norm(s):
    s = re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    return re.sub(r"\s+", " ", s).replace("( ", "(").replace(" )", ")").replace(" ;", ";").replace(" ,", ",").strip()


def test_header_declares_the_entries():
    hdr = _norm(open(os.path.join(ROOT, "include", "biosketch.h")).read())
    for name, proto in ENTRIES.items():
        assert _norm(proto) in hdr, name
    assert "enum { BSK_COUNTOP_ADD = 0, BSK_COUNTOP_KEEP = 1, BSK_COUNTOP_DROP = 2 };" in hdr
    assert "#define BSK_ABI_VERSION 1" in hdr
    # the block follows the classify block and closes the header
    assert hdr.index("int bsk_chunk_hits(") < hdr.index("int bsk_result_sets_counted(") < hdr.index("int bsk_sets_totals(") < hdr.rindex("#ifdef __cplusplus")


def test_python_binds_go_and_cpp_call_them():
    from bio_amd import _lib
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    go = open(os.path.join(ROOT, "bindings", "go", "sketches", "counts.go")).read()
    hpp = open(os.path.join(ROOT, "bio_amd", "csrc", "sketches.hpp")).read()
    for name in ENTRIES:
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == ARITY[name], name
        assert f"C.{name}(" in go, name
        assert name + "(" in hpp, name
    assert bound["bsk_sets_filter_counts"][1][2] is C.c_uint32 and bound["bsk_sets_filter_counts"][1][3] is C.c_uint32
    assert bound["bsk_sets_fetch_counts"][1][2] is C.c_uint64 and bound["bsk_sets_totals"][1][3] is C.c_uint64 and bound["bsk_sets_op_counted"][1][3] is C.c_int
    assert (_lib.COUNTOP_ADD, _lib.COUNTOP_KEEP, _lib.COUNTOP_DROP) == (0, 1, 2)
    for m in ("CountedSets(", "func (s *Sets) Counts(", "func (a *Sets) OpCounted(", "func (s *Sets) FilterCounts(", "func (s *Sets) Totals(",
              "func (e *Engine) SetsFromHostCounted("):
        assert m in go, m
    for m in ("from_result_counted", "from_host_counted", "fetch_counts", "op_counted", "filter_counts", "totals", "counted"):
        assert re.search(r"\b%s\(" % m, hpp), m
    from bio_amd import sketches as S
    sig = inspect.signature(S.BatchResult.counted_sets).parameters
    assert list(sig) == ["self", "whole_batch", "scale", "into"] and sig["whole_batch"].default is False and sig["scale"].default == 1 and sig["into"].default is None
    assert isinstance(S.Sets.counted, property) and list(inspect.signature(S.Sets.fetch_counts).parameters) == ["self"]
    for a in ("add", "keep", "drop"):
        assert list(inspect.signature(getattr(S.Sets, a)).parameters) == ["self", "other", "into"]
    sig = inspect.signature(S.Sets.filter_counts).parameters
    assert list(sig) == ["self", "min_count", "max_count", "into"] and sig["min_count"].default == 1 and sig["max_count"].default is None
    assert list(inspect.signature(S.Sets.totals).parameters) == ["self"]
    assert list(inspect.signature(S.Engine.sets_from_arrays_counted).parameters) == ["self", "offsets", "values", "counts"]


def test_the_kernels_live_where_the_build_expects_them():
    mk = open(os.path.join(ROOT, "bio_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS =.*\bcounts\.o\b", mk, re.M) and re.search(r"counts\.o:.*sets_internal\.hpp", mk) and re.search(r"^test_counts:", mk, re.M)
    assert '"test_counts"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    for fn in glob.glob(os.path.join(ROOT, "bio_amd", "csrc", "kernels_*.hpp")):
        assert "COUNT" not in "".join(re.findall(r"#define (BSK_\w+)\(X\)", open(fn).read())), fn  # no new kernel list: the plan atlas stays as it is


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
    assert not [s for s in re.findall(r" [TW] (\S*sets_(?:run_counts|grow_counts|build)\S*)", out)]  # the helpers stay inside the library


def test_null_and_bad_arguments_without_a_device(lib):
    from bio_amd import _lib as L
    fake = C.create_string_buffer(1024)  # zeroed: a bsk_sets of no context, no values, not counted -- every case below fails its checks first
    fp = C.addressof(fake)
    out = C.c_void_p(1234)
    for a, b in ((None, None), (fp, None), (None, fp), (fp, fp)):
        assert lib.bsk_sets_op_counted(None, a, b, L.COUNTOP_ADD, C.byref(out)) == L.ERR_ARG and out.value == 1234  # an argument error leaves *out
    assert lib.bsk_sets_op_counted(None, None, None, 99, None) == L.ERR_ARG
    for s, lo, hi in ((None, 1, 2), (fp, 1, 2), (fp, 0, 2), (fp, 3, 2)):
        assert lib.bsk_sets_filter_counts(None, s, lo, hi, C.byref(out)) == L.ERR_ARG and out.value == 1234
    assert lib.bsk_sets_filter_counts(None, None, 1, 2, None) == L.ERR_ARG
    assert lib.bsk_result_sets_counted(None, None, 0, 1, None) == L.ERR_ARG
    cnt, tot = np.full(4, 7, np.uint32), np.full(4, 7, np.uint64)
    assert lib.bsk_sets_fetch_counts(None, fp, 0, 0, cnt.ctypes.data, 4) == L.ERR_ARG and lib.bsk_sets_fetch_counts(None, None, 0, 0, None, 0) == L.ERR_ARG
    assert lib.bsk_sets_totals(None, fp, 0, 0, tot.ctypes.data) == L.ERR_ARG and lib.bsk_sets_totals(None, None, 0, 0, None) == L.ERR_ARG
    assert list(cnt) == [7] * 4 and list(tot) == [7] * 4
    p = C.c_void_p(99)
    assert lib.bsk_sets_counts_device(None, C.byref(p)) == L.ERR_ARG and p.value == 99 and lib.bsk_sets_counts_device(fp, None) == L.ERR_ARG
    assert lib.bsk_sets_counts_device(fp, C.byref(p)) == L.OK and p.value is None  # an uncounted object: NULL
    offs = np.array([0, 1], np.uint64)
    assert lib.bsk_sets_from_host_counted(None, offs.ctypes.data, 1, None, None, None) == L.ERR_ARG
    h = C.c_void_p(5)
    assert lib.bsk_sets_from_host_counted(None, None, 1, None, None, C.byref(h)) == L.ERR_ARG and h.value is None  # (bsk_sets_from_host's rule)
