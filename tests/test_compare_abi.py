"""CPU: the MinHash entries of include/biosketch.h (bsk_sets_bottom, bsk_sets_compare and the bsk_compare object) -- declared with the
contract's prototypes, bound by bio_amd._lib, called from the Go shim and the C++ owners, exported by the library, and their argument
checks as far as they run without a device."""
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
    "bsk_sets_bottom": "int bsk_sets_bottom(bsk_ctx *ctx, const bsk_sets *s, uint64_t n, bsk_sets **out);",
    "bsk_sets_compare": "int bsk_sets_compare(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, uint64_t limit, bsk_compare **cmp);",
    "bsk_compare_info": "int bsk_compare_info(const bsk_compare *c, uint64_t *n_a, uint64_t *n_b, uint64_t *limit);",
    "bsk_compare_plan": "int bsk_compare_plan(const bsk_compare *c, const char **plan, uint64_t figures[3]);",
    "bsk_compare_fetch": "int bsk_compare_fetch(bsk_ctx *ctx, const bsk_compare *c, uint64_t first_row, uint64_t n_rows, "
                         "uint32_t *shared, uint32_t *total, uint64_t cell_cap);",
    "bsk_compare_device": "int bsk_compare_device(const bsk_compare *c, const uint32_t **shared, const uint32_t **total);",
    "bsk_compare_release": "void bsk_compare_release(bsk_compare *c);",
}
ARITY = dict(bsk_sets_bottom=4, bsk_sets_compare=5, bsk_compare_info=4, bsk_compare_plan=3, bsk_compare_fetch=7, bsk_compare_device=3, bsk_compare_release=1)


def _norm(s):
    s = re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    return re.sub(r"\s+", " ", s).replace("( ", "(").replace(" )", ")").replace(" ;", ";").replace(" ,", ",").strip()


def test_header_declares_the_entries():
    hdr = _norm(open(os.path.join(ROOT, "include", "biosketch.h")).read())
    for name, proto in ENTRIES.items():
        assert _norm(proto) in hdr, name
    assert "typedef struct bsk_compare bsk_compare;" in hdr and "#define BSK_ABI_VERSION 1" in hdr
    # the block follows the counted-sets block and closes the header
    assert hdr.index("int bsk_sets_totals(") < hdr.index("int bsk_sets_bottom(") < hdr.index("typedef struct bsk_compare") < hdr.index("int bsk_sets_compare(")
    assert hdr.index("int bsk_sets_compare(") < hdr.index("void bsk_compare_release(") < hdr.rindex("#ifdef __cplusplus")
    assert hdr.count("void bsk_compare_release(") == 1
    raw = open(os.path.join(ROOT, "include", "biosketch.h")).read()
    assert "/* ---- MinHash: bottom-n sets, all-pairs comparison ----" in raw
    block = raw[raw.index("/* ---- MinHash"):]
    for said in ("limit == 0", "Mash estimator", "bsk_sets_bottom(limit)", "2^64-1", "a == b", "BSK_ERR_UNSUPPORTED", "2^31 cells", "bsk_index_search"):
        assert said in block, said


def test_python_binds_go_and_cpp_call_them():
    from bio_amd import _lib
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    go = open(os.path.join(ROOT, "bindings", "go", "sketches", "compare.go")).read()
    hpp = open(os.path.join(ROOT, "bio_amd", "csrc", "sketches.hpp")).read()
    for name in ENTRIES:
        assert name in bound and len(bound[name][1]) == ARITY[name], name
        assert bound[name][0] is (None if name == "bsk_compare_release" else C.c_int), name
        assert f"C.{name}(" in go, name
        assert name + "(" in hpp or name + ">" in hpp, name
    assert bound["bsk_sets_bottom"][1][2] is C.c_uint64 and bound["bsk_sets_compare"][1][3] is C.c_uint64
    assert bound["bsk_compare_fetch"][1][2] is C.c_uint64 and bound["bsk_compare_fetch"][1][3] is C.c_uint64 and bound["bsk_compare_fetch"][1][6] is C.c_uint64
    for m in ("func (s *Sets) Bottom(", "func (a *Sets) Compare(", "type Compare struct", "func (m *Compare) Info(", "func (m *Compare) Plan(",
              "func (m *Compare) Fetch(", "func (m *Compare) Device(", "func (m *Compare) Close(", "func (m *Compare) Jaccard(", "func (m *Compare) MashDistance("):
        assert m in go, m
    assert "class SetsCompare : public Owned<bsk_compare, bsk_compare_release>" in hpp
    for m in ("bottom", "compare", "info", "plan", "fetch"):
        assert re.search(r"\b%s\(" % m, hpp[hpp.index("// ---- MinHash"):hpp.index("// hits of a search")]), m
    from bio_amd import sketches as S
    sig = inspect.signature(S.Sets.bottom).parameters
    assert list(sig) == ["self", "n", "into"] and sig["into"].default is None
    sig = inspect.signature(S.Sets.compare).parameters
    assert list(sig) == ["self", "other", "limit", "reuse"] and sig["other"].default is None and sig["limit"].default == 0 and sig["reuse"].default is None
    for m in ("info", "plan", "close", "jaccard", "containment"):
        assert list(inspect.signature(getattr(S.Compare, m)).parameters) == ["self"], m
    assert list(inspect.signature(S.Compare.mash_distance).parameters) == ["self", "k"]
    assert isinstance(S.Compare.shared, property) and isinstance(S.Compare.total, property)


def test_python_mirror_arithmetic():
    """jaccard / containment / mash_distance on matrices put in by hand (no device)"""
    from bio_amd import sketches as S

    class Fixed(S.Compare):
        def __init__(self, shared, total, sizes, limit):
            self.h, self._host, self.a_sizes, self._limit = None, (np.array(shared, np.uint32), np.array(total, np.uint32)), np.array(sizes, np.uint64), limit

        def info(self):
            return dict(n_a=self._host[0].shape[0], n_b=self._host[0].shape[1], limit=self._limit)

    c = Fixed([[4, 0, 0], [1, 2, 0]], [[4, 5, 0], [3, 4, 0]], [4, 0], 0)
    j = c.jaccard()
    assert j.dtype == np.float64 and j.tolist() == [[1.0, 0.0, 0.0], [1 / 3, 0.5, 0.0]]
    assert c.containment().tolist() == [[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    d = c.mash_distance(21)
    assert d[0, 0] == 0.0 and d[0, 1] == 1.0 and d[0, 2] == 1.0
    assert d[1, 0] == pytest.approx(-np.log(2 * (1 / 3) / (1 + 1 / 3)) / 21, rel=1e-15) and d[1, 1] == pytest.approx(-np.log(2 * 0.5 / 1.5) / 21, rel=1e-15)
    with pytest.raises(ValueError):
        Fixed([[1]], [[1]], [1], 5).containment()


def test_the_kernels_live_where_the_build_expects_them():
    mk = open(os.path.join(ROOT, "bio_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS =.*\bcompare\.o\b", mk, re.M) and re.search(r"compare\.o:.*sets_internal\.hpp", mk) and re.search(r"^test_compare:", mk, re.M)
    assert re.search(r"^\trm -f .*\btest_compare\b", mk, re.M)
    assert '"test_compare"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    src = open(os.path.join(ROOT, "bio_amd", "csrc", "compare.hip")).read()
    assert "void k_cmp_tile(" in src and "asm" not in src and "rocprim" not in src and "scan_counts(" in src
    for fn in glob.glob(os.path.join(ROOT, "bio_amd", "csrc", "kernels_*.hpp")):
        assert "CMP" not in "".join(re.findall(r"#define (BSK_\w+)\(X\)", open(fn).read())), fn  # no new kernel list: the plan atlas stays as it is


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
    assert not [s for s in re.findall(r" [TW] (\S*(?:ctx_pool|grow_array|bottom_impl|compare_impl|k_cmp_tile|k_bt_gather)\S*)", out)]  # the helpers stay inside the library


def test_null_and_bad_arguments_without_a_device(lib):
    from bio_amd import _lib as L
    fake = C.create_string_buffer(1024)  # zeroed: a bsk_sets / bsk_compare of no context and nothing in it -- every case below fails its checks first
    fp = C.addressof(fake)
    out = C.c_void_p(1234)
    for s, n in ((None, 5), (fp, 5), (fp, 0), (None, 0)):
        assert lib.bsk_sets_bottom(None, s, n, C.byref(out)) == L.ERR_ARG and out.value == 1234  # an argument error leaves *out
    assert lib.bsk_sets_bottom(None, fp, 5, None) == L.ERR_ARG
    cmp_ = C.c_void_p(4321)
    for a, b in ((None, None), (fp, None), (None, fp), (fp, fp)):
        assert lib.bsk_sets_compare(None, a, b, 0, C.byref(cmp_)) == L.ERR_ARG and cmp_.value == 4321
    assert lib.bsk_sets_compare(None, fp, fp, 7, None) == L.ERR_ARG
    v = [C.c_uint64(77) for _ in range(3)]
    assert lib.bsk_compare_info(None, *[C.byref(x) for x in v]) == L.ERR_ARG and [x.value for x in v] == [77] * 3
    assert lib.bsk_compare_info(fp, None, None, None) == L.OK
    assert lib.bsk_compare_info(fp, *[C.byref(x) for x in v]) == L.OK and [x.value for x in v] == [0] * 3
    p, f = C.c_char_p(b"x"), (C.c_uint64 * 3)(9, 9, 9)
    assert lib.bsk_compare_plan(None, C.byref(p), f) == L.ERR_ARG and p.value == b"x" and list(f) == [9, 9, 9]
    assert lib.bsk_compare_plan(fp, None, None) == L.OK and lib.bsk_compare_plan(fp, C.byref(p), f) == L.OK and p.value == b"" and list(f) == [0, 0, 0]
    sh, tt = np.full(4, 7, np.uint32), np.full(4, 7, np.uint32)
    assert lib.bsk_compare_fetch(None, fp, 0, 0, sh.ctypes.data, tt.ctypes.data, 4) == L.ERR_ARG
    assert lib.bsk_compare_fetch(None, None, 0, 0, None, None, 0) == L.ERR_ARG
    assert list(sh) == [7] * 4 and list(tt) == [7] * 4
    a, b = C.c_void_p(5), C.c_void_p(6)
    assert lib.bsk_compare_device(None, C.byref(a), C.byref(b)) == L.ERR_ARG and (a.value, b.value) == (5, 6)
    assert lib.bsk_compare_device(fp, C.byref(a), None) == L.OK and a.value is None
    lib.bsk_compare_release(None)
