"""CPU: the abundance-weighted entries of include/biosketch.h (bsk_sets_compare_counted, bsk_compare_weights_device,
bsk_compare_fetch_weights, bsk_sets_sumsq) -- declared with the contract's prototypes behind the MinHash block, bound by bio_amd._lib,
called from the Go shim and the C++ owners, exported by the library, their argument checks as far as they run without a device, and the
Python mirror's arithmetic on matrices put in by hand."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import compare_counted_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "bsk_sets_compare_counted": "int bsk_sets_compare_counted(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, uint64_t limit, bsk_compare **cmp);",
    "bsk_compare_weights_device": "int bsk_compare_weights_device(const bsk_compare *c, const uint64_t **dot, const uint64_t **min_sum);",
    "bsk_compare_fetch_weights": "int bsk_compare_fetch_weights(bsk_ctx *ctx, const bsk_compare *c, uint64_t first_row, uint64_t n_rows, "
                                 "uint64_t *dot, uint64_t *min_sum, uint64_t cell_cap);",
    "bsk_sets_sumsq": "int bsk_sets_sumsq(bsk_ctx *ctx, const bsk_sets *s, uint64_t first, uint64_t count, uint64_t *sumsq);",
}
ARITY = dict(bsk_sets_compare_counted=5, bsk_compare_weights_device=3, bsk_compare_fetch_weights=7, bsk_sets_sumsq=5)


def _norm(s):
    s = re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    return re.sub(r"\s+", " ", s).replace("( ", "(").replace(" )", ")").replace(" ;", ";").replace(" ,", ",").strip()


def test_header_declares_the_entries():
    raw = open(os.path.join(ROOT, "include", "biosketch.h")).read()
    hdr = _norm(raw)
    for name, proto in ENTRIES.items():
        assert _norm(proto) in hdr, name
        assert hdr.count("int %s(" % name) == 1, name
    assert "#define BSK_ABI_VERSION 1" in hdr
    # the block follows bsk_compare_release and closes the header
    assert hdr.index("void bsk_compare_release(") < hdr.index("int bsk_sets_compare_counted(") < hdr.index("int bsk_compare_weights_device(")
    assert hdr.index("int bsk_compare_weights_device(") < hdr.index("int bsk_compare_fetch_weights(") < hdr.index("int bsk_sets_sumsq(") < hdr.rindex("#ifdef __cplusplus")
    assert "/* ---- abundance-weighted all-pairs comparison of counted sets ----" in raw
    block = raw[raw.index("/* ---- abundance-weighted"):]
    assert raw.index("/* ---- MinHash") < raw.index("void bsk_compare_release(") < raw.index("/* ---- abundance-weighted")
    for said in ("ca(v) * cb(v)", "saturating at 2^64-1", "min(ca(v), cb(v))", "exact", "associative", "counts 1 for every value", "dot == min_sum == shared",
                 "2^31 cells", "leaves it unweighted", "keeps the two arrays", "both NULL for an unweighted result", "BSK_ERR_ARG for an unweighted result",
                 "k_cmp_tile_w", "totals(a)[i] + totals(b)[j] - min_sum", "bsk_sets_sumsq", "bsk_sets_totals", "cosine", "limit == 0"):
        assert said in block, said


def test_python_binds_go_and_cpp_call_them():
    from bio_amd import _lib
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    go = open(os.path.join(ROOT, "bindings", "go", "sketches", "compare.go")).read() + open(os.path.join(ROOT, "bindings", "go", "sketches", "counts.go")).read()
    hpp = open(os.path.join(ROOT, "bio_amd", "csrc", "sketches.hpp")).read()
    for name in ENTRIES:
        assert name in bound and len(bound[name][1]) == ARITY[name] and bound[name][0] is C.c_int, name
        assert f"C.{name}(" in go, name
        assert name + "(" in hpp, name
    assert bound["bsk_sets_compare_counted"][1][3] is C.c_uint64 and bound["bsk_sets_compare_counted"][1] == bound["bsk_sets_compare"][1]
    assert bound["bsk_compare_fetch_weights"][1] == bound["bsk_compare_fetch"][1] and bound["bsk_sets_sumsq"][1] == bound["bsk_sets_totals"][1]
    for m in ("func (a *Sets) CompareCounted(", "func (m *Compare) Weights(", "func (m *Compare) FetchWeights(", "func (m *Compare) Cosine(", "func (s *Sets) SumSq("):
        assert m in go, m
    owners = hpp[hpp.index("class DeviceSets"):hpp.index("// hits of a search")]
    for m in ("compare_counted", "sumsq", "fetch_weights", "weighted"):
        assert re.search(r"\b%s\(" % m, owners), m
    assert owners.index("int sumsq(") < owners.index("class SetsCompare") < owners.index("int compare_counted(") < owners.index("int fetch_weights(")
    from bio_amd import sketches as S
    sig = inspect.signature(S.Sets.compare_counted).parameters
    assert list(sig) == ["self", "other", "limit", "reuse"] and sig["other"].default is None and sig["limit"].default == 0 and sig["reuse"].default is None
    assert list(inspect.signature(S.Sets.compare).parameters) == ["self", "other", "limit", "reuse"]  # as it was
    assert list(inspect.signature(S.Sets.sumsq).parameters) == ["self"]
    for m in ("cosine", "angular_similarity", "weighted_jaccard", "bray_curtis"):
        assert list(inspect.signature(getattr(S.Compare, m)).parameters) == ["self"], m
    sig = inspect.signature(S.Compare.fetch_weights).parameters
    assert list(sig) == ["self", "first_row", "n_rows"] and sig["first_row"].default == 0 and sig["n_rows"].default is None
    for p in ("dot", "min_sum", "weighted", "shared", "total"):
        assert isinstance(getattr(S.Compare, p), property), p


def test_the_kernel_lives_where_the_build_expects_it():
    mk = open(os.path.join(ROOT, "bio_amd", "csrc", "Makefile")).read()
    assert re.search(r"^test_compare_counted:.*tests/cpp/test_compare_counted\.cpp", mk, re.M) and re.search(r"^\trm -f .*\btest_compare_counted\b", mk, re.M)
    assert '"test_compare_counted"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "bio_amd/csrc/test_compare_counted\n" in open(os.path.join(ROOT, ".gitignore")).read()
    src = open(os.path.join(ROOT, "bio_amd", "csrc", "compare.hip")).read()
    assert "void k_cmp_tile(" in src and "void k_cmp_tile_w(" in src and re.search(r"^#define CMP_W_BLOCKS_PER_CU 3\b", src, re.M)
    assert src.index("namespace {") < src.index("void k_cmp_tile_w(") < src.index("}  // namespace")  # a helper like the others
    for window in ("s_ac[CMP_ROWS * CMP_WINDOW]", "s_bc[CMP_COLS * CMP_WINDOW]", "s_ac[r * CMP_WINDOW + ia]", "s_bc[ib * CMP_COLS + c]"):
        assert window in src, window  # a count sits at its value's index
    cnt = open(os.path.join(ROOT, "bio_amd", "csrc", "counts.hip")).read()
    assert "void k_ct_sumsq(" in cnt and "add_sat(" in cnt and "__shfl_xor(" in cnt[cnt.index("void k_ct_sumsq("):cnt.index("unsigned ct_grid(")]


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
    assert set(ENTRIES) <= set(re.findall(r" T (bsk_\w+)", out))
    assert not [s for s in re.findall(r" [TW] (\S*(?:compare_entry|compare_impl|k_cmp_tile_w|k_ct_sumsq|add_sat)\S*)", out)]  # the helpers stay inside the library


def test_null_and_bad_arguments_without_a_device(lib):
    from bio_amd import _lib as L
    fake = C.create_string_buffer(1024)  # zeroed: a bsk_sets / bsk_compare of no context and nothing in it -- every case below fails its checks first
    fp = C.addressof(fake)
    cmp_ = C.c_void_p(4321)
    for a, b in ((None, None), (fp, None), (None, fp), (fp, fp)):
        assert lib.bsk_sets_compare_counted(None, a, b, 0, C.byref(cmp_)) == L.ERR_ARG and cmp_.value == 4321  # an argument error leaves *cmp
    assert lib.bsk_sets_compare_counted(None, fp, fp, 7, None) == L.ERR_ARG
    a, b = C.c_void_p(5), C.c_void_p(6)
    assert lib.bsk_compare_weights_device(None, C.byref(a), C.byref(b)) == L.ERR_ARG and (a.value, b.value) == (5, 6)
    assert lib.bsk_compare_weights_device(fp, C.byref(a), None) == L.OK and a.value is None  # zeroed: unweighted
    assert lib.bsk_compare_weights_device(fp, None, C.byref(b)) == L.OK and b.value is None and lib.bsk_compare_weights_device(fp, None, None) == L.OK
    dt, ms = np.full(4, 7, np.uint64), np.full(4, 7, np.uint64)
    assert lib.bsk_compare_fetch_weights(None, fp, 0, 0, dt.ctypes.data, ms.ctypes.data, 4) == L.ERR_ARG
    assert lib.bsk_compare_fetch_weights(None, None, 0, 0, None, None, 0) == L.ERR_ARG
    assert list(dt) == [7] * 4 and list(ms) == [7] * 4
    q = np.full(3, 9, np.uint64)
    assert lib.bsk_sets_sumsq(None, fp, 0, 0, q.ctypes.data) == L.ERR_ARG and lib.bsk_sets_sumsq(None, None, 0, 0, None) == L.ERR_ARG
    assert lib.bsk_sets_sumsq(None, fp, 0, 2, None) == L.ERR_ARG and list(q) == [9] * 3


# ---- the Python mirror's arithmetic, no device ----
def fixed(shared, total, dot, ms, qa, qb, ta, tb, limit=0):
    from bio_amd import sketches as S

    class Fixed(S.Compare):
        def __init__(self):
            self.h, self._host, self.a_sizes = None, (np.array(shared, np.uint32), np.array(total, np.uint32)), np.zeros(len(shared), np.uint64)
            self._whost = (np.array(dot, np.uint64), np.array(ms, np.uint64))
            self._norms = tuple(np.array(x, np.uint64) for x in (qa, qb, ta, tb))

        def info(self):
            return dict(n_a=self._host[0].shape[0], n_b=self._host[0].shape[1], limit=limit)

    return Fixed()


def test_python_mirror_arithmetic():
    TOP = WC.MAX
    #            b0: norm 9, total 4    b1: norm 0, total 0     b2: norm 4, total 2
    dot = [[12, 0, TOP], [5, 0, 1], [3, 0, 2]]
    ms = [[3, 0, 2], [0, 0, 1], [1, 0, 1]]
    c = fixed([[1, 0, 1]] * 3, [[2, 1, 2]] * 3, dot, ms, qa=[16, 9, TOP], qb=[9, 0, 4], ta=[5, 0, 7], tb=[4, 0, 2])
    assert c.weighted and c.dot.dtype == np.uint64 and c.dot.tolist() == dot and c.min_sum.tolist() == ms
    cos = c.cosine()
    assert cos.dtype == np.float64 and cos.shape == (3, 3)
    assert cos[0, 0] == 1.0 and cos[1, 0] == 5 / 9 and cos[1, 2] == 1 / 6          # 12 / (4 * 3), 5 / (3 * 3), 1 / (3 * 2)
    assert cos[0, 1] == 0.0 and cos[1, 1] == 0.0                                   # a zero norm
    assert math.isnan(cos[0, 2]) and all(math.isnan(x) for x in cos[2])            # a saturated cell; a saturated norm
    want = WC.ref_cosine(np.array(dot, np.uint64), np.array([16, 9, TOP], np.uint64), np.array([9, 0, 4], np.uint64))
    assert np.array_equal(cos, want, equal_nan=True)
    ang = c.angular_similarity()
    assert ang[0, 0] == 1.0 and ang[0, 1] == 0.0 and math.isnan(ang[0, 2]) and ang[1, 0] == 1.0 - 2.0 * math.acos(5 / 9) / math.pi
    assert np.array_equal(ang, WC.ref_angular(want), equal_nan=True)
    wj = c.weighted_jaccard()
    assert wj[0, 0] == 3 / (5 + 4 - 3) and wj[1, 1] == 0.0 and wj[0, 1] == 0.0 and wj[2, 2] == 1 / 8 and wj.dtype == np.float64
    assert np.array_equal(wj, WC.ref_weighted_jaccard(c.min_sum, np.array([5, 0, 7], np.uint64), np.array([4, 0, 2], np.uint64)))
    bc = c.bray_curtis()
    assert bc[0, 0] == 1 - 6 / 9 and bc[1, 1] == 0.0 and bc[0, 1] == 1.0 and bc[2, 2] == 1 - 2 / 9
    assert np.array_equal(bc, WC.ref_bray_curtis(c.min_sum, np.array([5, 0, 7], np.uint64), np.array([4, 0, 2], np.uint64)))
    # a cosine a rounding above 1 has the angular similarity 1
    one = fixed([[1]], [[1]], [[3]], [[1]], qa=[3], qb=[3], ta=[1], tb=[1])
    assert one.angular_similarity()[0, 0] == 1.0
    # whole sets only
    cut = fixed([[1]], [[1]], [[1]], [[1]], qa=[1], qb=[1], ta=[1], tb=[1], limit=5)
    for m in ("cosine", "angular_similarity", "weighted_jaccard", "bray_curtis"):
        with pytest.raises(ValueError):
            getattr(cut, m)()
    assert cut.dot.tolist() == [[1]]  # the matrices themselves are defined for every limit


def test_an_unweighted_object_has_no_weighted_side():
    """the existing methods work on an object that has only h, _host and a_sizes; the weighted ones refuse it"""
    from bio_amd import sketches as S

    class Plain(S.Compare):
        def __init__(self):
            self.h, self._host, self.a_sizes = None, (np.array([[2, 0]], np.uint32), np.array([[4, 3]], np.uint32)), np.array([4], np.uint64)

        def info(self):
            return dict(n_a=1, n_b=2, limit=0)

    p = Plain()
    assert p.jaccard().tolist() == [[0.5, 0.0]] and p.containment().tolist() == [[0.5, 0.0]] and p.mash_distance(21)[0, 1] == 1.0
    assert p.weighted is False
    for m in ("cosine", "angular_similarity", "weighted_jaccard", "bray_curtis"):
        with pytest.raises(ValueError):
            getattr(p, m)()
    with pytest.raises(ValueError):
        p.dot
