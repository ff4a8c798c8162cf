"""CPU: the hits by target (bsk_hits_transpose, bsk_hits_tally and the bsk_tally_* entries) -- declared with the contract's prototypes
directly in front of the clusters block, bound by bio_amd._lib, called from the Go shim and the C++ owners, exported by the library with
their helpers hidden, built where the build expects them, and their argument checks as far as they run without a device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "bsk_hits_transpose": "int bsk_hits_transpose(bsk_ctx *ctx, const bsk_hits *h, uint64_t n_targets, bsk_hits **out);",
    "bsk_hits_tally": "int bsk_hits_tally(bsk_ctx *ctx, const bsk_hits *h, uint64_t n_targets, uint32_t flags, bsk_tally **out);",
    "bsk_tally_info": "int bsk_tally_info(const bsk_tally *t, uint64_t *n_targets, uint64_t *queries, uint64_t *hits, uint64_t *calls);",
    "bsk_tally_plan": "int bsk_tally_plan(const bsk_tally *t, const char **plan);",
    "bsk_tally_fetch": "int bsk_tally_fetch(bsk_ctx *ctx, const bsk_tally *t, uint64_t first, uint64_t count, uint64_t *rows, uint64_t *unique, uint64_t *shared);",
    "bsk_tally_device": "int bsk_tally_device(const bsk_tally *t, const uint64_t **rows, const uint64_t **unique, const uint64_t **shared);",
    "bsk_tally_release": "void bsk_tally_release(bsk_tally *t);",
}
ARITY = dict(bsk_hits_transpose=4, bsk_hits_tally=5, bsk_tally_info=5, bsk_tally_plan=2, bsk_tally_fetch=7, bsk_tally_device=4, bsk_tally_release=1)
KERNELS = ("k_tp_keys", "k_tp_offsets", "k_tp_place", "k_tl_check", "k_tl_add")


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
    assert _norm("enum { BSK_TALLY_ADD = 1 };") in hdr and _norm("typedef struct bsk_tally bsk_tally;") in hdr and "#define BSK_ABI_VERSION 1" in hdr
    order = ["int bsk_hits_top_by(", "enum { BSK_TALLY_ADD", "typedef struct bsk_tally", "int bsk_hits_transpose(", "int bsk_hits_tally(", "void bsk_tally_release(",
             "enum { BSK_CLUSTER_COMPONENTS", "enum { BSK_NEIGHBORS_UPPER", "int bsk_hits_fetch_totals("]
    at = [hdr.index(x) for x in order]
    assert at == sorted(at)
    a, b = raw.index("/* ---- hits by target"), raw.index("/* ---- clusters of a neighbour graph")
    assert raw.index("/* ---- hits selected by a measure") < a < b < raw.index("/* ---- sparse all-pairs comparison")  # the neighbours block still closes the header
    block = raw[a:b]
    for said in ("n_targets rows", "ascending", "keep their order in h", "same has-flags", "exactly\n * the flags of h", "trailing ones included", "need not have ascending rows",
                 "bit for bit", "keep the slot", "*out == h", "another context", "target >= n_targets", "before the object is taken over", "BSK_ERR_UNSUPPORTED", "release it",
                 "n_targets == 0", "k_tp_keys", "k_tp_offsets", "k_tp_place", "every key distinct", "No\n * atomics on the output", "nothing rests on the sort being stable",
                 "bit-identical from call to call", "targets=, hits= and\n * key_bits=", "n_large_queries is 0", "rows[t]", "unique[t]", "shared[t]", "cannot reach 2^64",
                 "add modulo 2^64", "are not tallied", "one bsk_hits_transpose\n * away", "only grow", "NULL slot\n * under ADD is a fresh table", "another n_targets",
                 "any other flag bit", "the table is unchanged", "k_tl_check", "before anything is added", "2 048 targets", "3 x 8 B x 2 048 = 48 KB", "160 KB",
                 "one global add per counter and workgroup", "straight to the table in global memory", "offsets difference 1", "which path ran", "first + count > n_targets"):
        assert said in block, said
    slot = raw[raw.index("/* The result slot."):raw.index("int bsk_result_sets_reuse(")]
    assert "bsk_hits_transpose" in slot and "bsk_hits_tally" in slot


def test_python_binds_go_and_cpp_call_them():
    from bio_amd import _lib
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    go = _read("bindings", "go", "sketches", "transpose.go")
    hpp = _read("bio_amd", "csrc", "sketches.hpp")
    for name in ENTRIES:
        assert name in bound and len(bound[name][1]) == ARITY[name] and bound[name][0] is (None if name == "bsk_tally_release" else C.c_int), name
        assert f"C.{name}(" in go, name
        assert name + ("(" if name != "bsk_tally_release" else ">") in hpp, name  # (the release is the owner's template argument)
    assert bound["bsk_hits_transpose"][1][2] is C.c_uint64 and bound["bsk_hits_tally"][1][2:4] == [C.c_uint64, C.c_uint32] and _lib.TALLY_ADD == 1
    for m in ("func (h *Hits) Transpose(nTargets uint64, reuse *Hits) (*Hits, error)", "func (h *Hits) Tally(nTargets uint64, add bool, into *Tally) (*Tally, error)",
              "type Tally struct", "func (t *Tally) Info()", "func (t *Tally) Fetch(first, count uint64)", "func (t *Tally) Release()", "C.BSK_TALLY_ADD"):
        assert m in go, m
    for m in ("class Tally : public Owned<bsk_tally, bsk_tally_release>", "int transpose(Engine &e, uint64_t n_targets, SearchHits &into) const",
              "int tally(Engine &e, uint64_t n_targets, bool add, Tally &into) const"):
        assert m in hpp, m
    assert hpp.index("class Tally :") < hpp.index("class SearchHits :")
    from bio_amd import sketches as S
    sig = inspect.signature(S.Hits.transpose).parameters
    assert list(sig) == ["self", "n_targets", "reuse"] and all(sig[k].default is None for k in ("n_targets", "reuse"))
    sig = inspect.signature(S.Hits.tally).parameters
    assert list(sig) == ["self", "n_targets", "into", "add"] and sig["n_targets"].default is None and sig["into"].default is None and sig["add"].default is False
    for attr in ("rows", "unique", "shared", "info", "plan", "fetch", "device", "close"):
        assert hasattr(S.Tally, attr), attr
    assert S.Tally._release == "bsk_tally_release" and list(inspect.signature(S.Tally.fetch).parameters) == ["self", "first", "count"]


def test_the_kernels_live_where_the_build_expects_them():
    mk = _read("bio_amd", "csrc", "Makefile")
    assert re.search(r"^OBJS =.*\btranspose\.o\b", mk, re.M) and re.search(r"transpose\.o:.*sets_internal\.hpp.*search_internal\.hpp", mk)
    assert re.search(r"^test_transpose:.*tests/cpp/test_transpose\.cpp.*sketches\.hpp.*libbiosketch\.so", mk, re.M) and re.search(r"^\trm -f .*\btest_transpose\b", mk, re.M)
    assert '"test_transpose"' in _read("__graft_entry__.py")
    assert "bio_amd/csrc/test_transpose" in _read(".gitignore").split()
    assert "test_transpose" in _read("tests", "test_gpu_transpose_cpp.py")
    src = _read("bio_amd", "csrc", "transpose.hip")
    for k in KERNELS:
        assert f"void {k}(" in src, k
    code = re.sub(r"//.*", "", src)
    assert "sets_sort_u64(" in code and "rocprim" not in code and "asm" not in code and "->cus" not in code  # the library's sort, no new instantiation, grids through the helper
    for banned in ("atomicCAS", "atomicExch", "while (", "__threadfence", "volatile", "double", "float", "hipMalloc", "<<<"):
        assert banned not in code, banned  # bounded loops, integers, pooled memory, no retry and no wait on another workgroup
    launches = re.findall(r"hipLaunchKernelGGL\([^;]*;", code)
    assert len(launches) == 6 and all(re.search(r"dim3\((?:grid_for|tp_grid)\(ctx", x) for x in launches)  # every grid is capped
    assert "inline unsigned tp_grid(const bsk_ctx *ctx, u64 items) { return grid_for(ctx, items, TP_BLOCK, 16); }" in src
    # the transpose has no atomics but the flag; the tally's are adds
    tp = code[code.index("void k_tp_keys("):code.index("void k_tl_check(")]
    assert "atomic" not in tp and set(re.findall(r"\batomic\w+", code)) == {"atomicOr", "atomicAdd"}
    assert re.search(r"#define TL_LDS_TARGETS 2048\b", src) and "3 * TL_LDS_TARGETS" in src and re.search(r"#define TL_BLOCK 512\b", src)
    # the other translation units of the hits know nothing of it
    for fn in ("search.hip", "fold.hip", "cluster.hip", "select.hip", "compare.hip"):
        other = _read("bio_amd", "csrc", fn)
        assert "transpose" not in other and "tally" not in other, fn
    slots = {k: int(v) for k, v in re.findall(r"\b(SLOT_\w+|POOL_SLOTS) = (\d+)", _read("bio_amd", "csrc", "host_types.hpp"))}
    mine = [slots[k] for k in ("SLOT_TRANSPOSE_WORK", "SLOT_TALLY_WORK")]
    assert len(set(mine)) == 2 and all(v < slots["POOL_SLOTS"] for v in mine)
    assert not [k for k, v in slots.items() if v in mine and k not in ("SLOT_TRANSPOSE_WORK", "SLOT_TALLY_WORK")]  # shared with nobody
    assert slots["POOL_SLOTS"] == max(v for k, v in slots.items() if k != "POOL_SLOTS") + 1


def test_the_checks_come_in_the_contracts_order():
    """without a context the argument checks cannot be told apart, so their order is read from the source: nothing touches the device before
    them, and the pass that refuses a target >= n_targets runs, and is read, before the slot is taken over and before anything is added"""
    src = _read("bio_amd", "csrc", "transpose.hip")
    args = src[src.index("int tp_check_args("):src.index("struct TpScratch")]
    at = [args.index(x) for x in ("null argument", "holds h itself", "another context", "BSK_ERR_UNSUPPORTED")]
    assert at == sorted(at) and "hip" not in args
    body = src[src.index('extern "C" int bsk_hits_transpose('):src.index('extern "C" int bsk_hits_tally(')]
    at = [body.index(x) for x in ("tp_check_args(", "hipSetDevice", "ctx_pool(", "k_tp_keys", "read_back(", "a target >= n_targets", "take_over(")]
    assert at == sorted(at)
    body = src[src.index('extern "C" int bsk_hits_tally('):src.index('extern "C" int bsk_tally_info(')]
    at = [body.index(x) for x in ("tp_check_args(", "unknown flag", "another n_targets", "hipSetDevice", "k_tl_check", "read_back(", "a target >= n_targets", "take_over(")]
    assert at == sorted(at) and "k_tl_add" not in body


@pytest.fixture(scope="module")
def lib():
    from bio_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_library_exports_them_and_hides_the_helpers(lib):
    from bio_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (bsk_\w+)", out))
    assert set(ENTRIES) <= exported
    hidden = "|".join(KERNELS + ("transpose_impl", "tally_impl", "tp_check_args", "TpScratch", "TpHits", "tl_add_hit", "tp_row_of"))
    assert not re.findall(r" [TW] (\S*(?:%s)\S*)" % hidden, out)  # the helpers stay inside the library
    declared = set(re.findall(r"\b(bsk_\w+)\(", _norm(_read("include", "biosketch.h"))))
    assert exported <= declared, exported - declared  # the header's entries and no more
    assert {s for s in exported if "transpose" in s or "tally" in s} == set(ENTRIES)
    for s in ENTRIES:  # the substrings other entries' tests claim
        assert not any(x in s for x in ("filter", "top_by", "cluster", "windows", "fold", "members")), s


def test_null_and_bad_arguments_without_a_device(lib):
    from bio_amd import _lib as L
    fake = C.create_string_buffer(2048)  # zeroed: hits of no context and nothing in them -- every case below fails its checks first
    fp = C.addressof(fake)
    out = C.c_void_p(4321)
    for ctx, h in ((None, None), (None, fp)):
        assert lib.bsk_hits_transpose(ctx, h, 5, C.byref(out)) == L.ERR_ARG and out.value == 4321
        for flags in (0, L.TALLY_ADD, 2, 0xFFFFFFFF):
            assert lib.bsk_hits_tally(ctx, h, 5, flags, C.byref(out)) == L.ERR_ARG and out.value == 4321
    assert lib.bsk_hits_transpose(None, fp, 5, None) == L.ERR_ARG and lib.bsk_hits_tally(None, fp, 5, 0, None) == L.ERR_ARG
    same = C.c_void_p(fp)  # *out == h
    assert lib.bsk_hits_transpose(None, fp, 5, C.byref(same)) == L.ERR_ARG and same.value == fp
    assert lib.bsk_hits_transpose(None, fp, 1 << 32, C.byref(out)) == L.ERR_ARG and out.value == 4321  # (the NULL context comes first)
    # the table's own entries
    v = C.c_uint64(7)
    assert lib.bsk_tally_info(None, C.byref(v), None, None, None) == L.ERR_ARG and v.value == 7
    p = C.c_char_p()
    assert lib.bsk_tally_plan(None, C.byref(p)) == L.ERR_ARG and lib.bsk_tally_device(None, None, None, None) == L.ERR_ARG
    assert lib.bsk_tally_fetch(None, None, 0, 0, None, None, None) == L.ERR_ARG and lib.bsk_tally_fetch(None, fp, 0, 0, None, None, None) == L.ERR_ARG
    lib.bsk_tally_release(None)
    # a table of no context and no targets: info, plan and device answer; a fetch beyond it is refused before anything is copied
    assert lib.bsk_tally_info(fp, C.byref(v), None, None, None) == L.OK and v.value == 0
    assert lib.bsk_tally_plan(fp, C.byref(p)) == L.OK and p.value == b""
