"""CPU: the entries of the window sets and the folded hits (bsk_result_sets_windows, bsk_hits_fold, bsk_hits_members_device,
bsk_hits_fetch_members) -- declared with the contract's prototypes between bsk_sets_sumsq and the clusters block, bound by bio_amd._lib,
called from the Go shim and the C++ owners, exported by the library and nothing else with them, built where the build expects them, and
their argument checks as far as they run without a device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "bsk_result_sets_windows": "int bsk_result_sets_windows(bsk_ctx *ctx, const bsk_result *r, const bsk_window_params *wp, int scale, bsk_sets **sets, "
                               "uint64_t *seq_offsets);",
    "bsk_hits_fold": "int bsk_hits_fold(bsk_ctx *ctx, const bsk_hits *h, const uint64_t *group_offsets, uint64_t n_groups, const bsk_fold_params *fp, bsk_hits **out);",
    "bsk_hits_members_device": "int bsk_hits_members_device(const bsk_hits *h, const uint32_t **members);",
    "bsk_hits_fetch_members": "int bsk_hits_fetch_members(bsk_ctx *ctx, const bsk_hits *h, uint64_t first, uint64_t count, uint32_t *members, uint64_t hit_cap);",
}
ARITY = dict(bsk_result_sets_windows=6, bsk_hits_fold=6, bsk_hits_members_device=2, bsk_hits_fetch_members=6)
WIN_KERNELS = ("k_win_count", "k_win_spans")
FOLD_KERNELS = ("k_fold_map", "k_fold_rows", "k_fold_check", "k_fold_runs", "k_fold_place", "k_fold_offsets")


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
    assert "enum { BSK_WINDOWS_COUNTED = 1 };" in hdr and "#define BSK_ABI_VERSION 1" in hdr
    assert _norm("typedef struct bsk_window_params { uint32_t window; uint32_t step; uint32_t count; uint32_t flags; } bsk_window_params;") in hdr
    assert _norm("typedef struct bsk_fold_params { uint32_t min_members; uint32_t flags; uint32_t frac_num; uint32_t frac_den; } bsk_fold_params;") in hdr
    order = ["int bsk_sets_sumsq(", "enum { BSK_WINDOWS_COUNTED", "typedef struct bsk_window_params", "int bsk_result_sets_windows(", "typedef struct bsk_fold_params",
             "int bsk_hits_fold(", "int bsk_hits_members_device(", "int bsk_hits_fetch_members(", "enum { BSK_CLUSTER_COMPONENTS", "int bsk_hits_cluster(",
             "enum { BSK_NEIGHBORS_UPPER", "int bsk_hits_fetch_totals("]
    at = [hdr.index(x) for x in order]
    assert at == sorted(at)
    a, b = raw.index("/* ---- window sets and folded hits"), raw.index("/* ---- clusters of a neighbour graph")
    assert raw.index("int bsk_sets_sumsq(") < a < b
    block = raw[a:b]
    # the definition, in the contract's terms
    for said in ("p = pos[] & ~BSK_POS_STRAND_BIT", "p = j", "last position P", "W = max(1, ceil((P + 1) / count)) and S = W", "W = window and S = step ? step : window",
                 "first(p) = p < W ? 0 : (p - W) / S + 1", "p / W", "nwin = c ? first(P) + 1 : 0", "w*S <= p < w*S + W", "at least one window", "several windows",
                 "empty sets", "nwin <= count", "not from the sequence length", "does not keep lengths", "seq_offsets[i] + w", "seq_offsets[n_reads]", "MaxUint64/scale",
                 "run length inside the window", "bsk_sets_reduce(windows, seq_offsets, n_reads, 1)", "for any step", "window >= 2^31", "keeps the slot", "release the slot",
                 "position order", "k_win_count", "k_win_spans",
                 "group_offsets[0] == 0", "non-decreasing", "at most 2^32", "n_groups < 2^32", "Empty groups are legal", "not retained", "saturating at 2^32-1",
                 "fifth u32 array", "max(min_members, 1)", "(uint64_t)members * frac_den >= (uint64_t)frac_num * group_size", "{1, 0, 0, 0}", "neither totals nor weights",
                 "carries no members", "strictly ascending", "bsk_hits_top results", "k_fold_check", "before the object is taken over", "*out == h", "n_queries == 0",
                 "k_fold_map", "k_fold_runs", "k_fold_place", "bit-identical", "groups=", "kept="):
        assert said in block, said
    slot = raw[raw.index("/* The result slot."):raw.index("int bsk_result_sets_reuse(")]
    assert "bsk_hits_fold" in slot and "bsk_result_sets_windows" in slot


def test_python_binds_go_and_cpp_call_them():
    from bio_amd import _lib
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    go = _read("bindings", "go", "sketches", "windows.go")
    hpp = _read("bio_amd", "csrc", "sketches.hpp")
    for name in ENTRIES:
        assert name in bound and len(bound[name][1]) == ARITY[name] and bound[name][0] is C.c_int, name
        assert f"C.{name}(" in go, name
        assert name + "(" in hpp, name
        assert "cluster" not in name
    for st, fields in ((_lib.WindowParams, ["window", "step", "count", "flags"]), (_lib.FoldParams, ["min_members", "flags", "frac_num", "frac_den"])):
        assert [f for f, _ in st._fields_] == fields and all(t is C.c_uint32 for _, t in st._fields_) and C.sizeof(st) == 16
    assert _lib.WINDOWS_COUNTED == 1
    assert bound["bsk_hits_fold"][1][3] is C.c_uint64 and bound["bsk_result_sets_windows"][1][3] is C.c_int
    for m in ("type WindowParams struct", "func (r *DeviceResult) WindowSets(p WindowParams, scale int, into *Sets) (sets *Sets, seqOffsets []uint64, err error)",
              "type FoldParams struct", "func (h *Hits) Fold(groupOffsets []uint64, p FoldParams, reuse *Hits) (*Hits, error)", "func (h *Hits) Members() unsafe.Pointer",
              "func (h *Hits) FetchMembers() ([]uint32, error)", "C.BSK_WINDOWS_COUNTED"):
        assert m in go, m
    for m in ("int from_windows(Engine &e, const bsk_result *r, const bsk_window_params &wp, int scale", "int fold(Engine &e, const std::vector<uint64_t> &group_offsets",
              "const uint32_t *members_device() const", "int fetch_members(Engine &e, std::vector<uint32_t> &members) const"):
        assert m in hpp, m
    from bio_amd import sketches as S
    sig = inspect.signature(S.BatchResult.window_sets).parameters
    assert list(sig) == ["self", "window", "step", "count", "scale", "counted", "into"] and [sig[k].default for k in list(sig)[1:]] == [0, 0, 0, 1, False, None]
    sig = inspect.signature(S.Hits.fold).parameters
    assert list(sig) == ["self", "group_offsets", "min_members", "min_fraction", "reuse"] and [sig[k].default for k in list(sig)[2:]] == [1, None, None]
    assert isinstance(S.Hits.members, property) and callable(S.Hits.has_members) and callable(S.Hits.fetch_members) and S.Sets.group_offsets is None


def test_the_kernels_live_where_the_build_expects_them():
    mk = _read("bio_amd", "csrc", "Makefile")
    assert re.search(r"^OBJS =.*\bwindows\.o\b", mk, re.M) and re.search(r"^OBJS =.*\bfold\.o\b", mk, re.M)
    assert re.search(r"windows\.o:.*sets_internal\.hpp", mk) and re.search(r"fold\.o:.*sets_internal\.hpp.*search_internal\.hpp", mk)
    assert re.search(r"^test_windows:.*tests/cpp/test_windows\.cpp.*sketches\.hpp.*libbiosketch\.so", mk, re.M) and re.search(r"^\trm -f .*\btest_windows\b", mk, re.M)
    assert '"test_windows"' in _read("__graft_entry__.py")
    assert "bio_amd/csrc/test_windows" in _read(".gitignore").split()
    win, fold = _read("bio_amd", "csrc", "windows.hip"), _read("bio_amd", "csrc", "fold.hip")
    for k in WIN_KERNELS:
        assert f"void {k}(" in win, k
    for k in FOLD_KERNELS:
        assert f"void {k}(" in fold, k
    for src in (win, fold):
        code = re.sub(r"//.*", "", src)
        assert "scan_counts(" in code and "rocprim" not in code and "asm" not in code and "->cus" not in code  # the library's scan, no new instantiation, grids through the helper
        for banned in ("atomicCAS", "atomicExch", "while (", "__threadfence", "volatile", "double", "float", "hipMalloc", "<<<"):
            assert banned not in code, banned  # bounded loops, integers, pooled memory, no retry and no wait on another workgroup
        assert len(re.findall(r"hipLaunchKernelGGL\(", code)) == len(re.findall(r"hipLaunchKernelGGL\([^;]*?(?:grid_for|fold_grid)\(ctx", code))  # every grid is capped
    # the windows go through the ONE sets path: the spans are its source, nothing of it is copied
    code = re.sub(r"//.*", "", win)
    assert "sets_build_spans(ctx, src, BSK_SETS_PER_SEQUENCE" in code and "segmented" not in code and "k_sets_rows" not in code
    sets = _read("bio_amd", "csrc", "sets.hip")
    assert sets.count("int sets_build_spans(") == 1 and sets.count("k_sets_rows, dim3") == 1 and sets.count("segmented_radix_sort_keys(tmp") == 2
    assert "sets_build_spans(ctx, SpanSrc{r->hash, r->refs, r->wfirst, r->wcount, r->n," in sets  # the three old entries: the result's own arrays
    assert "struct SpanSrc {" in _read("bio_amd", "csrc", "sets_internal.hpp")
    internal = _read("bio_amd", "csrc", "search_internal.hpp")
    for field in ("*members", "c_members", "bool has_members = false"):
        assert field in internal, field
    slots = {k: int(v) for k, v in re.findall(r"\b(SLOT_\w+|POOL_SLOTS) = (\d+)", _read("bio_amd", "csrc", "host_types.hpp"))}
    mine = [slots[k] for k in ("SLOT_WIN_SEQS", "SLOT_WIN_SPANS", "SLOT_FOLD_MAP", "SLOT_FOLD_WORK")]
    assert len(set(mine)) == 4 and all(v < slots["POOL_SLOTS"] for v in mine)
    assert not [k for k, v in slots.items() if v in mine and not k.startswith(("SLOT_WIN_", "SLOT_FOLD_"))]  # shared with nobody


def test_whoever_clears_the_totals_clears_the_members():
    for path in (("bio_amd", "csrc", "search.hip"), ("bio_amd", "csrc", "compare.hip"), ("bio_amd", "csrc", "fold.hip")):
        lines = _read(*path).splitlines()
        cleared = [k for k, ln in enumerate(lines) if re.search(r"\bres->has_total = false;", ln)]
        assert cleared, path
        for k in cleared:
            assert re.search(r"\bres->has_members = false;", lines[k + 2]), (path, k + 2, lines[k])
    assert "hipFree(h->members)" in _read("bio_amd", "csrc", "search.hip")
    assert "has_members" not in _read("bio_amd", "csrc", "pipeline.cpp")  # the sink goes through bsk_index_search and bsk_hits_top


def test_the_checks_come_in_the_contracts_order():
    """without a context the argument checks cannot be told apart, so their order is read from the source: nothing touches the device before
    them, and the pass that refuses unsorted rows and targets beyond the groups runs before the slot is taken over"""
    src = _read("bio_amd", "csrc", "windows.hip")
    body = src[src.index('extern "C" int bsk_result_sets_windows('):]
    at = [body.index(x) for x in ("null argument", "exactly one of window and count", "step > window", "window >= 2^31", "unknown flag", "bad scale", "another context",
                                  "take_over(")]
    assert at == sorted(at) and "hip" not in body[:body.index("take_over(")]
    impl = src[src.index("int windows_impl("):src.index('extern "C" int bsk_result_sets_windows(')]
    at = [impl.index(x) for x in ("hipSetDevice", "k_win_count", "scan_counts(", "read_back(", "2^32 windows or more", "BSK_ERR_UNSUPPORTED", "k_win_spans", "sets_build_spans(")]
    assert at == sorted(at)
    src = _read("bio_amd", "csrc", "fold.hip")
    body = src[src.index('extern "C" int bsk_hits_fold('):src.index('extern "C" int bsk_hits_members_device(')]
    at = [body.index(x) for x in ("null argument", "unknown flag", "frac_num > frac_den", "another context", "*out is h itself", "2^32 groups or more", "group_offsets[0] != 0",
                                  "group_offsets decrease", "more than 2^32 targets", "BSK_ERR_UNSUPPORTED", "hipSetDevice", "k_fold_map", "k_fold_check", "read_back(",
                                  "a target >= group_offsets[n_groups]", "not strictly ascending", "take_over(")]
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
    hidden = "|".join(WIN_KERNELS + FOLD_KERNELS + ("windows_impl", "fold_impl", "fold_scratch", "FoldScratch", "sets_build_spans", "SpanSrc", "WinRule", "FoldRule"))
    assert not re.findall(r" [TW] (\S*(?:%s)\S*)" % hidden, out)  # the helpers stay inside the library
    declared = set(re.findall(r"\b(bsk_\w+)\(", _norm(_read("include", "biosketch.h"))))
    assert exported <= declared, exported - declared  # the header's entries and no more
    assert {s for s in exported if "windows" in s or "fold" in s or "members" in s} == set(ENTRIES)


def test_null_and_bad_arguments_without_a_device(lib):
    from bio_amd import _lib as L
    fake = C.create_string_buffer(2048)  # zeroed: a result / hits of no context and nothing in it -- every case below fails its checks first
    fp = C.addressof(fake)
    out = C.c_void_p(4321)
    wp = L.WindowParams(7, 0, 0, 0)
    so = np.full(4, 7, np.uint64)
    for ctx, r, w in ((None, None, wp), (None, fp, wp), (None, fp, None)):
        assert lib.bsk_result_sets_windows(ctx, r, C.byref(w) if w is not None else None, 1, C.byref(out), so.ctypes.data) == L.ERR_ARG and out.value == 4321
    assert lib.bsk_result_sets_windows(None, fp, C.byref(wp), 1, None, None) == L.ERR_ARG
    for bad in (L.WindowParams(0, 0, 0, 0), L.WindowParams(7, 0, 3, 0), L.WindowParams(7, 8, 0, 0), L.WindowParams(0, 1, 3, 0), L.WindowParams(2**31, 0, 0, 0),
                L.WindowParams(7, 0, 0, 2), L.WindowParams(7, 0, 0, 0x80000000)):
        assert lib.bsk_result_sets_windows(None, fp, C.byref(bad), 1, C.byref(out), so.ctypes.data) == L.ERR_ARG and out.value == 4321
    assert lib.bsk_result_sets_windows(None, fp, C.byref(wp), -1, C.byref(out), so.ctypes.data) == L.ERR_ARG and out.value == 4321 and list(so) == [7] * 4
    go = np.array([0, 2, 5], np.uint64)
    for ctx, h, g in ((None, None, go), (None, fp, go), (None, fp, None)):
        assert lib.bsk_hits_fold(ctx, h, g.ctypes.data if g is not None else None, 2, None, C.byref(out)) == L.ERR_ARG and out.value == 4321
    assert lib.bsk_hits_fold(None, fp, go.ctypes.data, 2, None, None) == L.ERR_ARG
    for bad in (L.FoldParams(1, 1, 0, 0), L.FoldParams(1, 0x80000000, 0, 0), L.FoldParams(1, 0, 3, 2)):
        assert lib.bsk_hits_fold(None, fp, go.ctypes.data, 2, C.byref(bad), C.byref(out)) == L.ERR_ARG and out.value == 4321
    p = C.c_void_p(55)
    assert lib.bsk_hits_members_device(None, C.byref(p)) == L.ERR_ARG and p.value == 55
    assert lib.bsk_hits_members_device(fp, C.byref(p)) == L.OK and p.value is None  # hits without members
    assert lib.bsk_hits_members_device(fp, None) == L.OK
    buf = np.full(4, 7, np.uint32)
    assert lib.bsk_hits_fetch_members(None, fp, 0, 0, buf.ctypes.data, 4) == L.ERR_ARG
    assert lib.bsk_hits_fetch_members(None, None, 0, 0, buf.ctypes.data, 4) == L.ERR_ARG and list(buf) == [7] * 4
