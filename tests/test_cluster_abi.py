"""CPU: the entries of the clusters of a hits graph (bsk_hits_cluster, bsk_clusters_*, bsk_hits_from_host) -- declared with the contract's
prototypes between bsk_sets_sumsq and the neighbours block, bound by bio_amd._lib, called from the Go shim and the C++ owners, exported by
the library and nothing else with them, built where the build expects them, and their argument checks as far as they run without a device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "bsk_hits_cluster": "int bsk_hits_cluster(bsk_ctx *ctx, const bsk_hits *h, const bsk_cluster_params *cp, const uint64_t *score, bsk_clusters **out);",
    "bsk_clusters_info": "int bsk_clusters_info(const bsk_clusters *c, uint64_t *n_items, uint64_t *n_clusters, uint64_t *largest);",
    "bsk_clusters_plan": "int bsk_clusters_plan(const bsk_clusters *c, const char **plan, uint64_t figures[2]);",
    "bsk_clusters_fetch": "int bsk_clusters_fetch(bsk_ctx *ctx, const bsk_clusters *c, uint32_t *label, uint32_t *rep, uint64_t *offsets, uint32_t *members);",
    "bsk_clusters_device": "int bsk_clusters_device(const bsk_clusters *c, const uint32_t **label, const uint32_t **rep, const uint64_t **offsets, "
                           "const uint32_t **members);",
    "bsk_clusters_release": "void bsk_clusters_release(bsk_clusters *c);",
    "bsk_hits_from_host": "int bsk_hits_from_host(bsk_ctx *ctx, const uint64_t *offsets, uint64_t n_queries, const uint32_t *target, const uint32_t *shared, "
                          "const uint32_t *total, bsk_hits **hits);",
}
ARITY = dict(bsk_hits_cluster=5, bsk_clusters_info=4, bsk_clusters_plan=3, bsk_clusters_fetch=6, bsk_clusters_device=5, bsk_clusters_release=1, bsk_hits_from_host=7)
KERNELS = ("k_cl_check", "k_cl_score_keys", "k_cl_class_keys", "k_cl_ranks", "k_cl_edges", "k_cl_init", "k_cl_hook", "k_cl_jump", "k_cl_mis_scan", "k_cl_mis_apply",
           "k_cl_assign", "k_cl_rep", "k_cl_label", "k_cl_member_keys", "k_cl_members")


def _norm(s):
    s = re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    return re.sub(r"\s+", " ", s).replace("( ", "(").replace(" )", ")").replace(" ;", ";").replace(" ,", ",").strip()


def test_header_declares_the_entries_in_their_place():
    raw = open(os.path.join(ROOT, "include", "biosketch.h")).read()
    hdr = _norm(raw)
    for name, proto in ENTRIES.items():
        assert _norm(proto) in hdr, name
    assert "enum { BSK_CLUSTER_COMPONENTS = 0, BSK_CLUSTER_GREEDY = 1 };" in hdr and "#define BSK_ABI_VERSION 1" in hdr
    assert _norm("typedef struct bsk_cluster_params { uint32_t method; uint32_t flags; } bsk_cluster_params;") in hdr
    assert "typedef struct bsk_clusters bsk_clusters;" in hdr
    # after bsk_sets_sumsq, before the neighbours block, which still closes the header
    order = ["int bsk_sets_sumsq(", "enum { BSK_CLUSTER_COMPONENTS", "typedef struct bsk_cluster_params", "int bsk_hits_cluster(", "int bsk_clusters_info(",
             "int bsk_clusters_plan(", "int bsk_clusters_fetch(", "int bsk_clusters_device(", "void bsk_clusters_release(", "int bsk_hits_from_host(",
             "enum { BSK_NEIGHBORS_UPPER", "int bsk_sets_neighbors(", "int bsk_hits_fetch_totals("]
    at = [hdr.index(x) for x in order]
    assert at == sorted(at)
    assert raw.index("int bsk_sets_sumsq(") < raw.index("/* ---- clusters of a neighbour graph") < raw.index("/* ---- sparse all-pairs comparison")
    block = raw[raw.index("/* ---- clusters of a neighbour graph"):raw.index("/* ---- sparse all-pairs comparison")]
    for said in ("declared below this block", "UNDIRECTED", "repeated directions", "BSK_NEIGHBORS_UPPER", "target >= n", "ties go to the smaller index", "NOT transitive",
                 "cd-hit", "ascending by index", "bit-identical", "2^32", "n == 0", "The result slot", "n + 1", "n ROUNDS", "k_cl_hook", "k_cl_jump", "k_cl_mis_scan",
                 "k_cl_mis_apply", "32-bit atomics", "nothing reads", "earlier launch", "spins", "edges=", "rounds=", "from host", "strictly ascending", "not retained"):
        assert said in block, said
    slot = raw[raw.index("/* The result slot."):raw.index("int bsk_result_sets_reuse(")]
    assert "bsk_hits_cluster" in slot and "bsk_hits_from_host" in slot


def test_python_binds_go_and_cpp_call_them():
    from bio_amd import _lib
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    go = open(os.path.join(ROOT, "bindings", "go", "sketches", "cluster.go")).read()
    hpp = open(os.path.join(ROOT, "bio_amd", "csrc", "sketches.hpp")).read()
    for name in ENTRIES:
        assert name in bound and len(bound[name][1]) == ARITY[name], name
        assert bound[name][0] is (None if name == "bsk_clusters_release" else C.c_int), name
        assert f"C.{name}(" in go, name
        assert name + "(" in hpp or name + ">" in hpp, name
    assert bound["bsk_hits_from_host"][1][2] is C.c_uint64
    assert [f for f, _ in _lib.ClusterParams._fields_] == ["method", "flags"] and all(t is C.c_uint32 for _, t in _lib.ClusterParams._fields_)
    assert C.sizeof(_lib.ClusterParams) == 8 and (_lib.CLUSTER_COMPONENTS, _lib.CLUSTER_GREEDY) == (0, 1)
    for m in ("func (h *Hits) Cluster(p ClusterParams, score []uint64, reuse *Clusters) (*Clusters, error)", "type ClusterParams struct", "type Clusters struct",
              "func (r *Clusters) Info(", "func (r *Clusters) Plan(", "func (r *Clusters) Fetch(", "func (r *Clusters) Release(", "func (e *Engine) HitsFromHost(",
              "C.BSK_CLUSTER_COMPONENTS", "C.BSK_CLUSTER_GREEDY"):
        assert m in go, m
    for m in ("class Clusters : public Owned<bsk_clusters, bsk_clusters_release>", "int cluster(Engine &e, uint32_t method", "hits_from_host(", "int from_host(Engine &e"):
        assert m in hpp, m
    from bio_amd import sketches as S
    sig = inspect.signature(S.Hits.cluster).parameters
    assert list(sig) == ["self", "method", "score", "reuse"] and [sig[k].default for k in list(sig)[1:]] == ["components", None, None]
    sig = inspect.signature(S.Engine.hits_from_arrays).parameters
    assert list(sig)[:5] == ["self", "offsets", "target", "shared", "total"] and sig["total"].default is None
    for attr in ("info", "plan", "fetch"):
        assert callable(getattr(S.Clusters, attr))
    for attr in ("label", "rep", "offsets", "members", "sizes"):
        assert isinstance(getattr(S.Clusters, attr), property), attr
    assert S.Clusters._release == "bsk_clusters_release"


def test_the_kernels_live_where_the_build_expects_them():
    mk = open(os.path.join(ROOT, "bio_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS =.*\bcluster\.o\b", mk, re.M) and re.search(r"cluster\.o:.*sets_internal\.hpp.*search_internal\.hpp", mk)
    assert re.search(r"^test_cluster:.*tests/cpp/test_cluster\.cpp", mk, re.M) and re.search(r"^\trm -f .*\btest_cluster\b", mk, re.M)
    assert '"test_cluster"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "bio_amd/csrc/test_cluster" in open(os.path.join(ROOT, ".gitignore")).read().split()
    src = open(os.path.join(ROOT, "bio_amd", "csrc", "cluster.hip")).read()
    for k in KERNELS:
        assert f"void {k}(" in src, k
    code = re.sub(r"//.*", "", src)
    assert "sets_sort_u64(" in code and "scan_counts(" in code and "rocprim" not in code and "asm" not in code  # no new sort instantiation, no assembly
    for banned in ("atomicCAS", "atomicExch", "while (", "__threadfence", "volatile", "double", "float"):
        assert banned not in code, banned  # bounded loops, integers, no retry and no wait on another workgroup
    assert "struct bsk_clusters {" in open(os.path.join(ROOT, "bio_amd", "csrc", "search_internal.hpp")).read()
    assert 'extern "C" int bsk_hits_from_host(' in open(os.path.join(ROOT, "bio_amd", "csrc", "search.hip")).read()
    types = open(os.path.join(ROOT, "bio_amd", "csrc", "host_types.hpp")).read()
    slots = {k: int(v) for k, v in re.findall(r"\b(SLOT_\w+|POOL_SLOTS) = (\d+)", types)}
    mine = [slots[k] for k in ("SLOT_CLUSTER_NODES", "SLOT_CLUSTER_EDGES", "SLOT_CLUSTER_SORT")]
    assert len(set(mine)) == 3 and all(v < slots["POOL_SLOTS"] for v in mine)
    assert not [k for k, v in slots.items() if v in mine and not k.startswith("SLOT_CLUSTER_")]  # shared with nobody


def test_the_checks_come_in_the_contracts_order():
    """without a context the argument checks cannot be told apart, so their order is read from the source: nothing touches the device before them,
    and the pass that refuses a target >= n runs before the slot is taken over"""
    src = open(os.path.join(ROOT, "bio_amd", "csrc", "cluster.hip")).read()
    body = src[src.index('extern "C" int bsk_hits_cluster('):]
    body = body[:body.index('extern "C" int bsk_clusters_info(')]
    at = [body.index(x) for x in ("null argument", "unknown method", "unknown flag", "another context", "BSK_ERR_UNSUPPORTED", "hipSetDevice", "k_cl_check", "read_back(",
                                  "a target >= n_queries", "take_over(")]
    assert at == sorted(at)
    src = open(os.path.join(ROOT, "bio_amd", "csrc", "search.hip")).read()
    body = src[src.index('extern "C" int bsk_hits_from_host('):]
    body = body[:body.index("static int search_impl(")]
    at = [body.index(x) for x in ("null argument", "another context", "offsets[0] != 0", "offsets decrease", "null target or shared", "strictly ascending", "take_over(",
                                  "hipSetDevice", "from host")]
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
    hidden = "|".join(KERNELS + ("cluster_impl", "cl_scratch", "ClScratch", "IsRep", "cl_row_of"))
    assert not re.findall(r" [TW] (\S*(?:%s)\S*)" % hidden, out)  # the helpers stay inside the library
    declared = set(re.findall(r"\b(bsk_\w+)\(", _norm(open(os.path.join(ROOT, "include", "biosketch.h")).read())))
    assert exported <= declared, exported - declared  # the header's entries and no more
    assert {s for s in exported if "cluster" in s} | {"bsk_hits_from_host"} == set(ENTRIES)


def test_null_and_bad_arguments_without_a_device(lib):
    from bio_amd import _lib as L
    fake = C.create_string_buffer(1024)  # zeroed: a bsk_hits / bsk_clusters of no context and nothing in it -- every case below fails its checks first
    fp = C.addressof(fake)
    out = C.c_void_p(4321)
    for ctx, h in ((None, None), (None, fp)):
        assert lib.bsk_hits_cluster(ctx, h, None, None, C.byref(out)) == L.ERR_ARG and out.value == 4321  # an argument error leaves *out
    assert lib.bsk_hits_cluster(None, fp, None, None, None) == L.ERR_ARG
    for bad in (L.ClusterParams(2, 0), L.ClusterParams(0, 1), L.ClusterParams(1, 0x80000000), L.ClusterParams(0xFFFFFFFF, 0)):
        assert lib.bsk_hits_cluster(None, fp, C.byref(bad), None, C.byref(out)) == L.ERR_ARG and out.value == 4321
    n = (C.c_uint64 * 3)(7, 7, 7)
    assert lib.bsk_clusters_info(None, n, None, None) == L.ERR_ARG and list(n) == [7, 7, 7]
    assert lib.bsk_clusters_info(fp, C.cast(C.byref(n, 0), C.POINTER(C.c_uint64)), C.cast(C.byref(n, 8), C.POINTER(C.c_uint64)),
                                 C.cast(C.byref(n, 16), C.POINTER(C.c_uint64))) == L.OK and list(n) == [0, 0, 0]
    assert lib.bsk_clusters_info(fp, None, None, None) == L.OK
    p, f = C.c_char_p(b"x"), (C.c_uint64 * 2)(5, 5)
    assert lib.bsk_clusters_plan(None, C.byref(p), f) == L.ERR_ARG and p.value == b"x" and list(f) == [5, 5]
    assert lib.bsk_clusters_plan(fp, C.byref(p), f) == L.OK and p.value == b"" and list(f) == [0, 0]
    assert lib.bsk_clusters_plan(fp, None, None) == L.OK
    ptrs = [C.c_void_p(55) for _ in range(4)]
    assert lib.bsk_clusters_device(None, *[C.byref(x) for x in ptrs]) == L.ERR_ARG and all(x.value == 55 for x in ptrs)
    assert lib.bsk_clusters_device(fp, *[C.byref(x) for x in ptrs]) == L.OK and all(x.value is None for x in ptrs)
    assert lib.bsk_clusters_device(fp, None, None, None, None) == L.OK
    buf = np.full(4, 7, np.uint32)
    assert lib.bsk_clusters_fetch(None, fp, buf.ctypes.data, None, None, None) == L.ERR_ARG
    assert lib.bsk_clusters_fetch(None, None, buf.ctypes.data, None, None, None) == L.ERR_ARG and list(buf) == [7] * 4
    lib.bsk_clusters_release(None)


def test_hits_from_host_checks_its_arrays_on_the_host(lib):
    """null arguments and the three host checks (descending offsets, an unsorted row, a repeated target): BSK_ERR_ARG with the slot as it was.  Without a
    context every call here is refused whatever its arrays hold, so the texts are read from the source; tests/test_gpu_cluster.py repeats the calls with a
    context, where good arrays pass"""
    from bio_amd import _lib as L
    U64, U32 = np.uint64, np.uint32
    slot = C.c_void_p(4321)
    sh = np.ones(4, U32)
    for offsets, target in (([0, 2, 1], [1, 2]), ([0, 2, 2], [2, 1]), ([0, 2, 2], [1, 1]), ([1, 2, 2], [1, 2]), ([0, 1, 2], [0, 1])):
        o, t = np.array(offsets, U64), np.array(target, U32)
        assert lib.bsk_hits_from_host(None, o.ctypes.data, 2, t.ctypes.data, sh.ctypes.data, None, C.byref(slot)) == L.ERR_ARG and slot.value == 4321
    o = np.array([0, 1, 2], U64)
    assert lib.bsk_hits_from_host(None, None, 2, None, None, None, C.byref(slot)) == L.ERR_ARG and slot.value == 4321
    assert lib.bsk_hits_from_host(None, o.ctypes.data, 2, None, None, None, None) == L.ERR_ARG
    src = open(os.path.join(ROOT, "bio_amd", "csrc", "search.hip")).read()
    body = src[src.index('extern "C" int bsk_hits_from_host('):]
    body = body[:body.index("take_over(")]
    assert "offsets[q + 1] < offsets[q]" in body and "target[i] <= target[i - 1]" in body and "hip" not in body.replace("hits", "")  # host code only
