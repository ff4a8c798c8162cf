"""CPU: the grid cap's test aid (bsk_ctx_grid_stats) -- declared with its prototype beside bsk_ctx_reload_options, bound by bio_amd._lib,
exported by the library, refusing null arguments without a device; and that the sets side sizes no grid from the CU count itself."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bio_amd", "csrc")
PROTO = "int bsk_ctx_grid_stats(const bsk_ctx *ctx, uint64_t out[2]);"


def _norm(s):
    s = re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    return re.sub(r"\s+", " ", s).strip()


@pytest.fixture(scope="module")
def lib():
    from bio_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_header_declares_it_and_python_binds_it():
    from bio_amd import _lib
    raw = open(os.path.join(ROOT, "include", "biosketch.h")).read()
    hdr = _norm(raw)
    assert PROTO in hdr
    assert hdr.index("int bsk_ctx_reload_options(") < hdr.index("int bsk_ctx_grid_stats(") < hdr.index("int bsk_build_has_experiments(")
    assert "BSK_GRID_CAP" in raw[raw.index("int bsk_ctx_reload_options("):raw.index("int bsk_ctx_grid_stats(")]  # the comment names the switch
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    res, args = bound["bsk_ctx_grid_stats"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(C.c_uint64)]


def test_library_exports_it(lib):
    from bio_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T bsk_ctx_grid_stats$", out, re.M)
    assert not re.findall(r" [TW] (\S*(?:capped_grid|grid_cap_blocks|grid_for)\S*)", out)  # the helpers stay inside the library


def test_null_arguments_without_a_device(lib):
    from bio_amd import _lib as L
    out = (C.c_uint64 * 2)(7, 7)
    fake = C.create_string_buffer(64)
    assert lib.bsk_ctx_grid_stats(None, out) == L.ERR_ARG and list(out) == [7, 7]
    assert lib.bsk_ctx_grid_stats(None, None) == L.ERR_ARG
    assert lib.bsk_ctx_grid_stats(C.addressof(fake), None) == L.ERR_ARG  # (the context is not looked at before the check)


def test_no_sets_side_unit_sizes_a_grid_from_the_cu_count_itself():
    """the switch is read where the others are, and no translation unit of the sets side looks at the CU count: their grids can only come
    from the helper in host_types.hpp.  (Of the sketch side only the planned kernels' own grids stay off it -- planner.hip and the unit
    grids beside it keep ctx->cus; the small passes there call grid_for(ctx, items, block), which goes through the helper too.)"""
    src = {fn: re.sub(r"//.*", "", open(os.path.join(CSRC, fn)).read()) for fn in os.listdir(CSRC) if fn.endswith((".hip", ".hpp", ".cpp"))}
    bio = src["biosketch.hip"]
    assert '"BSK_GRID_CAP"' in bio[bio.index("void BskOpts::load()"):bio.index('extern "C" int bsk_build_has_experiments')]
    for fn in ("sets.hip", "setops.hip", "counts.hip", "compare.hip", "search.hip", "cluster.hip", "sets_internal.hpp"):
        assert "->cus" not in src[fn], fn
