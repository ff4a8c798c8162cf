"""CPU: the unit-grid switch's test aid (bsk_ctx_unit_grid_stats) -- declared with its prototype behind bsk_ctx_grid_stats, bound by
bio_amd._lib, exported by the library, refusing null arguments without a device; the switch is read where the others are, its helper stays
inside the library and keeps counters of its own."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bio_amd", "csrc")
PROTO = "int bsk_ctx_unit_grid_stats(const bsk_ctx *ctx, uint64_t out[2]);"


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
    assert hdr.index("int bsk_ctx_grid_stats(") < hdr.index("int bsk_ctx_unit_grid_stats(") < hdr.index("int bsk_build_has_experiments(")
    assert "BSK_UNIT_GRID" in raw[raw.index("int bsk_ctx_grid_stats("):raw.index("int bsk_ctx_unit_grid_stats(")]  # the comment names the switch
    bound = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    res, args = bound["bsk_ctx_unit_grid_stats"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(C.c_uint64)]


def test_library_exports_it(lib):
    from bio_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T bsk_ctx_unit_grid_stats$", out, re.M)
    assert not [s for s in re.findall(r" [TW] (\S*unit_grid\S*)", out) if s != "bsk_ctx_unit_grid_stats"]  # the helper stays inside the library


def test_null_arguments_without_a_device(lib):
    from bio_amd import _lib as L
    out = (C.c_uint64 * 2)(7, 7)
    fake = C.create_string_buffer(64)
    assert lib.bsk_ctx_unit_grid_stats(None, out) == L.ERR_ARG and list(out) == [7, 7]
    assert lib.bsk_ctx_unit_grid_stats(None, None) == L.ERR_ARG
    assert lib.bsk_ctx_unit_grid_stats(C.addressof(fake), None) == L.ERR_ARG  # (the context is not looked at before the check)


def test_switch_is_read_once_and_the_helper_keeps_its_own_counters():
    src = {fn: re.sub(r"//.*", "", open(os.path.join(CSRC, fn)).read()) for fn in os.listdir(CSRC) if fn.endswith((".hip", ".hpp", ".cpp"))}
    bio = src["biosketch.hip"]
    assert '"BSK_UNIT_GRID"' in bio[bio.index("void BskOpts::load()"):bio.index('extern "C" int bsk_build_has_experiments')]
    assert sum(s.count('"BSK_UNIT_GRID"') for s in src.values()) == 1  # nowhere else: never on the bsk_sketch path
    ht = src["host_types.hpp"]
    helper = ht[ht.index("static inline unsigned unit_grid("):ht.index("int grid_for(")]
    assert "unit_grid_stats[0]" in helper and "unit_grid_stats[1]" in helper and "->grid_stats" not in helper  # bsk_ctx_grid_stats' figures are held exactly elsewhere
    assert "ctx->opt.unit_grid ?" in helper and ": want;" in helper  # unset: the caller's own size, untouched
    stats = bio[bio.index('extern "C" int bsk_ctx_unit_grid_stats('):]
    stats = stats[:stats.index("\n}\n")]
    assert "ctx->side ? ctx->side->unit_grid_stats[i] : 0" in stats  # the side context's launches count
