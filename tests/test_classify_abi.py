"""CPU: the read-classification entries of include/biosketch.h -- bsk_index_attach, bsk_hits_top, the hits sink's two open calls and
bsk_chunk_hits -- declared with the contract's signatures, bound by bio_amd._lib, called from the Go shim, and their argument checks as
far as they run without a device."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "bsk_index_attach": "int bsk_index_attach(bsk_ctx *ctx, const bsk_index *ix, bsk_index **handle);",
    "bsk_hits_top": "int bsk_hits_top(bsk_ctx *ctx, const bsk_hits *h, uint32_t n, bsk_hits **top);",
    "bsk_pipeline_open_fastx_search": "int bsk_pipeline_open_fastx_search(const bsk_pipeline_config *cfg, const char *const *paths, int n_paths, "
                                      "const bsk_params *p, const bsk_pipeline_search *s, bsk_pipeline **out);",
    "bsk_pipeline_open_memory_search": "int bsk_pipeline_open_memory_search(const bsk_pipeline_config *cfg, const uint8_t *bytes, const uint64_t *offsets, "
                                       "uint64_t n, int repeat, const bsk_params *p, const bsk_pipeline_search *s, bsk_pipeline **out);",
    "bsk_chunk_hits": "int bsk_chunk_hits(const bsk_chunk *c, const uint32_t **target, const uint32_t **shared);",
}


def _norm(s):
    s = re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    return re.sub(r"\s+", " ", s).replace("( ", "(").replace(" )", ")").replace(" ;", ";").replace(" ,", ",").strip()


def _header():
    return _norm(open(os.path.join(ROOT, "include", "biosketch.h")).read())


def test_header_declares_the_classify_entries():
    hdr = _header()
    for name, proto in ENTRIES.items():
        assert _norm(proto) in hdr, name
    body = re.search(r"typedef struct bsk_pipeline_search \{(.*?)\} bsk_pipeline_search;", hdr).group(1)
    assert [(t.strip(), n) for t, n in re.findall(r"([\w ]+?) \*?(\w+);", body)] == [("const bsk_index", "index"), ("bsk_search_params", "params"), ("uint32_t", "top_n"),
                                                       ("uint32_t", "reserved")]
    assert "enum { BSK_SINK_HITS = 3 };" in hdr
    assert "#define BSK_ABI_VERSION 1" in hdr
    # the frozen structs are as they were
    cfg = re.search(r"typedef struct bsk_pipeline_config \{(.*?)\} bsk_pipeline_config;", hdr).group(1)
    assert re.findall(r"(\w+);", cfg) == ["devices", "n_devices", "n_streams", "chunk_records", "sink", "sets_scale", "alphabet", "host_checksum", "n_readers",
                                          "reserved"]
    chunk = re.search(r"typedef struct bsk_chunk \{(.*?)\} bsk_chunk;", hdr).group(1)
    assert re.findall(r"(\w+);", chunk) == ["sequence", "source_index", "device", "first_record", "n_tuples", "n_values", "checksum", "link_bytes", "has_pos",
                                            "offsets32", "offsets64", "status", "hash", "pos16", "pos32", "opaque"]


def test_python_binds_and_go_calls_them():
    from bio_amd import _lib
    bound = {n for n, _, _ in _lib.SYMBOLS}
    go = "".join(open(f).read() for f in glob.glob(os.path.join(ROOT, "bindings", "go", "sketches", "*.go")))
    for name in ENTRIES:
        assert name in bound, name
        assert f"C.{name}(" in go, name
    assert _lib.SINK_HITS == 3
    assert C.sizeof(_lib.PipelineSearch) == 40 and _lib.PipelineSearch.params.offset == 8 and _lib.PipelineSearch.top_n.offset == 32
    assert C.sizeof(_lib.PipelineConfig) == 48 and C.sizeof(_lib.Chunk) == 136  # frozen
    from bio_amd import sketches as S
    import inspect
    for cls, attrs in ((S.Index, ("attach",)), (S.Hits, ("top",))):
        for a in attrs:
            assert hasattr(cls, a), (cls, a)
    sig = inspect.signature(S.Engine.pipeline_open).parameters
    assert sig["search"].default is None and sig["top_n"].default == 0 and sig["min_shared"].default == 1  # "no search" unless asked for
    hpp = open(os.path.join(ROOT, "bio_amd", "csrc", "sketches.hpp")).read()
    for name in ("bsk_index_attach", "bsk_hits_top", "bsk_pipeline_open_memory_search", "bsk_chunk_hits"):
        assert name + "(" in hpp, name


@pytest.fixture(scope="module")
def lib():
    from bio_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_null_and_bad_arguments_without_a_device(lib):
    from bio_amd import _lib as L
    out = C.c_void_p(1234)
    assert lib.bsk_index_attach(None, None, C.byref(out)) == L.ERR_ARG and out.value is None
    assert lib.bsk_index_attach(None, None, None) == L.ERR_ARG
    top = C.c_void_p()
    assert lib.bsk_hits_top(None, None, 0, C.byref(top)) == L.ERR_ARG and not top.value
    assert lib.bsk_hits_top(None, None, 1, C.byref(top)) == L.ERR_ARG and not top.value
    assert lib.bsk_hits_top(None, None, 1, None) == L.ERR_ARG

    data = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTACGT", np.uint8).copy()
    offs = np.array([0, 32], np.uint64)
    p = L.Params(L.MINIMIZER, 21, 11, 0, 0, 0, 1, 0, 1, 1)
    dev = (C.c_int * 1)(0)
    fake_index = C.create_string_buffer(256)  # never read: every case below fails its checks first
    paths = (C.c_char_p * 1)(b"/nonexistent.fq")

    def opens(sink=L.SINK_HITS, index=C.addressof(fake_index), reserved=0, sp_reserved=0, qcov=0.0, scale=1, null_search=False):
        cfg = L.PipelineConfig(dev, 1, 1, 100, sink, scale, L.ALPHA_DNA, 0, 0, 0)
        s = L.PipelineSearch(index, L.SearchParams(1, sp_reserved, qcov, 0.0), 1, reserved)
        sp = None if null_search else C.byref(s)
        rcs = []
        for call in (lambda h: lib.bsk_pipeline_open_memory_search(C.byref(cfg), data.ctypes.data, offs.ctypes.data, 1, 1, C.byref(p), sp, C.byref(h)),
                     lambda h: lib.bsk_pipeline_open_fastx_search(C.byref(cfg), paths, 1, C.byref(p), sp, C.byref(h))):
            h = C.c_void_p(77)
            rcs.append(call(h))
            assert h.value is None
        return rcs

    for sink in (L.SINK_COUNTS, L.SINK_TUPLES, L.SINK_SETS, 4):
        assert opens(sink=sink) == [L.ERR_ARG] * 2, sink
    assert opens(index=None) == [L.ERR_ARG] * 2
    assert opens(reserved=1) == [L.ERR_ARG] * 2
    assert opens(sp_reserved=1) == [L.ERR_ARG] * 2
    assert opens(qcov=1.5) == [L.ERR_ARG] * 2
    assert opens(qcov=float("nan")) == [L.ERR_ARG] * 2
    assert opens(scale=-1) == [L.ERR_ARG] * 2
    assert opens(null_search=True) == [L.ERR_ARG] * 2
    assert lib.bsk_pipeline_open_memory_search(None, None, None, 0, 1, None, None, None) == L.ERR_ARG
    # the plain open calls still refuse the hits sink
    cfg = L.PipelineConfig(dev, 1, 1, 100, L.SINK_HITS, 1, L.ALPHA_DNA, 0, 0, 0)
    h = C.c_void_p(77)
    assert lib.bsk_pipeline_open_memory(C.byref(cfg), data.ctypes.data, offs.ctypes.data, 1, 1, C.byref(p), C.byref(h)) == L.ERR_ARG and h.value is None
    h = C.c_void_p(77)
    assert lib.bsk_pipeline_open_fastx(C.byref(cfg), paths, 1, C.byref(p), C.byref(h)) == L.ERR_ARG and h.value is None
    # bsk_chunk_hits: NULL, and a chunk of another sink
    t, s = C.c_void_p(5), C.c_void_p(5)
    assert lib.bsk_chunk_hits(None, C.byref(t), C.byref(s)) == L.ERR_ARG and t.value is None and s.value is None
    for sink in (L.SINK_COUNTS, L.SINK_TUPLES, L.SINK_SETS):
        c = L.Chunk()
        c.sink = sink
        c.opaque = C.addressof(fake_index)
        assert lib.bsk_chunk_hits(C.byref(c), C.byref(t), C.byref(s)) == L.ERR_ARG
    lib.bsk_index_release(None)
