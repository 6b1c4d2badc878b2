"""CPU-side checks of the bfloat16 feature path (gnx_block_forward_typed): the two entries are declared, exported and bound, the element
code, validation before any GPU work, no host fallback without a GPU, the run-time kernel source with the bf16 key compiles for gfx950, and
GNBlock's dtype checks run before any library call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_block_typed_workspace_bytes", "gnx_block_forward_typed", "gnx_jit_precompile_typed")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    return gn._lib.load()


def _header():
    with open(os.path.join(ROOT, "include", "gnx.h")) as f:
        return f.read()


def test_typed_entries_declared_exported_and_bound(lib):
    import graphnets_jl_amd as gn
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        m = re.search(r"GNX_API [\w\s\*]+?\b" + name + r"\(([^;]*?)\);", text, flags=re.S)
        assert m, f"{name} is not declared in include/gnx.h"
        assert hasattr(lib, name), f"{name} is not exported by libgnx.so"
        assert name in gn._lib.SIGNATURES
        assert m.group(1).count(",") + 1 == len(gn._lib.SIGNATURES[name][1]), name
    assert len(gn._lib.SIGNATURES["gnx_block_forward_typed"][1]) == 14
    assert len(gn._lib.SIGNATURES["gnx_block_typed_workspace_bytes"][1]) == 5
    assert lib.gnx_version() == 130


def test_elem_code():
    import graphnets_jl_amd as gn
    assert re.search(r"#define GNX_ELEM_BF16 5\b", _header())
    assert gn._lib.ELEM_BF16 == 5
    assert len({gn._lib.ELEM_U8, gn._lib.ELEM_I32, gn._lib.ELEM_I64, gn._lib.ELEM_F32, gn._lib.ELEM_F64, gn._lib.ELEM_BF16}) == 6


def _params(gn, dims=(10, 5, 0), out=(3, 4, 5)):
    L = gn._lib
    p = L.BlockParams(*dims, *out)
    w = np.zeros(64, dtype=np.float32)  # (never read: every call below fails before any GPU work)
    p.edgefn.weight = p.nodefn.weight = p.graphfn.weight = w.ctypes.data
    return p, w


def test_bad_elem_and_flags_are_rejected_before_gpu_work(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep = _params(gn)
    buf = np.zeros(16, dtype=np.float32)
    ptr = buf.ctypes.data
    for elem in (-1, 0, 1, 2, 4, 6, 99):
        assert lib.gnx_block_typed_workspace_bytes(None, C.byref(p), 1, elem, 0) == 0
        assert lib.gnx_block_forward_typed(None, C.byref(p), elem, ptr, ptr, ptr, 1, ptr, ptr, ptr, ptr, 64, 0, None) == L.ERR_INVALID_ARG
        assert b"elem" in lib.gnx_last_error()
    # deferring the graph update is not a bf16 form
    assert lib.gnx_block_typed_workspace_bytes(None, C.byref(p), 1, L.ELEM_BF16, L.FLAG_DEFER_GRAPH_UPDATE) == 0
    assert lib.gnx_block_forward_typed(None, C.byref(p), L.ELEM_BF16, ptr, ptr, ptr, 1, ptr, ptr, ptr, ptr, 64, L.FLAG_DEFER_GRAPH_UPDATE,
                                       None) == L.ERR_INVALID_ARG
    assert b"DEFER" in lib.gnx_last_error()
    # a NULL handle is an argument error in both element types, as in gnx_block_forward
    assert lib.gnx_block_typed_workspace_bytes(None, C.byref(p), 1, L.ELEM_BF16, 0) == 0
    for elem in (L.ELEM_F32, L.ELEM_BF16):
        assert lib.gnx_block_forward_typed(None, C.byref(p), elem, ptr, ptr, ptr, 1, ptr, ptr, ptr, ptr, 64, 0, None) == L.ERR_INVALID_ARG
    assert np.all(buf == 0)
    # the adjacency constructors keep rejecting the feature-only element code
    h = C.c_void_p(None)
    nn = (C.c_int64 * 1)(2)
    adj = np.array([[1, 0], [1, 1]], dtype=np.uint16)
    ptrs = (C.c_void_p * 1)(adj.ctypes.data)
    assert lib.gnx_graphs_create_dense(ptrs, nn, 1, L.ELEM_BF16, 1, C.byref(h)) == L.ERR_INVALID_ARG
    assert not h.value


def test_no_silent_cpu_fallback_for_bf16(lib):
    """Without a GPU the handle a well-formed typed call needs cannot be made (a HIP error, > 0), and the typed call on what the constructor
    left fails without writing a byte on the host: there is no CPU path."""
    import torch
    import graphnets_jl_amd as gn
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = gn._lib
    h = C.c_void_p(None)
    nn = (C.c_int64 * 1)(3)
    adj = np.array([[1, 0, 1], [1, 1, 0], [0, 0, 1]], dtype=np.int64)
    ptrs = (C.c_void_p * 1)(adj.ctypes.data)
    assert lib.gnx_graphs_create_dense(ptrs, nn, 1, L.ELEM_I64, 1, C.byref(h)) > 0
    assert not h.value
    p, _keep = _params(gn)
    ef = np.ones(5 * 10, dtype=np.uint16)
    nf = np.ones(3 * 5, dtype=np.uint16)
    out = np.full(64, 0x7fc0, dtype=np.uint16)
    ws = np.zeros(1 << 16, dtype=np.uint8)
    rc = lib.gnx_block_forward_typed(h, C.byref(p), L.ELEM_BF16, ef.ctypes.data, nf.ctypes.data, None, 1, out.ctypes.data, out.ctypes.data,
                                     out.ctypes.data, ws.ctypes.data, ws.size, 0, None)
    assert rc != 0
    assert np.all(out == 0x7fc0) and np.all(ws == 0)


def test_runtime_specialised_bf16_kernel_source_compiles_for_gfx950(lib):
    """The embedded kernel text compiles with hiprtc for an unlisted width set with the bf16 key (odd widths: 2-byte aligned rows), and the
    bf16 key is a code object of its own; ineligible widths and unknown element types are refused."""
    import graphnets_jl_amd as gn
    L = gn._lib
    n_bf, n_f32 = C.c_size_t(0), C.c_size_t(0)
    p = L.BlockParams(7, 3, 3, 5, 1, 3)
    assert lib.gnx_jit_precompile_typed(C.byref(p), 128, L.ELEM_BF16, C.byref(n_bf)) == 0, lib.gnx_last_error()
    assert n_bf.value > 4096
    assert lib.gnx_jit_precompile_typed(C.byref(p), 128, L.ELEM_F32, C.byref(n_f32)) == 0, lib.gnx_last_error()
    assert n_f32.value > 4096 and n_f32.value != n_bf.value
    assert lib.gnx_jit_precompile_typed(C.byref(L.BlockParams(10, 5, 0, 3, 4, 5)), 64, L.ELEM_BF16, C.byref(n_bf)) == 0, lib.gnx_last_error()
    assert lib.gnx_jit_precompile_typed(C.byref(L.BlockParams(40, 3, 2, 5, 6, 1)), 128, L.ELEM_BF16, C.byref(n_bf)) == L.ERR_DIMS
    assert lib.gnx_jit_precompile_typed(C.byref(p), 128, 7, C.byref(n_bf)) == L.ERR_INVALID_ARG


def test_gnblock_mixed_dtypes_raise_before_any_library_call(monkeypatch):
    import torch
    import graphnets_jl_amd as gn

    def no_lib():
        raise AssertionError("the library was called")

    monkeypatch.setattr(gn._lib, "load", no_lib)
    blk = gn.GNBlock((10, 5, 0), (3, 4, 5), device="cpu")
    ef = torch.zeros((10, 6, 1), dtype=torch.bfloat16)
    nf = torch.zeros((5, 3, 1), dtype=torch.float32)
    with pytest.raises(TypeError, match="bfloat16"):
        blk(gn.NT(object(), ef, nf, None))
    with pytest.raises(TypeError, match="bfloat16"):
        blk(gn.NT(object(), ef.float(), nf.to(torch.bfloat16), torch.zeros((2, 1, 1), dtype=torch.float64)))
    # the fp32-only entry points refuse a bf16 tensor instead of reading its bytes as floats
    core = gn.GNCore((10, 5, 3), device="cpu")
    with pytest.raises(TypeError, match="bfloat16"):
        core(gn.NT(object(), ef, nf.to(torch.bfloat16), torch.zeros((3, 1, 1), dtype=torch.bfloat16)))
    with pytest.raises(TypeError, match="bfloat16"):
        gn.logitcrossentropy(torch.zeros((3, 4), dtype=torch.bfloat16), torch.zeros((3, 4), dtype=torch.bfloat16))
    with pytest.raises(TypeError, match="bfloat16"):
        gn.collapsef(gn.NT(object(), ef, None, None))
    with pytest.raises(TypeError, match="bfloat16"):
        gn.padded(gn.NT(object(), ef, None, None))
    with pytest.raises(ValueError):
        gn.batch(dict(graphs=np.eye(2), ef=None, nf=np.zeros((5, 2, 1)), gf=None), device="cpu", dtype=torch.float16)
