"""CPU-side checks of the bfloat16 backward (gnx_block_backward_typed): both entries are declared, exported and bound, unknown element types
are refused before any GPU work without touching the caller's buffers, there is no host fallback without a GPU, and GNBlock's refusal of a
differentiable bf16 call — now naming the `bf16_backward` switch — comes before any library call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_block_backward_typed_workspace_bytes", "gnx_block_backward_typed")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    return gn._lib.load()


def _header():
    with open(os.path.join(ROOT, "include", "gnx.h")) as f:
        return f.read()


def test_typed_backward_entries_declared_exported_and_bound(lib):
    import graphnets_jl_amd as gn
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        m = re.search(r"GNX_API [\w\s\*]+?\b" + name + r"\(([^;]*?)\);", text, flags=re.S)
        assert m, f"{name} is not declared in include/gnx.h"
        assert hasattr(lib, name), f"{name} is not exported by libgnx.so"
        assert name in gn._lib.SIGNATURES
        assert m.group(1).count(",") + 1 == len(gn._lib.SIGNATURES[name][1]), name
    # the fp32 entry's parameters plus `elem`
    assert len(gn._lib.SIGNATURES["gnx_block_backward_typed"][1]) == len(gn._lib.SIGNATURES["gnx_block_backward"][1]) + 1 == 20
    assert len(gn._lib.SIGNATURES["gnx_block_backward_typed_workspace_bytes"][1]) == 4
    assert lib.gnx_version() == 130


def _params(gn, dims=(10, 5, 0), out=(3, 4, 5)):
    L = gn._lib
    p = L.BlockParams(*dims, *out)
    w = np.zeros(64, dtype=np.float32)  # (never read: every call below fails before any GPU work)
    p.edgefn.weight = p.nodefn.weight = p.graphfn.weight = w.ctypes.data
    return p, w


def _call(lib, h, p, elem, ptr, grads, ws):
    return lib.gnx_block_backward_typed(h, C.byref(p), elem, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, 1, ptr, ptr, ptr, C.byref(grads),
                                        ws.ctypes.data, ws.size, None)


def test_bad_elem_is_rejected_before_gpu_work(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep = _params(gn)
    buf = np.full(64, 0x7fc0, dtype=np.uint16)
    gbuf = np.full(256, 7.0, dtype=np.float32)
    ws = np.full(1024, 0x5A, dtype=np.uint8)
    grads = L.BlockGrads(*[L.DenseGrad(gbuf.ctypes.data, gbuf.ctypes.data) for _ in range(3)])
    fake = C.c_void_p(buf.ctypes.data)  # a non-NULL "handle": an unknown elem must be refused before it is looked at
    for elem in (-1, 0, 1, 2, 4, 6, 99):
        for h in (None, fake):
            assert lib.gnx_block_backward_typed_workspace_bytes(h, C.byref(p), 1, elem) == 0
            assert _call(lib, h, p, elem, buf.ctypes.data, grads, ws) == L.ERR_INVALID_ARG
            assert b"elem" in lib.gnx_last_error()
    # a NULL handle is an argument error in both element types, as in gnx_block_backward
    for elem in (L.ELEM_F32, L.ELEM_BF16):
        assert lib.gnx_block_backward_typed_workspace_bytes(None, C.byref(p), 1, elem) == 0
        assert _call(lib, None, p, elem, buf.ctypes.data, grads, ws) == L.ERR_INVALID_ARG
        assert b"NULL" in lib.gnx_last_error()
    assert lib.gnx_block_backward(None, C.byref(p), *([buf.ctypes.data] * 9), 1, *([buf.ctypes.data] * 3), C.byref(grads), ws.ctypes.data, ws.size,
                                  None) == L.ERR_INVALID_ARG
    assert np.all(buf == 0x7fc0) and np.all(gbuf == 7.0) and np.all(ws == 0x5A)


def test_no_silent_cpu_fallback_for_the_bf16_backward(lib):
    """Without a GPU the handle a well-formed typed call needs cannot be made (a HIP error, > 0), and the typed backward on what the
    constructor left fails without writing a byte on the host: there is no CPU path."""
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
    ins = np.ones(64, dtype=np.uint16)
    out = np.full(64, 0x7fc0, dtype=np.uint16)
    gbuf = np.full(256, 7.0, dtype=np.float32)
    ws = np.zeros(1 << 16, dtype=np.uint8)
    grads = L.BlockGrads(*[L.DenseGrad(gbuf.ctypes.data, gbuf.ctypes.data) for _ in range(3)])
    i, o = ins.ctypes.data, out.ctypes.data
    rc = lib.gnx_block_backward_typed(h, C.byref(p), L.ELEM_BF16, i, i, None, i, i, i, i, i, i, 1, o, o, None, C.byref(grads), ws.ctypes.data, ws.size, None)
    assert rc != 0
    assert lib.gnx_block_backward_typed_workspace_bytes(h, C.byref(p), 1, L.ELEM_BF16) == 0
    assert np.all(out == 0x7fc0) and np.all(ws == 0) and np.all(gbuf == 7.0) and np.all(ins == 1)


def test_gnblock_refuses_a_differentiable_bf16_call_unless_switched_on(monkeypatch):
    """bf16_backward off (the default): NotImplementedError that names the switch, before any library call"""
    import torch
    import graphnets_jl_amd as gn

    def no_lib():
        raise AssertionError("the library was called")

    monkeypatch.setattr(gn._lib, "load", no_lib)
    g = object.__new__(gn.GNGraphBatch)  # (no constructor: it would need the library)
    g._h, g.n_graphs, g.n_nodes, g.n_edges = None, 1, 3, 6
    ef = torch.zeros((10, 6, 1), dtype=torch.bfloat16)
    nf = torch.zeros((5, 3, 1), dtype=torch.bfloat16)
    for blk in (gn.GNBlock((10, 5, 0), (3, 4, 5), device="cpu"), gn.GNBlock((10, 5, 0), (3, 4, 5), device="cpu", bf16_backward=False)):
        assert blk.bf16_backward is False
        blk.edgefn.weight.requires_grad_(True)
        with pytest.raises(NotImplementedError, match="bf16_backward") as e:
            blk(gn.NT(g, ef, nf, None))
        assert "rounded to bfloat16" in str(e.value)
    # a feature that requires grad is refused the same way
    blk = gn.GNBlock((10, 5, 0), (3, 4, 5), device="cpu")
    with pytest.raises(NotImplementedError, match="bf16_backward"):
        blk(gn.NT(g, ef.clone().requires_grad_(True), nf, None))
    # the switch is a constructor argument and a plain attribute; switched on, the call goes on to the library
    assert gn.GNBlock((10, 5, 0), (3, 4, 5), device="cpu", bf16_backward=True).bf16_backward is True
    blk.bf16_backward = True
    blk.edgefn.weight.requires_grad_(True)
    with pytest.raises(AssertionError, match="the library was called"):
        blk(gn.NT(g, ef, nf, None))
    # Chain update functions on bf16 keep raising, switch or not
    blk.edgefn = gn.Chain(gn.Dense(20, 8, "relu", "cpu"), gn.Dense(8, 3, "identity", "cpu"))
    with pytest.raises(NotImplementedError, match="Chain"):
        blk(gn.NT(g, ef, nf, None))
