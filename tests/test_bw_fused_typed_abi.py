"""CPU-side checks of the fused narrow backward on bfloat16 features (gnx_block_backward_fused_typed): the three entries are declared, exported
and bound with the typed pair's parameter lists, a NULL handle, NULL params or an unknown element type are refused before any GPU work without
touching the caller's buffers (the queries return 0), GNBlock carries both switches together, and the ten instantiations of the kernel compile
for gfx950 without scratch memory, the fp32 ones with the register counts they had (read from the compiler's resource remarks)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_block_backward_fused_typed_applies", "gnx_block_backward_fused_typed_workspace_bytes", "gnx_block_backward_fused_typed")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    return gn._lib.load()


def test_fused_typed_entries_declared_exported_and_bound(lib):
    import graphnets_jl_amd as gn
    with open(os.path.join(ROOT, "include", "gnx.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        m = re.search(r"GNX_API [\w\s\*]+?\b" + name + r"\(([^;]*?)\);", text, flags=re.S)
        assert m, f"{name} is not declared in include/gnx.h"
        assert hasattr(lib, name), f"{name} is not exported by libgnx.so"
        assert name in gn._lib.SIGNATURES
        assert m.group(1).count(",") + 1 == len(gn._lib.SIGNATURES[name][1]), name
    S = gn._lib.SIGNATURES
    assert S["gnx_block_backward_fused_typed"] == S["gnx_block_backward_typed"]  # gnx_block_backward_typed's parameter list
    assert S["gnx_block_backward_fused_typed_workspace_bytes"] == S["gnx_block_backward_typed_workspace_bytes"]
    assert S["gnx_block_backward_fused_typed_applies"] == (C.c_int32, S["gnx_block_backward_typed_workspace_bytes"][1])
    assert lib.gnx_version() == 130


def _setup(gn):
    L = gn._lib
    p = L.BlockParams(10, 5, 0, 3, 4, 5)
    w = np.zeros(64, dtype=np.float32)  # (never read: every call below fails before any GPU work)
    p.edgefn.weight = p.nodefn.weight = p.graphfn.weight = w.ctypes.data
    buf = np.full(64, 0x7fc0, dtype=np.uint16)
    gbuf = np.full(256, 7.0, dtype=np.float32)
    ws = np.full(1024, 0x5A, dtype=np.uint8)
    grads = L.BlockGrads(*[L.DenseGrad(gbuf.ctypes.data, gbuf.ctypes.data) for _ in range(3)])
    return p, w, buf, gbuf, ws, grads


def _call(lib, h, pp, elem, b, grads, ws):
    return lib.gnx_block_backward_fused_typed(h, pp, elem, *([b] * 9), 1, *([b] * 3), C.byref(grads), ws.ctypes.data, ws.size, None)


def test_null_handle_or_params_are_refused_before_gpu_work(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep, buf, gbuf, ws, grads = _setup(gn)
    fake = C.c_void_p(buf.ctypes.data)  # a non-NULL "handle" next to NULL params: refused before it is looked at
    for elem in (L.ELEM_F32, L.ELEM_BF16):
        for h, pp in ((None, C.byref(p)), (fake, None), (None, None)):
            assert lib.gnx_block_backward_fused_typed_applies(h, pp, 1, elem) == 0
            assert lib.gnx_block_backward_fused_typed_workspace_bytes(h, pp, 1, elem) == 0
            assert _call(lib, h, pp, elem, buf.ctypes.data, grads, ws) == L.ERR_INVALID_ARG
            assert b"NULL" in lib.gnx_last_error()
    assert np.all(buf == 0x7fc0) and np.all(gbuf == 7.0) and np.all(ws == 0x5A)


def test_bad_elem_is_refused_before_gpu_work(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep, buf, gbuf, ws, grads = _setup(gn)
    fake = C.c_void_p(buf.ctypes.data)  # a non-NULL "handle": an unknown elem must be refused before it is looked at
    for elem in (-1, 0, 1, 2, 4, 6, 99):
        assert elem not in (L.ELEM_F32, L.ELEM_BF16)
        for h in (None, fake):
            assert lib.gnx_block_backward_fused_typed_applies(h, C.byref(p), 1, elem) == 0
            assert lib.gnx_block_backward_fused_typed_workspace_bytes(h, C.byref(p), 1, elem) == 0
            assert _call(lib, h, C.byref(p), elem, buf.ctypes.data, grads, ws) == L.ERR_INVALID_ARG  # the typed call's status and message
            assert b"elem" in lib.gnx_last_error()
    assert np.all(buf == 0x7fc0) and np.all(gbuf == 7.0) and np.all(ws == 0x5A)


def test_gnblock_carries_both_switches():
    import graphnets_jl_amd as gn
    blk = gn.GNBlock((10, 5, 0), (3, 4, 5), device="cpu", bf16_backward=True, fused_backward=True)
    assert blk.bf16_backward is True and blk.fused_backward is True
    blk = gn.GNBlock((10, 5, 0), (3, 4, 5), device="cpu")
    assert blk.bf16_backward is False and blk.fused_backward is False
    blk.bf16_backward = blk.fused_backward = True
    assert blk.bf16_backward is True and blk.fused_backward is True
    assert "gnx_block_backward_fused_typed" in gn.GNBlock.__doc__


def test_ten_instantiations_without_scratch_and_the_fp32_registers_unchanged():
    """the compiler's resource remarks (as tools/time_bw_fused_bf16.py records them): k_bw_edge_wave keeps the VGPR counts it had before the body
    became a template over the element type, k_bw_edge_wave_bf16 exists for the same five width sets with the same LDS, nothing uses scratch"""
    from tools.time_bw_fused_bf16 import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    res = resources()
    vgpr = {"(10, 5, 0, 3)": 51, "(3, 4, 5, 3)": 50, "(4, 3, 2, 3)": 44, "(2, 2, 2, 2)": 38, "(0, 2, 0, 2)": 31}
    assert set(res) == set(vgpr), sorted(res)
    for dims, r in res.items():
        assert set(r) == {"fp32", "bf16"}, (dims, sorted(r))
        assert r["fp32"]["vgpr"] == vgpr[dims], (dims, r["fp32"])
        assert r["fp32"]["scratch"] == 0 and r["bf16"]["scratch"] == 0, (dims, r)
        assert r["bf16"]["lds"] == r["fp32"]["lds"], (dims, r)  # (the LDS rows and accumulators stay fp32)
