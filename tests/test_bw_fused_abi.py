"""CPU-side checks of the fused narrow backward (gnx_block_backward_fused): the three entries are declared, exported and bound, a NULL handle
or NULL params are refused before any GPU work without touching the caller's buffers, GNBlock carries the `fused_backward` switch, and the five
instantiations of k_bw_edge_wave compile for gfx950 without scratch memory (read from the compiler's resource remarks)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_block_backward_fused_applies", "gnx_block_backward_fused_workspace_bytes", "gnx_block_backward_fused")
SETS = ((10, 5, 0, 3), (3, 4, 5, 3), (0, 2, 0, 2), (2, 2, 2, 2), (4, 3, 2, 3))  # (de, dn, dg, oe)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    return gn._lib.load()


def test_fused_entries_declared_exported_and_bound(lib):
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
    assert S["gnx_block_backward_fused"] == S["gnx_block_backward"]  # gnx_block_backward's parameter list, unchanged
    assert S["gnx_block_backward_fused_workspace_bytes"] == S["gnx_block_backward_workspace_bytes"]
    assert S["gnx_block_backward_fused_applies"] == (C.c_int32, S["gnx_block_backward_workspace_bytes"][1])
    assert lib.gnx_version() == 130


def test_null_handle_or_params_are_refused_before_gpu_work(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p = L.BlockParams(10, 5, 0, 3, 4, 5)
    w = np.zeros(64, dtype=np.float32)  # (never read: every call below fails before any GPU work)
    p.edgefn.weight = p.nodefn.weight = p.graphfn.weight = w.ctypes.data
    buf = np.full(64, 3.0, dtype=np.float32)
    gbuf = np.full(256, 7.0, dtype=np.float32)
    ws = np.full(1024, 0x5A, dtype=np.uint8)
    grads = L.BlockGrads(*[L.DenseGrad(gbuf.ctypes.data, gbuf.ctypes.data) for _ in range(3)])
    fake = C.c_void_p(buf.ctypes.data)  # a non-NULL "handle" next to NULL params: refused before it is looked at
    b = buf.ctypes.data
    for h, pp in ((None, C.byref(p)), (fake, None), (None, None)):
        assert lib.gnx_block_backward_fused_applies(h, pp, 1) == 0
        assert lib.gnx_block_backward_fused_workspace_bytes(h, pp, 1) == 0 == lib.gnx_block_backward_workspace_bytes(h, pp, 1)
        assert lib.gnx_block_backward_fused(h, pp, *([b] * 9), 1, *([b] * 3), C.byref(grads), ws.ctypes.data, ws.size, None) == L.ERR_INVALID_ARG
        assert b"NULL" in lib.gnx_last_error()
    assert np.all(buf == 3.0) and np.all(gbuf == 7.0) and np.all(ws == 0x5A)


def test_gnblock_has_the_switch():
    import graphnets_jl_amd as gn
    blk = gn.GNBlock((10, 5, 0), (3, 4, 5), device="cpu")
    assert blk.fused_backward is False and blk.bf16_backward is False
    blk.fused_backward = True
    assert blk.fused_backward is True
    assert gn.GNBlock((10, 5, 0), (3, 4, 5), device="cpu", fused_backward=True).fused_backward is True
    assert gn.GNCore((10, 5, 3), device="cpu").block.fused_backward is False  # (GNCore's inner block is not touched)


def test_the_five_instantiations_compile_without_scratch():
    from tools.kernel_resources import HIPCC, remarks
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    # {(de, dn, dg, oe): {sgpr, vgpr, scratch, lds, occupancy}} of the k_bw_edge_wave instantiations of gnx_backward_narrow.hip
    res = {}
    for name, r in remarks("gnx_backward_narrow.hip").items():
        m = re.match(r"_ZN3gnx14k_bw_edge_waveILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEEv", name)
        if m:
            res[tuple(int(v) for v in m.groups())] = dict(sgpr=r["sgpr"], vgpr=r["vgpr"], scratch=r["scratch"], lds=r["lds"], occupancy=r["waves_per_simd"])
    assert set(res) == set(SETS), sorted(res)
    for dims, r in res.items():
        assert r["scratch"] == 0, (dims, r)
        de, dn, dg, oe = dims
        ke = de + 2 * dn + dg
        assert oe * (ke + 1) <= 64  # one lane per (k, j) pair
        assert r["lds"] <= 4 * 4 * (64 * ((oe + ke) | 1) + 64) + 1024, (dims, r)  # four wave slices of 64 rows, four accumulator rows
