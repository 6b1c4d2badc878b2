"""CPU-side checks of the fused narrow backward at any narrow width set (gnx_block_backward_narrow): the four entries are declared, exported and
bound, the three backward entries with gnx_block_backward_fused_typed's parameter lists; a NULL handle, NULL params or an unknown element type
are refused before any GPU work without touching the caller's buffers; the kernel compiles at run time (hiprtc, no GPU) for width sets outside
the ahead-of-time list — two weight-gradient pairs per lane included — and is refused for the sets the eligibility rule excludes; it uses no
scratch memory and at most 64 KB of LDS at those sets; GNBlock carries the `narrow_backward` switch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_block_backward_narrow_applies", "gnx_block_backward_narrow_workspace_bytes", "gnx_block_backward_narrow", "gnx_jit_precompile_bw_edge")
AOT = ((10, 5, 0, 3), (3, 4, 5, 3), (0, 2, 0, 2), (2, 2, 2, 2), (4, 3, 2, 3))  # (de, dn, dg, oe)
RUN_TIME = ((3, 2, 4, 3), (2, 3, 1, 7), (6, 6, 3, 3), (20, 10, 4, 1), (1, 0, 0, 1), (0, 1, 0, 9), (0, 0, 1, 5))
REFUSED = ((10, 5, 3, 3), (23, 15, 10, 1))  # oe * Ke = 69; oe + Ke = 64: the kernel's LDS rows


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    return gn._lib.load()


def test_narrow_entries_declared_exported_and_bound(lib):
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
    assert S["gnx_block_backward_narrow"] == S["gnx_block_backward_fused_typed"]
    assert S["gnx_block_backward_narrow_workspace_bytes"] == S["gnx_block_backward_fused_typed_workspace_bytes"]
    assert S["gnx_block_backward_narrow_applies"] == S["gnx_block_backward_fused_typed_applies"]
    assert S["gnx_jit_precompile_bw_edge"] == (C.c_int32, [C.POINTER(gn._lib.BlockParams), C.c_int32, C.POINTER(C.c_size_t)])
    assert lib.gnx_version() == 130


def _setup(gn):
    L = gn._lib
    p = L.BlockParams(2, 3, 1, 7, 4, 5)
    w = np.zeros(128, dtype=np.float32)  # (never read: every call below fails before any GPU work)
    p.edgefn.weight = p.nodefn.weight = p.graphfn.weight = w.ctypes.data
    buf = np.full(64, 0x7fc0, dtype=np.uint16)
    gbuf = np.full(256, 7.0, dtype=np.float32)
    ws = np.full(1024, 0x5A, dtype=np.uint8)
    grads = L.BlockGrads(*[L.DenseGrad(gbuf.ctypes.data, gbuf.ctypes.data) for _ in range(3)])
    return p, w, buf, gbuf, ws, grads


def _call(lib, h, pp, elem, b, grads, ws):
    return lib.gnx_block_backward_narrow(h, pp, elem, *([b] * 9), 1, *([b] * 3), C.byref(grads), ws.ctypes.data, ws.size, None)


def test_null_handle_or_params_are_refused_before_gpu_work(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep, buf, gbuf, ws, grads = _setup(gn)
    fake = C.c_void_p(buf.ctypes.data)  # a non-NULL "handle" next to NULL params: refused before it is looked at
    for elem in (L.ELEM_F32, L.ELEM_BF16):
        for h, pp in ((None, C.byref(p)), (fake, None), (None, None)):
            assert lib.gnx_block_backward_narrow_applies(h, pp, 1, elem) == 0
            assert lib.gnx_block_backward_narrow_workspace_bytes(h, pp, 1, elem) == 0
            assert _call(lib, h, pp, elem, buf.ctypes.data, grads, ws) == L.ERR_INVALID_ARG
            assert b"NULL" in lib.gnx_last_error()
    assert np.all(buf == 0x7fc0) and np.all(gbuf == 7.0) and np.all(ws == 0x5A)


def test_bad_elem_is_refused_before_gpu_work(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep, buf, gbuf, ws, grads = _setup(gn)
    fake = C.c_void_p(buf.ctypes.data)  # a non-NULL "handle": an unknown elem must be refused before it is looked at
    n = C.c_size_t(12345)
    for elem in (-1, 0, 1, 2, 4, 6, 99):
        assert elem not in (L.ELEM_F32, L.ELEM_BF16)
        for h in (None, fake):
            assert lib.gnx_block_backward_narrow_applies(h, C.byref(p), 1, elem) == 0
            assert lib.gnx_block_backward_narrow_workspace_bytes(h, C.byref(p), 1, elem) == 0
            assert _call(lib, h, C.byref(p), elem, buf.ctypes.data, grads, ws) == L.ERR_INVALID_ARG
            assert b"elem" in lib.gnx_last_error()
        assert lib.gnx_jit_precompile_bw_edge(C.byref(p), elem, C.byref(n)) == L.ERR_INVALID_ARG and b"elem" in lib.gnx_last_error()
    assert lib.gnx_jit_precompile_bw_edge(None, L.ELEM_F32, C.byref(n)) == L.ERR_INVALID_ARG and b"NULL" in lib.gnx_last_error()
    assert n.value == 12345
    assert np.all(buf == 0x7fc0) and np.all(gbuf == 7.0) and np.all(ws == 0x5A)


def _stats(lib):
    s = (C.c_int64 * 4)()
    assert lib.gnx_jit_stats(s) == 0
    return list(s)


def test_the_kernel_compiles_at_run_time_for_eligible_width_sets_only(lib, monkeypatch):
    import graphnets_jl_amd as gn
    L = gn._lib
    monkeypatch.delenv("GNX_JIT_CACHE", raising=False)  # (the library reads it per request: every request below compiles)
    before = _stats(lib)
    sets = RUN_TIME + AOT
    for de, dn, dg, oe in sets:
        for elem in (L.ELEM_F32, L.ELEM_BF16):
            n = C.c_size_t(0)
            assert lib.gnx_jit_precompile_bw_edge(C.byref(L.BlockParams(de, dn, dg, oe, 4, 5)), elem, C.byref(n)) == 0, ((de, dn, dg, oe), lib.gnx_last_error())
            assert n.value > 0
    for de, dn, dg, oe in REFUSED:
        for elem in (L.ELEM_F32, L.ELEM_BF16):
            n = C.c_size_t(0)
            assert lib.gnx_jit_precompile_bw_edge(C.byref(L.BlockParams(de, dn, dg, oe, 4, 5)), elem, C.byref(n)) == L.ERR_DIMS, (de, dn, dg, oe)
            assert n.value == 0
    after = _stats(lib)
    assert after[0] == before[0] + 2 * len(sets) and after[2] == before[2] == 0, (before, after)
    assert lib.gnx_jit_precompile_bw_edge(C.byref(L.BlockParams(3, 2, 4, 3, 4, 5)), L.ELEM_F32, None) == 0  # (code_bytes is optional)


def test_no_scratch_and_the_lds_of_the_eligibility_rule():
    from tools.kernel_resources import HIPCC, eligible, resources, static_lds
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    sets = RUN_TIME + AOT
    assert all(eligible(*s) for s in sets) and not any(eligible(*s) for s in REFUSED)
    res = resources("bw_narrow", sets)
    assert set(res) == {str(s) for s in sets}, sorted(res)
    for s in sets:
        r = res[str(s)]
        assert set(r) == {"fp32", "bf16"}, (s, sorted(r))
        assert r["fp32"]["scratch"] == 0 and r["bf16"]["scratch"] == 0, (s, r)
        assert r["fp32"]["lds"] <= 64 * 1024, (s, r)
        assert r["bf16"]["lds"] == r["fp32"]["lds"], (s, r)  # (the LDS rows and accumulators stay fp32)
        assert r["fp32"]["lds"] <= static_lds(*s) + 1024, (s, r, static_lds(*s))  # what the rule counts (the compiler pads to its allocation unit)


def test_gnblock_has_the_switch():
    import graphnets_jl_amd as gn
    blk = gn.GNBlock((3, 2, 4), (3, 4, 5), device="cpu")
    assert blk.narrow_backward is False and blk.fused_backward is False and blk.bf16_backward is False
    blk.narrow_backward = True
    assert blk.narrow_backward is True and blk.fused_backward is False and blk.bf16_backward is False
    blk = gn.GNBlock((3, 2, 4), (3, 4, 5), device="cpu", narrow_backward=True)
    assert blk.narrow_backward is True and blk.fused_backward is False and blk.bf16_backward is False
    blk = gn.GNBlock((3, 2, 4), (3, 4, 5), device="cpu", narrow_backward=True, fused_backward=True, bf16_backward=True)
    assert blk.narrow_backward is True and blk.fused_backward is True and blk.bf16_backward is True
    assert gn.GNCore((10, 5, 3), device="cpu").block.narrow_backward is False  # (GNCore's inner block is not touched)
    assert "gnx_block_backward_narrow" in gn.GNBlock.__doc__
