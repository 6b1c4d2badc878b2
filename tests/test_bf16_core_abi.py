"""CPU-side checks of the bfloat16 GNCore forward (gnx_core_forward_typed): the two entries are declared, exported and bound; everything the
typed entry can refuse without a handle is refused before any GPU work; GNCore's dtype and mode checks run before any library call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_core_typed_workspace_bytes", "gnx_core_forward_typed")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    return gn._lib.load()


def test_typed_core_entries_declared_exported_and_bound(lib):
    import graphnets_jl_amd as gn
    with open(os.path.join(ROOT, "include", "gnx.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        m = re.search(r"GNX_API [\w\s\*]+?\b" + name + r"\(([^;]*?)\);", text, flags=re.S)
        assert m, f"{name} is not declared in include/gnx.h"
        assert hasattr(lib, name), f"{name} is not exported by libgnx.so"
        assert name in gn._lib.SIGNATURES
        assert m.group(1).count(",") + 1 == len(gn._lib.SIGNATURES[name][1]), name
    assert len(gn._lib.SIGNATURES["gnx_core_typed_workspace_bytes"][1]) == 5
    assert len(gn._lib.SIGNATURES["gnx_core_forward_typed"][1]) == len(gn._lib.SIGNATURES["gnx_core_forward"][1]) + 1 == 14
    assert lib.gnx_version() == 130


def _params(gn, dims=(10, 5, 3), out=None):
    L = gn._lib
    p = L.CoreParams()
    p.block = L.BlockParams(*dims, *(out or dims))
    w = np.zeros(1024, dtype=np.float32)  # (never read: every call below fails before any GPU work)
    p.block.edgefn.weight = p.block.nodefn.weight = p.block.graphfn.weight = w.ctypes.data
    for i in range(3):
        p.ln1[i].gamma = p.ln1[i].beta = p.ln2[i].gamma = p.ln2[i].beta = w.ctypes.data
        p.ff[i].fc1.weight = p.ff[i].fc2.weight = w.ctypes.data
    return p, w


def test_refusals_before_any_gpu_work(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep = _params(gn)
    buf = np.zeros(64, dtype=np.float32)
    ptr = buf.ctypes.data
    call = lambda elem, flags, bufs=(ptr,) * 6, q=p: lib.gnx_core_forward_typed(None, C.byref(q), elem, *bufs[:3], 1, *bufs[3:], ptr, 256, flags, None)
    # an unknown element type
    for elem in (7, -1, 0, 4, 6):
        assert lib.gnx_core_typed_workspace_bytes(None, C.byref(p), 1, elem, 0) == 0
        assert call(elem, 0) == L.ERR_INVALID_ARG and b"elem" in lib.gnx_last_error()
    # deferring the graph update is not a bf16 form
    assert lib.gnx_core_typed_workspace_bytes(None, C.byref(p), 1, L.ELEM_BF16, L.FLAG_DEFER_GRAPH_UPDATE) == 0
    assert call(L.ELEM_BF16, L.FLAG_DEFER_GRAPH_UPDATE) == L.ERR_INVALID_ARG and b"DEFER" in lib.gnx_last_error()
    # a bf16 buffer at an odd 2-byte address, input or output
    for i in range(6):
        bufs = [ptr] * 6
        bufs[i] = ptr + 2
        assert call(L.ELEM_BF16, 0, tuple(bufs)) == L.ERR_INVALID_ARG and b"4-byte aligned" in lib.gnx_last_error(), i
    # dims that the block does not map to themselves, and a zero width
    for dims, out in (((10, 5, 3), (10, 5, 4)), ((10, 5, 3), (3, 4, 5)), ((10, 0, 3), (10, 0, 3))):
        q, _k = _params(gn, dims, out)
        assert call(L.ELEM_BF16, 0, q=q) == L.ERR_DIMS, (dims, out)
    # a NULL handle is an argument error in both element types, as in gnx_core_forward; so are NULL params
    assert lib.gnx_core_typed_workspace_bytes(None, C.byref(p), 1, L.ELEM_BF16, 0) == 0
    for elem in (L.ELEM_F32, L.ELEM_BF16):
        assert call(elem, 0) == L.ERR_INVALID_ARG
        assert lib.gnx_core_forward_typed(None, None, elem, ptr, ptr, ptr, 1, ptr, ptr, ptr, ptr, 256, 0, None) == L.ERR_INVALID_ARG
    assert np.all(buf == 0)


def test_gncore_bf16_checks_run_before_any_library_call(monkeypatch):
    import torch
    import graphnets_jl_amd as gn

    def no_lib():
        raise AssertionError("the library was called")

    monkeypatch.setattr(gn._lib, "load", no_lib)
    bf = lambda *s: torch.zeros(s, dtype=torch.bfloat16)
    ef, nf, gf = bf(10, 6, 1), bf(5, 3, 1), bf(3, 1, 1)
    # the switch is off by default: a bf16 tensor is refused, and the message names the switch
    core = gn.GNCore((10, 5, 3), device="cpu")
    assert core.bf16 is False
    with pytest.raises(TypeError, match="bfloat16") as e:
        core(gn.NT(object(), ef, nf, gf))
    assert "bf16=True" in str(e.value)
    # on: mixed dtypes
    core = gn.GNCore((10, 5, 3), device="cpu", bf16=True)
    assert core.bf16 is True
    with pytest.raises(TypeError, match="bfloat16"):
        core(gn.NT(object(), ef, nf.float(), gf))
    with pytest.raises(TypeError, match="bfloat16"):
        core(gn.NT(object(), ef.double(), nf, gf))
    # on: a differentiable call
    core.block.edgefn.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="backward"):
        core(gn.NT(object(), ef, nf, gf))
    core.block.edgefn.weight.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="backward"):
        core(gn.NT(object(), ef.clone().requires_grad_(True), nf, gf))
    # on: Dropout forced active
    drop = gn.GNCore((10, 5, 3), dropout=0.25, device="cpu", bf16=True)
    gn.trainmode(drop)
    with pytest.raises(NotImplementedError, match="Dropout"):
        drop(gn.NT(object(), ef, nf, gf))
    # (each core of a list carries its own switch)
    cores = gn.GNCoreList([gn.GNCore((10, 5, 3), device="cpu", bf16=True), gn.GNCore((10, 5, 3), device="cpu")])
    assert [c.bf16 for c in cores.list] == [True, False]
