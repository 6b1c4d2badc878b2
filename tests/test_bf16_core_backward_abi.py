"""CPU-side checks of the bfloat16 GNCore backward (gnx_core_backward_typed): the two entries are declared, exported and bound; everything the
typed entry can refuse without a handle is refused before any GPU work and leaves the caller's buffers alone; GNCore's dtype, switch and mode
checks run before any library call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_core_backward_typed_workspace_bytes", "gnx_core_backward_typed")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    return gn._lib.load()


def test_typed_core_backward_entries_declared_exported_and_bound(lib):
    import graphnets_jl_amd as gn
    with open(os.path.join(ROOT, "include", "gnx.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        m = re.search(r"GNX_API [\w\s\*]+?\b" + name + r"\(([^;]*?)\);", text, flags=re.S)
        assert m, f"{name} is not declared in include/gnx.h"
        assert hasattr(lib, name), f"{name} is not exported by libgnx.so"
        assert name in gn._lib.SIGNATURES
        assert m.group(1).count(",") + 1 == len(gn._lib.SIGNATURES[name][1]), name
    assert len(gn._lib.SIGNATURES["gnx_core_backward_typed_workspace_bytes"][1]) == 4
    assert len(gn._lib.SIGNATURES["gnx_core_backward_typed"][1]) == len(gn._lib.SIGNATURES["gnx_core_backward"][1]) + 1 == 17
    assert lib.gnx_version() == 130


def _params(gn, dims=(10, 5, 3)):
    L = gn._lib
    p = L.CoreParams()
    p.block = L.BlockParams(*dims, *dims)
    w = np.zeros(1024, dtype=np.float32)  # (never read: every call below fails before any GPU work)
    p.block.edgefn.weight = p.block.nodefn.weight = p.block.graphfn.weight = w.ctypes.data
    for i in range(3):
        p.ln1[i].gamma = p.ln1[i].beta = p.ln2[i].gamma = p.ln2[i].beta = w.ctypes.data
        p.ff[i].fc1.weight = p.ff[i].fc2.weight = w.ctypes.data
    return p, w


def test_refusals_on_a_null_handle_leave_host_buffers_untouched(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep = _params(gn)
    ins = np.full(64, 1.5, dtype=np.float32)        # the six inputs
    outs = np.full(64, 2.5, dtype=np.float32)       # d_ef / d_nf / d_gf, every parameter gradient and the workspace
    pi, po = ins.ctypes.data, outs.ctypes.data
    gr = L.CoreGrads()
    gr.block.edgefn.weight = gr.ln1[0].gamma = gr.ff[2].fc2.bias = po
    call = lambda elem, six=(pi,) * 6, d=(po,) * 3: lib.gnx_core_backward_typed(None, C.byref(p), elem, *six, 1, *d, C.byref(gr), po, 256, None)
    # an unknown element type: refused by name, and the query gives no size for it
    for elem in (7, -1, 0, 4, 6):
        assert lib.gnx_core_backward_typed_workspace_bytes(None, C.byref(p), 1, elem) == 0
        assert call(elem) == L.ERR_INVALID_ARG and b"elem" in lib.gnx_last_error()
    # a bf16 buffer at an odd 2-byte address, any of the nine
    for i in range(9):
        bufs = [pi] * 6 + [po] * 3
        bufs[i] += 2
        assert call(L.ELEM_BF16, tuple(bufs[:6]), tuple(bufs[6:])) == L.ERR_INVALID_ARG, i
    # a NULL handle or NULL params is an argument error in both element types, as in gnx_core_backward; the query returns 0
    for elem in (L.ELEM_F32, L.ELEM_BF16):
        assert lib.gnx_core_backward_typed_workspace_bytes(None, C.byref(p), 1, elem) == 0
        assert call(elem) == L.ERR_INVALID_ARG
        assert lib.gnx_core_backward_typed(None, None, elem, pi, pi, pi, pi, pi, pi, 1, po, po, po, None, po, 256, None) == L.ERR_INVALID_ARG
    assert np.all(ins == 1.5) and np.all(outs == 2.5)


def test_gncore_bf16_backward_checks_run_before_any_library_call(monkeypatch):
    import torch
    import graphnets_jl_amd as gn

    def no_lib():
        raise AssertionError("the library was called")

    monkeypatch.setattr(gn._lib, "load", no_lib)
    bf = lambda *s: torch.zeros(s, dtype=torch.bfloat16)
    ef, nf, gf = bf(10, 6, 1), bf(5, 3, 1), bf(3, 1, 1)
    # the switch is off by default and is a plain attribute: a differentiable call is refused, and the message names the switch
    core = gn.GNCore((10, 5, 3), device="cpu", bf16=True)
    assert core.bf16_backward is False
    core.block.edgefn.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="backward") as e:
        core(gn.NT(object(), ef, nf, gf))
    assert "bf16_backward" in str(e.value)
    core.block.edgefn.weight.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="bf16_backward"):
        core(gn.NT(object(), ef.clone().requires_grad_(True), nf, gf))
    # on: mixed dtypes are still a TypeError, differentiable or not
    core = gn.GNCore((10, 5, 3), device="cpu", bf16=True, bf16_backward=True)
    assert core.bf16 is True and core.bf16_backward is True
    core.ffwd.eff[0].weight.requires_grad_(True)
    with pytest.raises(TypeError, match="bfloat16"):
        core(gn.NT(object(), ef, nf.float(), gf))
    with pytest.raises(TypeError, match="bfloat16"):
        core(gn.NT(object(), ef.double(), nf, gf))
    # bf16_backward without bf16 changes nothing: a bf16 tensor is refused as before
    plain = gn.GNCore((10, 5, 3), device="cpu", bf16_backward=True)
    with pytest.raises(TypeError, match="bfloat16"):
        plain(gn.NT(object(), ef, nf, gf))
    # on, with Dropout: p > 0 inside a gradient call (Flux's automatic mode), and forced by trainmode outside one
    drop = gn.GNCore((10, 5, 3), dropout=0.25, device="cpu", bf16=True, bf16_backward=True)
    with pytest.raises(NotImplementedError, match="Dropout"):
        drop(gn.NT(object(), ef.clone().requires_grad_(True), nf, gf))
    drop.gn1.edgeln.gamma.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="Dropout"):
        drop(gn.NT(object(), ef, nf, gf))
    drop.gn1.edgeln.gamma.requires_grad_(False)
    gn.trainmode(drop)
    with pytest.raises(NotImplementedError, match="Dropout"):
        drop(gn.NT(object(), ef, nf, gf))
    # (each core of a list carries its own switches)
    cores = gn.GNCoreList([gn.GNCore((10, 5, 3), device="cpu", bf16=True, bf16_backward=True), gn.GNCore((10, 5, 3), device="cpu", bf16=True)])
    assert [c.bf16_backward for c in cores.list] == [True, False]
