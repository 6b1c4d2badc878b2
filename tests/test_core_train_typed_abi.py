"""CPU-side checks of the typed training-mode pair of a GNCore (gnx_core_forward_train_typed / gnx_core_backward_train_typed and their three
queries): declared, exported and bound with matching parameter counts; an unknown element type, a Dropout probability outside [0, 1], a
`narrow` other than 0 / 1, a misaligned bf16 buffer and GNX_FLAG_DEFER_GRAPH_UPDATE with an active Dropout are refused on a fake handle
without touching the caller's buffers; every query returns 0 on NULL; GNCore carries the `typed_dropout` switch, off by default, and off
still raises; every instantiation of k_core_post_train compiles for gfx950 without scratch memory."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests.test_core_bw_narrow_abi import _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_core_train_fused_applies", "gnx_core_train_typed_workspace_bytes", "gnx_core_forward_train_typed",
       "gnx_core_backward_train_typed_workspace_bytes", "gnx_core_backward_train_typed")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    return gn._lib.load()


def test_entries_declared_exported_and_bound(lib):
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
    drop = C.POINTER(gn._lib.Dropout)
    res, args = S["gnx_core_forward_train_typed"]
    typed = S["gnx_core_forward_typed"]  # the typed forward's list with the Dropout behind elem
    assert res == typed[0] and args[:3] == typed[1][:3] and args[3] == drop and args[4:] == typed[1][3:]
    res, args = S["gnx_core_backward_train_typed"]
    typed = S["gnx_core_backward_typed"]  # the typed backward's list with (dropout, narrow) behind elem
    assert res == typed[0] and args[:3] == typed[1][:3] and args[3] == drop and args[4] == C.c_int32 and args[5:] == typed[1][3:]
    assert S["gnx_core_train_typed_workspace_bytes"] == S["gnx_core_typed_workspace_bytes"]
    assert S["gnx_core_train_fused_applies"] == S["gnx_core_backward_narrow_applies"]
    assert S["gnx_core_backward_train_typed_workspace_bytes"][1] == S["gnx_core_backward_typed_workspace_bytes"][1] + [C.c_int32]
    assert lib.gnx_version() == 130


def _fwd(lib, h, pp, elem, drop, b, ws, flags=0, out=None):
    o = b if out is None else out
    return lib.gnx_core_forward_train_typed(h, pp, elem, drop, b, b, b, 1, o, o, o, ws.ctypes.data, ws.size, flags, None)


def _bwd(lib, h, pp, elem, drop, narrow, b, grads, ws):
    return lib.gnx_core_backward_train_typed(h, pp, elem, drop, narrow, *([b] * 6), 1, *([b] * 3), C.byref(grads), ws.ctypes.data, ws.size, None)


def test_every_query_returns_zero_on_null(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep, buf, _gbuf, _ws, _grads = _setup(gn)
    fake = C.c_void_p(buf.ctypes.data)
    for elem in (L.ELEM_F32, L.ELEM_BF16):
        for h, pp in ((None, C.byref(p)), (fake, None), (None, None)):
            assert lib.gnx_core_train_fused_applies(h, pp, 1, elem) == 0
            assert lib.gnx_core_train_typed_workspace_bytes(h, pp, 1, elem, 0) == 0
            for narrow in (0, 1):
                assert lib.gnx_core_backward_train_typed_workspace_bytes(h, pp, 1, elem, narrow) == 0
    for elem in (-1, 0, 1, 2, 4, 6, 99):  # an unknown element type, on a fake handle: 0 before the handle is looked at
        assert elem not in (L.ELEM_F32, L.ELEM_BF16)
        assert lib.gnx_core_train_fused_applies(fake, C.byref(p), 1, elem) == 0
        assert lib.gnx_core_train_typed_workspace_bytes(fake, C.byref(p), 1, elem, 0) == 0
        assert lib.gnx_core_backward_train_typed_workspace_bytes(fake, C.byref(p), 1, elem, 0) == 0
    for narrow in (-1, 2, 7):
        assert lib.gnx_core_backward_train_typed_workspace_bytes(fake, C.byref(p), 1, L.ELEM_F32, narrow) == 0


def test_refusals_on_a_fake_handle_write_nothing(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep, buf, gbuf, ws, grads = _setup(gn)
    fake = C.c_void_p(buf.ctypes.data)  # a non-NULL "handle": every call below is refused before it is looked at
    b = buf.ctypes.data
    live = L.Dropout(0.3, 0, 7)
    for elem in (-1, 0, 1, 2, 4, 6, 99):
        assert _fwd(lib, fake, C.byref(p), elem, C.byref(live), b, ws) == L.ERR_INVALID_ARG and b"elem" in lib.gnx_last_error()
        assert _fwd(lib, fake, C.byref(p), elem, None, b, ws) == L.ERR_INVALID_ARG and b"elem" in lib.gnx_last_error()
        assert _bwd(lib, fake, C.byref(p), elem, C.byref(live), 0, b, grads, ws) == L.ERR_INVALID_ARG and b"elem" in lib.gnx_last_error()
    for prob in (-0.25, 1.5, float("nan"), float("inf")):
        for elem in (L.ELEM_F32, L.ELEM_BF16):
            drop = L.Dropout(prob, 0, 7)
            assert _fwd(lib, fake, C.byref(p), elem, C.byref(drop), b, ws) == L.ERR_INVALID_ARG and b"Dropout" in lib.gnx_last_error()
            for narrow in (0, 1):
                assert _bwd(lib, fake, C.byref(p), elem, C.byref(drop), narrow, b, grads, ws) == L.ERR_INVALID_ARG and b"Dropout" in lib.gnx_last_error()
    for elem in (L.ELEM_F32, L.ELEM_BF16):
        for drop in (None, C.byref(live)):
            assert _bwd(lib, fake, C.byref(p), elem, drop, 2, b, grads, ws) == L.ERR_INVALID_ARG and b"narrow" in lib.gnx_last_error()
            assert _bwd(lib, fake, C.byref(p), elem, drop, -1, b, grads, ws) == L.ERR_INVALID_ARG and b"narrow" in lib.gnx_last_error()
    # a bf16 buffer that is 2-byte but not 4-byte aligned, as an input and as an output
    assert b % 4 == 0
    assert _fwd(lib, fake, C.byref(p), L.ELEM_BF16, C.byref(live), b + 2, ws, out=b) == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error()
    assert _fwd(lib, fake, C.byref(p), L.ELEM_BF16, C.byref(live), b, ws, out=b + 2) == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error()
    # GNX_FLAG_DEFER_GRAPH_UPDATE with an active Dropout, either element type; its query returns 0
    for elem in (L.ELEM_F32, L.ELEM_BF16):
        assert _fwd(lib, fake, C.byref(p), elem, C.byref(live), b, ws, flags=L.FLAG_DEFER_GRAPH_UPDATE) == L.ERR_INVALID_ARG
        assert b"DEFER" in lib.gnx_last_error()
        assert lib.gnx_core_train_typed_workspace_bytes(fake, C.byref(p), 1, elem, L.FLAG_DEFER_GRAPH_UPDATE) == 0
    # dims the block does not map to themselves: GNX_ERR_DIMS, still before the handle
    p.block.oe = 7
    assert _fwd(lib, fake, C.byref(p), L.ELEM_BF16, C.byref(live), b, ws) == L.ERR_DIMS
    assert np.all(buf == 0x7fc0) and np.all(gbuf == 7.0) and np.all(ws == 0x5A)


def test_gncore_has_the_switch_and_off_still_raises():
    import torch
    import graphnets_jl_amd as gn
    core = gn.GNCore((10, 5, 3), device="cpu")
    assert core.typed_dropout is False and core.bf16 is False and core.bf16_backward is False and core.narrow_backward is False
    core.typed_dropout = True
    assert core.typed_dropout is True and core.bf16 is False and core.narrow_backward is False
    core = gn.GNCore((10, 5, 3), dropout=0.25, device="cpu", typed_dropout=True, bf16=True, bf16_backward=True, narrow_backward=True)
    assert core.typed_dropout is True and core.bf16 is True and core.bf16_backward is True and core.narrow_backward is True
    assert "gnx_core_forward_train_typed" in gn.GNCore.__doc__ and "gnx_core_backward_train_typed" in gn.GNCore.__doc__
    # off (the default): the three refusals of a bfloat16 call, before any library call
    x = gn.NT(object(), torch.zeros((10, 4, 1), dtype=torch.bfloat16), torch.zeros((5, 3, 1), dtype=torch.bfloat16), torch.zeros((3, 1, 1), dtype=torch.bfloat16))
    core = gn.GNCore((10, 5, 3), dropout=0.25, device="cpu", bf16=True)
    assert core.typed_dropout is False
    for q in core.parameters():
        q.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="bf16_backward"):  # a gradient call without bf16_backward
        core(x)
    core.bf16_backward = True
    with pytest.raises(NotImplementedError, match="Dropout"):  # p > 0 inside a gradient call
        core(x)
    gn.trainmode(core)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="Dropout"):  # forced by trainmode
        core(x)


def test_every_instantiation_compiles_without_scratch():
    from tools.kernel_resources import FAMILIES, HIPCC, resources
    ELEMS, WIDTHS = (FAMILIES["core_train_narrow"][k] for k in ("ELEMS", "WIDTHS"))
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    res = resources("core_train_narrow")
    assert sorted(res) == sorted(ELEMS) == ["bf16", "f32"]
    for e in ELEMS:
        assert sorted(res[e]) == list(WIDTHS) == list(range(1, 17)), (e, sorted(res[e]))
        for d in WIDTHS:
            assert res[e][d]["scratch"] == 0, (e, d, res[e][d])
            assert res[e][d]["lds"] <= 64 * 1024, (e, d, res[e][d])
    with open(os.path.join(ROOT, "profiles", "core_train_narrow_resources.json")) as f:
        rec = json.load(f)
    for e in ELEMS:
        assert sorted(int(k) for k in rec["elems"][e]) == list(WIDTHS) and all(v["scratch"] == 0 for v in rec["elems"][e].values())
