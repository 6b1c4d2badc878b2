"""CPU-side checks of gnx_chain_block_backward_wave_typed and its two queries: declared, exported and bound with
gnx_chain_block_backward_narrow_typed's parameter lists; the Julia shim names them; api._entry selects the call on bfloat16 features with
`wave_chain_backward` (which wins over `native_chain_backward` and `narrow_chain_backward`) and nothing changes without it; the refusals come in
the order of the other typed Chain pullbacks on a fake handle — bad elem, NULL handle, NULL params, a misaligned bf16 pointer — and write nothing."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_chain_narrow_abi import _fake_handle, _params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_chain_block_backward_wave_typed_applies", "gnx_chain_block_backward_wave_typed_workspace_bytes", "gnx_chain_block_backward_wave_typed")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    return gn._lib.load()


def test_entries_declared_exported_bound_and_named_by_the_shim(lib):
    import graphnets_jl_amd as gn
    S = gn._lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "gnx.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    with open(os.path.join(ROOT, "julia", "GraphNetsHIP.jl")) as f:
        shim = f.read()
    for name in NEW:
        m = re.search(r"GNX_API [\w\s\*]+?\b" + name + r"\(([^;]*?)\);", text, flags=re.S)
        assert m and hasattr(lib, name) and name in S, name
        assert m.group(1).count(",") + 1 == len(S[name][1]), name
        assert S[name] == S[name.replace("backward_wave_typed", "backward_narrow_typed")], name
        assert f"(:{name}, libgnx)" in shim, name
    assert lib.gnx_version() == 130


def test_entry_selects_the_call_on_bf16_with_the_wave_switch():
    import graphnets_jl_amd as gn
    F32, BF16 = gn._lib.ELEM_F32, gn._lib.ELEM_BF16
    base = {"bf16_chain", "bf16_backward"}
    for more in ((), ("native_chain_backward",), ("narrow_chain_backward",), ("native_chain_backward", "narrow_chain_backward")):
        e = gn.api._entry("chain", "backward", BF16, base | {"wave_chain_backward"} | set(more))
        assert e == gn.api._Entry(NEW[1], (BF16,), NEW[2], (BF16,), (), None), more
    assert gn.api._entry("chain", "backward", BF16, base | {"native_chain_backward"}).call == "gnx_chain_block_backward_narrow_typed"
    assert gn.api._entry("chain", "backward", BF16, base).call == "gnx_chain_block_backward_typed"
    assert gn.api._entry("chain", "backward", F32, base | {"wave_chain_backward"}).call == "gnx_chain_block_backward_wave"
    with pytest.raises(NotImplementedError, match="bf16_backward"):
        gn.api._entry("chain", "backward", BF16, {"bf16_chain", "wave_chain_backward"})
    assert "gnx_chain_block_backward_wave_typed" in gn.GNBlock.__doc__


def test_refusals_in_their_order_write_nothing(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep = _params(gn)  # in_dims (10, 5, 0): gf is nothing
    hbuf = _fake_handle()
    fake = C.c_void_p(hbuf.ctypes.data)
    buf = np.full(4096, 0x7fc0, dtype=np.uint16)
    gbuf = np.full(4096, 7.0, dtype=np.float32)
    ws = np.full(1024, 0x5A, dtype=np.uint8)
    b, g = buf.ctypes.data, gbuf.ctypes.data
    assert b % 4 == 0
    arrs = [(L.DenseGrad * 2)(*[L.DenseGrad(g, g) for _ in range(2)]) for _ in range(3)]
    grads = L.ChainBlockGrads(*[C.cast(a, C.POINTER(L.DenseGrad)) for a in arrs])

    def bwd(elem, ins=(b, b, None), ups=(b, b, b), douts=(b, b, None), h=fake, pp=C.byref(p), R=1):
        return lib.gnx_chain_block_backward_wave_typed(h, pp, elem, *ins, *ups, R, *douts, C.byref(grads), ws.ctypes.data, ws.size, None)

    for elem in (-1, 0, 2, 99):  # a bad elem: before anything else, a NULL handle, NULL params and a misaligned pointer included
        assert elem not in (L.ELEM_F32, L.ELEM_BF16)
        for kw in ({}, dict(h=None), dict(pp=None), dict(ins=(b + 2, b, None))):
            assert bwd(elem, **kw) == L.ERR_INVALID_ARG and b"elem" in lib.gnx_last_error(), (elem, kw)
        assert lib.gnx_chain_block_backward_wave_typed_applies(fake, C.byref(p), 1, elem) == 0
        assert lib.gnx_chain_block_backward_wave_typed_workspace_bytes(fake, C.byref(p), 1, elem) == 0
    for elem in (L.ELEM_F32, L.ELEM_BF16):  # a NULL handle or params: before the parameters and the alignment
        for kw in (dict(h=None), dict(pp=None), dict(h=None, ins=(b + 2, b, None), R=0)):
            assert bwd(elem, **kw) == L.ERR_INVALID_ARG and b"NULL handle or params" in lib.gnx_last_error(), (elem, kw)
        assert lib.gnx_chain_block_backward_wave_typed_applies(None, None, 1, elem) == 0
        assert lib.gnx_chain_block_backward_wave_typed_workspace_bytes(None, None, 1, elem) == 0
    # the parameters before the alignment
    assert bwd(L.ELEM_BF16, R=0, ins=(b + 2, b, None)) == L.ERR_INVALID_ARG and b"n_replicas" in lib.gnx_last_error()
    # a bf16 buffer that is 2-byte but not 4-byte aligned, each of the nine (gf and d_gf have no width here), before a NULL feature
    for k in range(2):
        ins = tuple(b + 2 if i == k else v for i, v in enumerate((b, b, None)))
        assert bwd(L.ELEM_BF16, ins=ins) == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error()
        assert bwd(L.ELEM_BF16, douts=ins) == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error()
    for k in range(3):
        assert bwd(L.ELEM_BF16, ups=tuple(b + 2 if i == k else b for i in range(3))) == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error()
    assert bwd(L.ELEM_BF16, ins=(None, b, None), ups=(b + 2, b, b)) == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error()
    assert bwd(L.ELEM_BF16, ins=(None, b, None)) == L.ERR_INVALID_ARG and b"input" in lib.gnx_last_error()
    assert np.all(buf == 0x7fc0) and np.all(gbuf == 7.0) and np.all(ws == 0x5A)
