"""CPU-side checks of the typed Chain-block pair (gnx_chain_block_forward_typed / gnx_chain_block_backward_typed and their three queries):
declared, exported and bound with matching parameter counts; the queries return 0 on NULL, bad replica counts and an unknown element type; an
unknown element type, a `narrow` other than 0 / 1 and a bf16 buffer at +2 bytes are refused on a fake handle without touching the caller's
buffers; `_typed_applies` follows the narrow rule on the counts of a fake handle; GNBlock carries the `bf16_chain` switch, off by default, and
off still raises before any library call; the nine instantiations of k_chain_mlp_bf16 compile for gfx950 without scratch memory and the
committed record lists them."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests.test_chain_narrow_abi import _fake_handle, _params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_chain_block_forward_typed_applies", "gnx_chain_block_forward_typed_workspace_bytes", "gnx_chain_block_forward_typed",
       "gnx_chain_block_backward_typed_workspace_bytes", "gnx_chain_block_backward_typed")
QUERIES = NEW[:2] + NEW[3:4]
UNKNOWN_ELEMS = (-1, 0, 1, 2, 4, 6, 99)


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
    q = S["gnx_chain_block_workspace_bytes"][1] + [C.c_int32, C.c_int32]  # (h, p, n_replicas, elem, narrow)
    assert S["gnx_chain_block_forward_typed_applies"] == (C.c_int32, q)
    assert S["gnx_chain_block_forward_typed_workspace_bytes"] == (C.c_size_t, q) == S["gnx_chain_block_backward_typed_workspace_bytes"]
    res, args = S["gnx_chain_block_forward_typed"]
    plain = S["gnx_chain_block_forward"]  # its list with elem behind the params and narrow in front of the flags
    assert res == plain[0] and args[:2] == plain[1][:2] and args[2] == C.c_int32 and args[3:12] == plain[1][2:11] and args[12] == C.c_int32 and args[13:] == plain[1][11:]
    res, args = S["gnx_chain_block_backward_typed"]
    plain = S["gnx_chain_block_backward"]  # its list with elem behind the params and narrow in front of the stream
    assert res == plain[0] and args[:2] == plain[1][:2] and args[2] == C.c_int32 and args[3:-2] == plain[1][2:-1] and args[-2] == C.c_int32 and args[-1] == plain[1][-1]
    assert lib.gnx_version() == 130


def test_queries_return_zero_on_null_bad_replicas_and_an_unknown_elem(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep = _params(gn)
    hbuf = _fake_handle(G=3)
    fake = C.c_void_p(hbuf.ctypes.data)
    for name in QUERIES:
        q = getattr(lib, name)
        for elem in (L.ELEM_F32, L.ELEM_BF16):
            for narrow in (0, 1):
                for h, pp in ((None, C.byref(p)), (fake, None), (None, None)):
                    assert q(h, pp, 1, elem, narrow) == 0, name
                for R in (0, -1, -7, 2, 65536):  # R <= 0; R > 1 on a batch of three graphs; beyond the grid
                    assert q(fake, C.byref(p), R, elem, narrow) == 0, (name, R)
            for narrow in (-1, 2, 7):
                assert q(fake, C.byref(p), 1, elem, narrow) == 0, (name, narrow)
        for elem in UNKNOWN_ELEMS:  # on a fake handle: 0 before the handle is looked at
            assert elem not in (L.ELEM_F32, L.ELEM_BF16)
            for narrow in (0, 1):
                assert q(fake, C.byref(p), 1, elem, narrow) == 0, (name, elem)


def test_typed_applies_follows_the_narrow_rule(lib):
    """on the counts of a fake handle (no table is read): 1 exactly where narrow = 1, bf16, and every function with output and rows is in the mask"""
    import graphnets_jl_amd as gn
    L = gn._lib
    ap = lib.gnx_chain_block_forward_typed_applies
    hbuf = _fake_handle(G=3)
    fake = C.c_void_p(hbuf.ctypes.data)
    p, _keep = _params(gn)
    assert lib.gnx_chain_block_forward_narrow_applies(fake, C.byref(p), 1) == 7
    assert ap(fake, C.byref(p), 1, L.ELEM_BF16, 1) == 1
    assert ap(fake, C.byref(p), 1, L.ELEM_BF16, 0) == 0 and ap(fake, C.byref(p), 1, L.ELEM_F32, 1) == 0 and ap(fake, C.byref(p), 1, L.ELEM_F32, 0) == 0
    p33, _k = _params(gn, widths=((33, 3), (8, 4), (6, 5)))  # a mixed mask: staged
    assert lib.gnx_chain_block_forward_narrow_applies(fake, C.byref(p33), 1) == 6 and ap(fake, C.byref(p33), 1, L.ELEM_BF16, 1) == 0
    pn, _k = _params(gn, widths=((16, 3), (8, 4), ()))  # no graph output: the two functions that run are in the mask
    assert lib.gnx_chain_block_forward_narrow_applies(fake, C.byref(pn), 1) == 3 and ap(fake, C.byref(pn), 1, L.ELEM_BF16, 1) == 1
    hb = _fake_handle(G=3, N=4, E=0)  # a batch without edges: the edge function has no rows to run on
    no_edges = C.c_void_p(hb.ctypes.data)
    assert lib.gnx_chain_block_forward_narrow_applies(no_edges, C.byref(p), 1) == 6 and ap(no_edges, C.byref(p), 1, L.ELEM_BF16, 1) == 1
    assert ap(no_edges, C.byref(p33), 1, L.ELEM_BF16, 1) == 1  # (the 33-wide edge function does not run there)


def test_refusals_on_a_fake_handle_write_nothing(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep = _params(gn)  # in_dims (10, 5, 0): gf is nothing
    hbuf = _fake_handle()
    fake = C.c_void_p(hbuf.ctypes.data)
    buf = np.full(4096, 0x7fc0, dtype=np.uint16)
    gbuf = np.full(4096, 7.0, dtype=np.float32)
    ws = np.full(1024, 0x5A, dtype=np.uint8)
    b = buf.ctypes.data
    assert b % 4 == 0
    g = gbuf.ctypes.data
    arrs = [(L.DenseGrad * 2)(*[L.DenseGrad(g, g) for _ in range(2)]) for _ in range(3)]
    grads = L.ChainBlockGrads(*[C.cast(a, C.POINTER(L.DenseGrad)) for a in arrs])

    def fwd(elem, narrow, ins=(b, b, None), outs=(b, b, b), h=fake, pp=C.byref(p), wsn=ws.size):
        return lib.gnx_chain_block_forward_typed(h, pp, elem, *ins, 1, *outs, ws.ctypes.data, wsn, narrow, 0, None)

    def bwd(elem, narrow, ins=(b, b, None), ups=(b, b, b), douts=(b, b, None), h=fake, pp=C.byref(p)):
        return lib.gnx_chain_block_backward_typed(h, pp, elem, *ins, *ups, 1, *douts, C.byref(grads), ws.ctypes.data, ws.size, narrow, None)

    for elem in UNKNOWN_ELEMS:
        for narrow in (0, 1):
            assert fwd(elem, narrow) == L.ERR_INVALID_ARG and b"elem" in lib.gnx_last_error()
            assert bwd(elem, narrow) == L.ERR_INVALID_ARG and b"elem" in lib.gnx_last_error()
    for elem in (L.ELEM_F32, L.ELEM_BF16):
        for narrow in (-1, 2):
            assert fwd(elem, narrow) == L.ERR_INVALID_ARG and b"narrow" in lib.gnx_last_error()
            assert bwd(elem, narrow) == L.ERR_INVALID_ARG and b"narrow" in lib.gnx_last_error()
        for narrow in (0, 1):  # a NULL handle / NULL params: an argument error in both element types, as in the fp32 entries
            assert fwd(elem, narrow, h=None) == L.ERR_INVALID_ARG and fwd(elem, narrow, pp=None) == L.ERR_INVALID_ARG
            assert bwd(elem, narrow, h=None) == L.ERR_INVALID_ARG and bwd(elem, narrow, pp=None) == L.ERR_INVALID_ARG
    # a bf16 buffer that is 2-byte but not 4-byte aligned: every input, output, upstream gradient and input gradient in turn
    for narrow in (0, 1):
        for k in range(2):
            ins = tuple(b + 2 if i == k else v for i, v in enumerate((b, b, None)))
            assert fwd(L.ELEM_BF16, narrow, ins=ins) == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error()
            assert bwd(L.ELEM_BF16, narrow, ins=ins) == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error()
            douts = tuple(b + 2 if i == k else v for i, v in enumerate((b, b, None)))
            assert bwd(L.ELEM_BF16, narrow, douts=douts) == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error()
        for k in range(3):
            outs = tuple(b + 2 if i == k else b for i in range(3))
            assert fwd(L.ELEM_BF16, narrow, outs=outs) == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error()
            assert bwd(L.ELEM_BF16, narrow, ups=outs) == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error()
    # the native path's workspace refusal names the new query (all three functions fused: the fake handle is not read past its counts)
    # — the workspace holds the graph function's input rows and the fp32 rows of ef' and nf': 16 bytes are too few
    assert fwd(L.ELEM_BF16, 1, wsn=16) == L.ERR_WORKSPACE and b"gnx_chain_block_forward_typed_workspace_bytes()" in lib.gnx_last_error()
    assert np.all(buf == 0x7fc0) and np.all(gbuf == 7.0) and np.all(ws == 0x5A)


def test_gnblock_has_the_switch_and_off_still_raises(monkeypatch):
    import torch
    import graphnets_jl_amd as gn
    blk = gn.GNBlock((10, 5, 3), (3, 4, 5), device="cpu")
    assert blk.bf16_chain is False and blk.narrow_chain is False and blk.bf16_backward is False
    blk.bf16_chain = True
    assert blk.bf16_chain is True and blk.narrow_chain is False and blk.bf16_backward is False
    assert gn.GNBlock((10, 5, 3), (3, 4, 5), device="cpu", bf16_chain=True).bf16_chain is True
    assert "bf16_chain" in gn.GNBlock.__doc__ and "gnx_chain_block_forward_typed" in gn.GNBlock.__doc__ and "gnx_chain_block_backward_typed" in gn.GNBlock.__doc__

    def no_library():
        raise AssertionError("the refusal must come before any library call")

    monkeypatch.setattr(gn._lib, "load", no_library)
    x = gn.NT(object(), torch.zeros((10, 4, 1), dtype=torch.bfloat16), torch.zeros((5, 3, 1), dtype=torch.bfloat16), torch.zeros((3, 1, 1), dtype=torch.bfloat16))
    for kw in (dict(), dict(bf16_backward=True), dict(narrow_chain=True, narrow_chain_backward=True)):
        blk = gn.GNBlock((10, 5, 3), (3, 4, 5), device="cpu", **kw)
        blk.edgefn = gn.Chain(gn.Dense(23, 16, "relu", "cpu"), gn.Dense(16, 3, "identity", "cpu"))
        assert blk.bf16_chain is False
        with torch.no_grad(), pytest.raises(NotImplementedError, match="Chain") as e:
            blk(x)
        assert "bf16_chain" in str(e.value)
    # on, a differentiable call, bf16_backward off: refused in that switch's name, still before any library call
    blk = gn.GNBlock((10, 5, 3), (3, 4, 5), device="cpu", bf16_chain=True)
    blk.edgefn = gn.Chain(gn.Dense(23, 16, "relu", "cpu"), gn.Dense(16, 3, "identity", "cpu"))
    blk.edgefn.layers[0].weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="bf16_backward"):
        blk(x)
    # mixed bfloat16 / float32 features: TypeError, as everywhere
    xm = gn.NT(object(), torch.zeros((10, 4, 1), dtype=torch.bfloat16), torch.zeros((5, 3, 1), dtype=torch.float32), torch.zeros((3, 1, 1), dtype=torch.bfloat16))
    with torch.no_grad(), pytest.raises(TypeError, match="mix"):
        blk(xm)


def test_every_instantiation_compiles_without_scratch():
    from tools.kernel_resources import FAMILIES, HIPCC, resources
    LDS_BUDGET_BYTES, SRC, WMAX = (FAMILIES["chain_narrow_bf16"][k] for k in ("LDS_BUDGET_BYTES", "SRC", "WMAX"))
    with open(os.path.join(ROOT, "profiles", "chain_narrow_bf16_resources.json")) as f:
        rec = json.load(f)
    assert sorted(rec["srcs"]) == sorted(SRC) == ["edge", "node", "rows"] and rec["lds_budget_bytes"] == LDS_BUDGET_BYTES == 40960
    for s in SRC:
        assert sorted(int(k) for k in rec["srcs"][s]) == list(WMAX) == [8, 16, 32]
        assert all(v["scratch"] == 0 and v["lds_static"] == 0 for v in rec["srcs"][s].values()), rec["srcs"][s]
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    res = resources("chain_narrow_bf16")
    assert sum(len(res[s]) for s in SRC) == 9
    for s in SRC:
        assert sorted(res[s]) == list(WMAX), (s, sorted(res[s]))
        for w in WMAX:
            assert res[s][w]["scratch"] == 0 and res[s][w]["lds_static"] == 0, (s, w, res[s][w])
            assert sorted(res[s][w]) == sorted(rec["srcs"][s][str(w)]), (s, w)  # the committed record carries the same figures' keys
