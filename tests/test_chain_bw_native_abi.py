"""CPU-side checks of the native bf16 Chain pullback's entries (gnx_chain_block_backward_narrow_typed and its two queries): declared, exported and
bound with gnx_chain_block_backward_typed's parameter list without `narrow`; the queries return 0 on NULL, on bad replicas and on an unknown
elem; `_applies` follows the native rule on the counts of a fake handle; the call's refusals come in the typed entry's order and write nothing,
the workspace refusal in the new query's name; GNBlock carries the `native_chain_backward` switch, off by default and described; the nine
instantiations of k_chain_mlp_bw_bf16 compile for gfx950 without scratch memory and the committed record lists them."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests.test_chain_narrow_abi import _fake_handle, _params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_chain_block_backward_narrow_typed_applies", "gnx_chain_block_backward_narrow_typed_workspace_bytes", "gnx_chain_block_backward_narrow_typed")
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
    q = S["gnx_chain_block_backward_workspace_bytes"][1] + [C.c_int32]  # (h, p, n_replicas, elem)
    assert len(q) == 4
    assert S["gnx_chain_block_backward_narrow_typed_applies"] == (C.c_int32, q)
    assert S["gnx_chain_block_backward_narrow_typed_workspace_bytes"] == (C.c_size_t, q)
    res, args = S["gnx_chain_block_backward_narrow_typed"]
    typed = S["gnx_chain_block_backward_typed"]  # its list without `narrow`, which stands in front of the stream
    assert res == typed[0] and args == typed[1][:-2] + typed[1][-1:] and len(args) == 17
    assert lib.gnx_version() == 130


def test_queries_return_zero_on_null_bad_replicas_and_an_unknown_elem(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep = _params(gn)
    hbuf = _fake_handle(G=3)
    fake = C.c_void_p(hbuf.ctypes.data)
    for name in NEW[:2]:
        q = getattr(lib, name)
        for elem in (L.ELEM_F32, L.ELEM_BF16):
            for h, pp in ((None, C.byref(p)), (fake, None), (None, None)):
                assert q(h, pp, 1, elem) == 0, name
            for R in (0, -1, -7, 2, 65536):  # R <= 0; R > 1 on a batch of three graphs; beyond the grid
                assert q(fake, C.byref(p), R, elem) == 0, (name, R)
        for elem in UNKNOWN_ELEMS:  # on a fake handle: 0 before the handle is looked at
            assert elem not in (L.ELEM_F32, L.ELEM_BF16)
            assert q(fake, C.byref(p), 1, elem) == 0, (name, elem)


def test_applies_follows_the_native_rule(lib):
    """on the counts of a fake handle (no table is read): 1 exactly where the features are bf16, the edge function has an output and edges, and
    every function with an output and rows is in gnx_chain_block_backward_narrow_applies' mask"""
    import graphnets_jl_amd as gn
    L = gn._lib
    ap, mask = lib.gnx_chain_block_backward_narrow_typed_applies, lib.gnx_chain_block_backward_narrow_applies
    hbuf = _fake_handle(G=3)
    fake = C.c_void_p(hbuf.ctypes.data)
    hb = _fake_handle(G=3, N=4, E=0)
    no_edges = C.c_void_p(hb.ctypes.data)
    p, _keep = _params(gn)
    assert mask(fake, C.byref(p), 1) == 7 and ap(fake, C.byref(p), 1, L.ELEM_BF16) == 1 and ap(fake, C.byref(p), 1, L.ELEM_F32) == 0
    assert mask(no_edges, C.byref(p), 1) == 6 and ap(no_edges, C.byref(p), 1, L.ELEM_BF16) == 0  # no edges: no edge level to pull back through
    p33, _k = _params(gn, widths=((33, 3), (8, 4), (6, 5)))  # mixed masks stay staged
    assert mask(fake, C.byref(p33), 1) == 6 and ap(fake, C.byref(p33), 1, L.ELEM_BF16) == 0
    pg, _k = _params(gn, widths=((16, 3), (8, 4), (33, 5)))
    assert mask(fake, C.byref(pg), 1) == 3 and ap(fake, C.byref(pg), 1, L.ELEM_BF16) == 0
    # the pullback's LDS rule, not the forward's: [32,32,32,3] behind a 32-wide input is fused by the forward and cut here (tests/test_chain_bw_narrow_abi.py)
    pl, _k = _params(gn, in_dims=(32, 0, 0), widths=((32, 32, 32, 3), (8, 4), (6, 5)))
    assert lib.gnx_chain_block_forward_narrow_applies(fake, C.byref(pl), 1) == 7 and mask(fake, C.byref(pl), 1) == 6 and ap(fake, C.byref(pl), 1, L.ELEM_BF16) == 0
    pn, _k = _params(gn, widths=((16, 3), (8, 4), ()))  # no graph output: the two functions that run are in the mask
    assert mask(fake, C.byref(pn), 1) == 3 and ap(fake, C.byref(pn), 1, L.ELEM_BF16) == 1
    pz, _k = _params(gn, widths=((), (8, 4), (6, 5)))  # an edge function without output: the call refuses it
    assert ap(fake, C.byref(pz), 1, L.ELEM_BF16) == 0


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

    def bwd(elem, ins=(b, b, None), ups=(b, b, b), douts=(b, b, None), h=fake, pp=C.byref(p), R=1, wsp=ws.ctypes.data, wsn=ws.size):
        return lib.gnx_chain_block_backward_narrow_typed(h, pp, elem, *ins, *ups, R, *douts, C.byref(grads), wsp, wsn, None)

    for elem in UNKNOWN_ELEMS:  # before anything else, a NULL handle included
        assert bwd(elem) == L.ERR_INVALID_ARG and b"elem" in lib.gnx_last_error()
        assert bwd(elem, h=None) == L.ERR_INVALID_ARG and b"elem" in lib.gnx_last_error()
    for elem in (L.ELEM_F32, L.ELEM_BF16):
        assert bwd(elem, h=None) == L.ERR_INVALID_ARG and bwd(elem, pp=None) == L.ERR_INVALID_ARG
    # bad replicas: the typed entry's codes (fp32: gnx_chain_block_backward's one code for every refused parameter set)
    assert bwd(L.ELEM_BF16, R=0) == L.ERR_INVALID_ARG and b"n_replicas" in lib.gnx_last_error()
    assert bwd(L.ELEM_F32, R=0) == L.ERR_DIMS and b"n_replicas" in lib.gnx_last_error()
    # a bf16 buffer that is 2-byte but not 4-byte aligned: every input, upstream gradient and input gradient in turn
    for k in range(2):
        ins = tuple(b + 2 if i == k else v for i, v in enumerate((b, b, None)))
        assert bwd(L.ELEM_BF16, ins=ins) == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error()
        douts = tuple(b + 2 if i == k else v for i, v in enumerate((b, b, None)))
        assert bwd(L.ELEM_BF16, douts=douts) == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error()
    for k in range(3):
        ups = tuple(b + 2 if i == k else b for i in range(3))
        assert bwd(L.ELEM_BF16, ups=ups) == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error()
    assert bwd(L.ELEM_BF16, ins=(None, b, None)) == L.ERR_INVALID_ARG and b"input" in lib.gnx_last_error()
    pz, _k = _params(gn, widths=((), (8, 4), (6, 5)))
    assert bwd(L.ELEM_F32, pp=C.byref(pz)) == L.ERR_DIMS and b"edge function without output" in lib.gnx_last_error()
    # (a staged bf16 call asks for its workspace first, as the typed entry does)
    typed = lib.gnx_chain_block_backward_typed(fake, C.byref(pz), L.ELEM_BF16, b, b, None, b, b, b, 1, b, b, None, C.byref(grads), ws.ctypes.data, ws.size, 1, None)
    assert bwd(L.ELEM_BF16, pp=C.byref(pz)) == typed == L.ERR_WORKSPACE
    # the workspace refusals: a bf16 call in the new query's name — on the native path (all three functions fused: the fake handle is not read past
    # its counts) and on the staged one (a mixed mask) — an fp32 call in gnx_chain_block_backward_narrow's, the entry it is
    assert lib.gnx_chain_block_backward_narrow_typed_applies(fake, C.byref(p), 1, L.ELEM_BF16) == 1
    p33, _k = _params(gn, widths=((16, 3), (8, 4), (33, 5)))
    assert lib.gnx_chain_block_backward_narrow_typed_applies(fake, C.byref(p33), 1, L.ELEM_BF16) == 0
    for wsp, wsn in ((ws.ctypes.data, 16), (None, 1 << 20)):
        for pp in (p, p33):
            assert bwd(L.ELEM_BF16, pp=C.byref(pp), wsp=wsp, wsn=wsn) == L.ERR_WORKSPACE
            assert b"gnx_chain_block_backward_narrow_typed_workspace_bytes()" in lib.gnx_last_error()
        assert bwd(L.ELEM_F32, wsp=wsp, wsn=wsn) == L.ERR_WORKSPACE and b"gnx_chain_block_backward_narrow_workspace_bytes()" in lib.gnx_last_error()
    assert np.all(buf == 0x7fc0) and np.all(gbuf == 7.0) and np.all(ws == 0x5A)


def test_gnblock_has_the_switch_off_by_default():
    import graphnets_jl_amd as gn
    blk = gn.GNBlock((10, 5, 3), (3, 4, 5), device="cpu")
    assert blk.native_chain_backward is False
    blk.native_chain_backward = True
    assert blk.native_chain_backward is True and blk.narrow_chain_backward is False and blk.bf16_chain is False and blk.bf16_backward is False
    assert gn.GNBlock((10, 5, 3), (3, 4, 5), device="cpu", native_chain_backward=True).native_chain_backward is True
    doc = gn.GNBlock.__doc__
    assert "native_chain_backward" in doc and "gnx_chain_block_backward_narrow_typed" in doc


def test_every_instantiation_compiles_without_scratch():
    from tools.kernel_resources import FAMILIES, HIPCC, resources
    LDS_BUDGET_BYTES, SRC, WMAX = (FAMILIES["chain_bw_narrow_bf16"][k] for k in ("LDS_BUDGET_BYTES", "SRC", "WMAX"))
    with open(os.path.join(ROOT, "profiles", "chain_bw_narrow_bf16_resources.json")) as f:
        rec = json.load(f)
    assert sorted(rec["srcs"]) == sorted(SRC) == ["edge", "node", "rows"] and rec["lds_budget_bytes"] == LDS_BUDGET_BYTES == 65536
    for s in SRC:
        assert sorted(int(k) for k in rec["srcs"][s]) == list(WMAX) == [8, 16, 32]
        assert all(v["scratch"] == 0 and v["lds_static"] == 0 for v in rec["srcs"][s].values()), rec["srcs"][s]
    # an instantiation beyond 256 VGPRs would lose the fp32 kernel's second wave per SIMD: the record has to say so
    lost = [f"{s}/{w}" for s in SRC for w, v in rec["srcs"][s].items() if v["vgpr"] > 256]
    assert all(n in rec["instantiations_with_fewer_waves_per_simd_than_fp32"] for n in lost), lost
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    res = resources("chain_bw_narrow_bf16")
    assert sum(len(res[s]) for s in SRC) == 9
    for s in SRC:
        assert sorted(res[s]) == list(WMAX), (s, sorted(res[s]))
        for w in WMAX:
            assert res[s][w]["scratch"] == 0 and res[s][w]["lds_static"] == 0, (s, w, res[s][w])
            assert sorted(res[s][w]) == sorted(rec["srcs"][s][str(w)]), (s, w)  # the committed record carries the same figures' keys
