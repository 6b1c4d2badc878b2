"""CPU-side checks of the fused Chain-block forward (gnx_chain_block_forward_narrow and its two queries): declared, exported and bound with
gnx_chain_block_forward's parameter lists; `_applies` and the workspace query return 0 on NULL, on bad arguments and for R <= 0; a too-small
workspace is refused in the name of the new query, without touching the caller's buffers; GNBlock carries the `narrow_chain` switch, off by
default; the nine instantiations of k_chain_mlp compile for gfx950 without scratch memory and the committed record lists them."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_chain_block_forward_narrow_applies", "gnx_chain_block_forward_narrow_workspace_bytes", "gnx_chain_block_forward_narrow")


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
    assert S["gnx_chain_block_forward_narrow"] == S["gnx_chain_block_forward"]
    assert S["gnx_chain_block_forward_narrow_workspace_bytes"] == S["gnx_chain_block_workspace_bytes"]
    assert S["gnx_chain_block_forward_narrow_applies"] == (C.c_int32, S["gnx_chain_block_workspace_bytes"][1])
    assert lib.gnx_version() == 130


def _params(gn, in_dims=(10, 5, 0), widths=((16, 3), (8, 4), (6, 5))):
    """gnx_chain_block_params over host arrays; the weight pointers are never read (every call below ends before any GPU work)"""
    L = gn._lib
    w = np.zeros(2048, dtype=np.float32)
    keep = [w]
    p = L.ChainBlockParams()
    p.de, p.dn, p.dg = in_dims
    for name, ws in zip(("edgefn", "nodefn", "graphfn"), widths):
        n = max(len(ws), 1)
        arr = (L.Dense * n)()
        for l in arr:
            l.weight = l.bias = w.ctypes.data
        wid = (C.c_int32 * n)(*ws)
        keep += [arr, wid]
        c = getattr(p, name)
        c.layers, c.widths, c.n_layers = arr, wid, len(ws)
    return p, keep


def _fake_handle(G=1, N=4, E=6):
    """a non-NULL "handle" whose leading counts (G, N, E) are all the calls below read before they refuse"""
    h = np.zeros(1024, dtype=np.int64)
    h[:3] = (G, N, E)
    return h


def test_queries_return_zero_on_null_bad_arguments_and_bad_replicas(lib):
    import graphnets_jl_amd as gn
    p, _keep = _params(gn)
    hbuf = _fake_handle(G=3)
    fake = C.c_void_p(hbuf.ctypes.data)
    for q in (lib.gnx_chain_block_forward_narrow_applies, lib.gnx_chain_block_forward_narrow_workspace_bytes):
        for h, pp in ((None, C.byref(p)), (fake, None), (None, None)):
            assert q(h, pp, 1) == 0
        for R in (0, -1, -7, 2, 65536):  # R <= 0; R > 1 on a batch of three graphs; beyond the grid
            assert q(fake, C.byref(p), R) == 0, R
        for bad in (dict(in_dims=(-1, 5, 0)), dict(in_dims=(0, 0, 0)), dict(widths=((16, -3), (8, 4), (6, 5))), dict(widths=((0, 3), (8, 4), (6, 5))),
                    dict(widths=((), (), ())), dict(widths=((3,) * 17, (8, 4), (6, 5)))):
            pb, _k = _params(gn, **bad)
            assert q(fake, C.byref(pb), 1) == 0, bad
        pb, _k = _params(gn)
        pb.edgefn.layers[0].act = 9
        assert q(fake, C.byref(pb), 1) == 0
        pb, _k = _params(gn)
        pb.nodefn.layers[1].kind = 1  # a LayerNorm that would change the width (8 -> 4)
        assert q(fake, C.byref(pb), 1) == 0
    # the rule itself, on the counts of the fake handle (no table is read by _applies)
    assert lib.gnx_chain_block_forward_narrow_applies(fake, C.byref(p), 1) == 7
    p33, _k = _params(gn, widths=((33, 3), (8, 4), (6, 5)))
    assert lib.gnx_chain_block_forward_narrow_applies(fake, C.byref(p33), 1) == 6
    pk, _k = _params(gn, in_dims=(10, 12, 0))  # K_e = 34
    assert lib.gnx_chain_block_forward_narrow_applies(fake, C.byref(pk), 1) == 6
    # the LDS budget of 10240 floats: 20 * 32 + 32, then 32 * 32 + 32 per layer, 32 * 4 + 4 for the last
    plds, _k = _params(gn, widths=((32,) * 10 + (3,), (8, 4), (6, 5)))  # 672 + 9 * 1056 + 132 = 10308
    assert lib.gnx_chain_block_forward_narrow_applies(fake, C.byref(plds), 1) == 6
    pfit, _k = _params(gn, widths=((32,) * 9 + (3,), (8, 4), (6, 5)))   # 672 + 8 * 1056 + 132 = 9252
    assert lib.gnx_chain_block_forward_narrow_applies(fake, C.byref(pfit), 1) == 7
    no_edges = _fake_handle(G=3, N=4, E=0)
    assert lib.gnx_chain_block_forward_narrow_applies(C.c_void_p(no_edges.ctypes.data), C.byref(p), 1) == 6


def test_refusals_name_the_new_query_and_write_nothing(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep = _params(gn)
    hbuf = _fake_handle()
    fake = C.c_void_p(hbuf.ctypes.data)
    buf = np.full(4096, 7.0, dtype=np.float32)
    ws = np.full(1024, 0x5A, dtype=np.uint8)
    b = buf.ctypes.data
    call = lambda h, pp, R, wsp, wsn, i=b, o=b: lib.gnx_chain_block_forward_narrow(h, pp, i, i, None, R, o, o, o, wsp, wsn, 0, None)
    assert call(None, C.byref(p), 1, ws.ctypes.data, ws.size) == L.ERR_INVALID_ARG
    assert call(fake, None, 1, ws.ctypes.data, ws.size) == L.ERR_INVALID_ARG
    assert call(fake, C.byref(p), 0, ws.ctypes.data, ws.size) == L.ERR_INVALID_ARG and b"n_replicas" in lib.gnx_last_error()
    assert call(fake, C.byref(p), 1, ws.ctypes.data, ws.size, i=None) == L.ERR_INVALID_ARG and b"input" in lib.gnx_last_error()
    assert call(fake, C.byref(p), 1, ws.ctypes.data, ws.size, o=None) == L.ERR_INVALID_ARG and b"output" in lib.gnx_last_error()
    # all three functions are fused: the workspace holds the graph function's input rows (and the layout's padding) — 16 bytes are too few
    for wsp, wsn in ((ws.ctypes.data, 16), (None, 1 << 20)):
        assert call(fake, C.byref(p), 1, wsp, wsn) == L.ERR_WORKSPACE
        assert b"gnx_chain_block_forward_narrow_workspace_bytes()" in lib.gnx_last_error()
    assert np.all(buf == 7.0) and np.all(ws == 0x5A)


def test_gnblock_has_the_switch_off_by_default():
    import graphnets_jl_amd as gn
    blk = gn.GNBlock((10, 5, 3), (3, 4, 5), device="cpu")
    assert blk.narrow_chain is False
    blk.narrow_chain = True
    assert blk.narrow_chain is True
    assert gn.GNBlock((10, 5, 3), (3, 4, 5), device="cpu", narrow_chain=True).narrow_chain is True
    assert "gnx_chain_block_forward_narrow" in gn.GNBlock.__doc__


def test_every_instantiation_compiles_without_scratch():
    from tools.kernel_resources import FAMILIES, HIPCC, resources
    LDS_BUDGET_BYTES, SRC, WMAX = (FAMILIES["chain_narrow"][k] for k in ("LDS_BUDGET_BYTES", "SRC", "WMAX"))
    with open(os.path.join(ROOT, "profiles", "chain_narrow_resources.json")) as f:
        rec = json.load(f)
    assert sorted(rec["srcs"]) == sorted(SRC) == ["edge", "node", "rows"] and rec["lds_budget_bytes"] == LDS_BUDGET_BYTES == 40960
    for s in SRC:
        assert sorted(int(k) for k in rec["srcs"][s]) == list(WMAX) == [8, 16, 32]
        assert all(v["scratch"] == 0 for v in rec["srcs"][s].values()), rec["srcs"][s]
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    res = resources("chain_narrow")
    for s in SRC:
        assert sorted(res[s]) == list(WMAX), (s, sorted(res[s]))
        for w in WMAX:
            assert res[s][w]["scratch"] == 0 and res[s][w]["lds_static"] == 0, (s, w, res[s][w])
