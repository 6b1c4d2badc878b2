"""CPU-side checks of the fused Chain-block pullback (gnx_chain_block_backward_narrow and its two queries): declared, exported and bound with
gnx_chain_block_backward's parameter lists; `_applies` and the workspace query return 0 on NULL, on bad arguments and on bad replicas; `_applies`
on a fake handle returns the mask that a Python restatement of the formula in include/gnx.h gives; a too-small workspace is refused in the name
of the new query, without touching the caller's buffers; GNBlock carries the `narrow_chain_backward` switch, off by default; the nine
instantiations of k_chain_mlp_bw compile for gfx950 without scratch memory and the committed record lists them."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests.test_chain_narrow_abi import _fake_handle, _params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_chain_block_backward_narrow_applies", "gnx_chain_block_backward_narrow_workspace_bytes", "gnx_chain_block_backward_narrow")


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
    assert S["gnx_chain_block_backward_narrow"] == S["gnx_chain_block_backward"]
    assert S["gnx_chain_block_backward_narrow_workspace_bytes"] == S["gnx_chain_block_backward_workspace_bytes"]
    assert S["gnx_chain_block_backward_narrow_applies"] == (C.c_int32, S["gnx_chain_block_backward_workspace_bytes"][1])
    assert lib.gnx_version() == 130


ceil4 = lambda x: (x + 3) & ~3


def formula_takes(k_in, widths, ln=(), rows=1):
    """include/gnx.h, gnx_chain_block_backward_narrow: the forward's rule and par + 2 (64 ld + P) <= 16384 floats.  `ln`: indices of LayerNorm layers"""
    n = len(widths)
    if n < 1 or n > 16 or rows == 0 or widths[-1] <= 0 or k_in > 32 or any(w > 32 for w in widths):
        return False
    par = P = 0
    k = k_in
    for i, w in enumerate(widths):
        par += 2 * ceil4(w) if i in ln else ceil4(k) * ceil4(w) + ceil4(w)
        P += 2 * w if i in ln else w * (k + 1)
        k = w
    if par > 10240:
        return False
    ld = (k_in + sum(widths[:-1]) + max(2 * w if i in ln else w for i, w in enumerate(widths))) | 1
    return par + 2 * (64 * ld + P) <= 16384


def formula_mask(in_dims, widths, counts=(1, 4, 6), ln=((), (), ())):
    de, dn, dg = in_dims
    G, N, E = counts
    ew, nw, gw = widths
    oe, on = (ew[-1] if ew else 0), (nw[-1] if nw else 0)
    return ((1 if formula_takes(de + 2 * dn + dg, ew, ln[0], E) else 0) | (2 if formula_takes(oe + dn + dg, nw, ln[1], N) else 0) |
            (4 if formula_takes(oe + on + dg, gw, ln[2], G) else 0))


def test_queries_return_zero_on_null_bad_arguments_and_bad_replicas(lib):
    import graphnets_jl_amd as gn
    p, _keep = _params(gn)
    hbuf = _fake_handle(G=3)
    fake = C.c_void_p(hbuf.ctypes.data)
    for q in (lib.gnx_chain_block_backward_narrow_applies, lib.gnx_chain_block_backward_narrow_workspace_bytes):
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
    # an edge function without output: the call refuses it, `_applies` says 0
    pz, _k = _params(gn, widths=((), (8, 4), (6, 5)))
    assert lib.gnx_chain_block_backward_narrow_applies(fake, C.byref(pz), 1) == 0


MASK_CASES = [
    ((10, 5, 0), ((16, 3), (8, 4), (6, 5))),
    # the two classes one wave's LDS covers — all widths <= 16 with 8 layers, all widths <= 32 with 3 layers: cut from the rule after the measurement
    # (include/gnx.h), so their functions that need more than half of the LDS per wave are outside it
    ((16, 0, 0), ((16,) * 8, (16,) * 8, (16,) * 7 + (8,))),            # K_e = K_n = 16 (K_g = 32)
    ((32, 0, 0), ((32, 32, 16), (32, 32, 16), (32, 32, 32))),          # K_e = 32, K_n = 16, K_g = 32
    ((2, 2, 1), ((8,) * 8, (3,), (2,))),
    # a 33-wide layer per function in turn
    ((10, 5, 0), ((33, 3), (8, 4), (6, 5))),
    ((10, 5, 0), ((16, 3), (33, 4), (6, 5))),
    ((10, 5, 0), ((16, 3), (8, 4), (33, 5))),
    ((10, 12, 0), ((16, 3), (8, 4), (6, 5))),  # K_e = 34
    # the LDS budget: 32-wide hidden layers do not fit two waves' tapes and accumulators; the forward fuses them (a legitimate mixed case)
    ((32, 0, 0), ((32, 32, 32, 3), (8, 4), (6, 5))),
    ((32, 0, 0), ((32, 32, 32), (8,), (4,))),
    ((8, 8, 8), ((32, 32, 32, 7), (32,) * 4, (16,) * 9)),
]


def test_applies_is_the_documented_formula(lib):
    import graphnets_jl_amd as gn
    hbuf = _fake_handle()  # G = 1, N = 4, E = 6: no table is read by _applies
    fake = C.c_void_p(hbuf.ctypes.data)
    seen = set()
    for in_dims, widths in MASK_CASES:
        p, _k = _params(gn, in_dims=in_dims, widths=widths)
        want = formula_mask(in_dims, widths)
        assert lib.gnx_chain_block_backward_narrow_applies(fake, C.byref(p), 1) == want, (in_dims, widths, want)
        seen.add(want)
    assert formula_mask(*MASK_CASES[0]) == 7 and formula_mask(*MASK_CASES[1]) == 0 and formula_mask(*MASK_CASES[2]) == 0 and formula_mask(*MASK_CASES[3]) == 7
    assert [formula_mask(*c) for c in MASK_CASES[4:8]] == [6, 5, 3, 6]
    assert formula_mask(*MASK_CASES[8]) == 6 and lib.gnx_chain_block_forward_narrow_applies(fake, C.byref(_params(gn, *MASK_CASES[8])[0]), 1) == 7
    # LayerNorm layers: their accumulators are 2 w, their parked deltas 2 w
    p, _k = _params(gn, in_dims=(32, 0, 0), widths=((32, 32, 16), (16, 32, 9), (32, 32, 4)))
    for ch, i in ((p.edgefn, 1), (p.nodefn, 0), (p.graphfn, 1)):
        ch.layers[i].kind = 1
    want = formula_mask((32, 0, 0), ((32, 32, 16), (16, 32, 9), (32, 32, 4)), ln=((1,), (0,), (1,)))
    assert lib.gnx_chain_block_backward_narrow_applies(fake, C.byref(p), 1) == want == 2  # (the edge and graph functions need more than half of the LDS per wave: cut)
    # E = 0 clears bit 0
    p, _k = _params(gn)
    no_edges = _fake_handle(G=3, N=4, E=0)
    assert lib.gnx_chain_block_backward_narrow_applies(C.c_void_p(no_edges.ctypes.data), C.byref(p), 1) == formula_mask((10, 5, 0), ((16, 3), (8, 4), (6, 5)), (3, 4, 0)) == 6


def test_refusals_name_the_new_query_and_write_nothing(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep = _params(gn)
    hbuf = _fake_handle()
    fake = C.c_void_p(hbuf.ctypes.data)
    buf = np.full(4096, 7.0, dtype=np.float32)
    ws = np.full(1024, 0x5A, dtype=np.uint8)
    b = buf.ctypes.data
    call = lambda h, pp, R, wsp, wsn, i=b: lib.gnx_chain_block_backward_narrow(h, pp, i, i, None, b, b, b, R, b, b, None, None, wsp, wsn, None)
    assert call(None, C.byref(p), 1, ws.ctypes.data, ws.size) == L.ERR_INVALID_ARG
    assert call(fake, None, 1, ws.ctypes.data, ws.size) == L.ERR_INVALID_ARG
    assert call(fake, C.byref(p), 0, ws.ctypes.data, ws.size) == L.ERR_DIMS and b"n_replicas" in lib.gnx_last_error()  # (gnx_chain_block_backward's code)
    assert call(fake, C.byref(p), 1, ws.ctypes.data, ws.size, i=None) == L.ERR_INVALID_ARG and b"input" in lib.gnx_last_error()
    pz, _k = _params(gn, widths=((), (8, 4), (6, 5)))
    assert call(fake, C.byref(pz), 1, ws.ctypes.data, ws.size) == L.ERR_DIMS and b"edge function without output" in lib.gnx_last_error()
    # all three functions are fused: the workspace holds what crosses levels and the partial rows — 16 bytes are too few
    for wsp, wsn in ((ws.ctypes.data, 16), (None, 1 << 20)):
        assert call(fake, C.byref(p), 1, wsp, wsn) == L.ERR_WORKSPACE
        assert b"gnx_chain_block_backward_narrow_workspace_bytes()" in lib.gnx_last_error()
    assert np.all(buf == 7.0) and np.all(ws == 0x5A)


def test_gnblock_has_the_switch_off_by_default():
    import graphnets_jl_amd as gn
    blk = gn.GNBlock((10, 5, 3), (3, 4, 5), device="cpu")
    assert blk.narrow_chain_backward is False
    blk.narrow_chain_backward = True
    assert blk.narrow_chain_backward is True and blk.narrow_chain is False
    assert gn.GNBlock((10, 5, 3), (3, 4, 5), device="cpu", narrow_chain_backward=True).narrow_chain_backward is True
    assert "gnx_chain_block_backward_narrow" in gn.GNBlock.__doc__


def test_every_instantiation_compiles_without_scratch():
    from tools.kernel_resources import FAMILIES, HIPCC, resources
    LDS_BUDGET_BYTES, SRC, WMAX = (FAMILIES["chain_bw_narrow"][k] for k in ("LDS_BUDGET_BYTES", "SRC", "WMAX"))
    with open(os.path.join(ROOT, "profiles", "chain_bw_narrow_resources.json")) as f:
        rec = json.load(f)
    assert sorted(rec["srcs"]) == sorted(SRC) == ["edge", "node", "rows"] and rec["lds_budget_bytes"] == LDS_BUDGET_BYTES == 65536
    for s in SRC:
        assert sorted(int(k) for k in rec["srcs"][s]) == list(WMAX) == [8, 16, 32]
        assert all(v["scratch"] == 0 for v in rec["srcs"][s].values()), rec["srcs"][s]
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    res = resources("chain_bw_narrow")
    for s in SRC:
        assert sorted(res[s]) == list(WMAX), (s, sorted(res[s]))
        for w in WMAX:
            assert res[s][w]["scratch"] == 0 and res[s][w]["lds_static"] == 0, (s, w, res[s][w])
