"""CPU-side checks of the fused FeedForward pullback of the narrow GNCore backward (gnx_core_backward_narrow): the three entries are declared,
exported and bound with matching parameter counts — the call with gnx_core_backward_typed's parameter list behind (elem, dropout) —; a NULL
handle, NULL params, an unknown element type and a Dropout probability outside [0, 1] are refused before any GPU work without touching the
caller's buffers; both queries return 0 on NULL; the kernel file compiles for gfx950 and none of its sixteen instantiations uses scratch memory;
GNCore carries the `narrow_backward` switch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_core_backward_narrow_applies", "gnx_core_backward_narrow_workspace_bytes", "gnx_core_backward_narrow")


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
    res, args = S["gnx_core_backward_narrow"]
    typed = S["gnx_core_backward_typed"]
    assert res == typed[0] and args[:3] == typed[1][:3] and args[3] == C.POINTER(gn._lib.Dropout) and args[4:] == typed[1][3:]
    assert S["gnx_core_backward_narrow_workspace_bytes"] == S["gnx_core_backward_typed_workspace_bytes"]
    assert S["gnx_core_backward_narrow_applies"] == (C.c_int32, S["gnx_core_backward_typed_workspace_bytes"][1])
    assert lib.gnx_version() == 130


def _setup(gn):
    L = gn._lib
    p = L.CoreParams()
    p.block = L.BlockParams(10, 5, 3, 10, 5, 3)
    w = np.zeros(1024, dtype=np.float32)  # (never read: every call below fails before any GPU work)
    p.block.edgefn.weight = p.block.nodefn.weight = p.block.graphfn.weight = w.ctypes.data
    for i in range(3):
        p.ln1[i].gamma = p.ln1[i].beta = p.ln2[i].gamma = p.ln2[i].beta = w.ctypes.data
        p.ff[i].fc1.weight = p.ff[i].fc2.weight = w.ctypes.data
        p.ff[i].fc1.act = 1
    p.eps = 1e-5
    buf = np.full(64, 0x7fc0, dtype=np.uint16)
    gbuf = np.full(256, 7.0, dtype=np.float32)
    ws = np.full(1024, 0x5A, dtype=np.uint8)
    gr = L.CoreGrads()
    g = gbuf.ctypes.data
    gr.block = L.BlockGrads(*[L.DenseGrad(g, g) for _ in range(3)])
    for i in range(3):
        gr.ln1[i].gamma = gr.ln1[i].beta = gr.ln2[i].gamma = gr.ln2[i].beta = g
        gr.ff[i].fc1, gr.ff[i].fc2 = L.DenseGrad(g, g), L.DenseGrad(g, g)
    return p, w, buf, gbuf, ws, gr


def _call(lib, h, pp, elem, drop, b, grads, ws):
    return lib.gnx_core_backward_narrow(h, pp, elem, drop, *([b] * 6), 1, *([b] * 3), C.byref(grads), ws.ctypes.data, ws.size, None)


def test_null_handle_or_params_are_refused_before_gpu_work(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep, buf, gbuf, ws, grads = _setup(gn)
    fake = C.c_void_p(buf.ctypes.data)  # a non-NULL "handle" next to NULL params: refused before it is looked at
    for elem in (L.ELEM_F32, L.ELEM_BF16):
        for h, pp in ((None, C.byref(p)), (fake, None), (None, None)):
            assert lib.gnx_core_backward_narrow_applies(h, pp, 1, elem) == 0
            assert lib.gnx_core_backward_narrow_workspace_bytes(h, pp, 1, elem) == 0
            assert _call(lib, h, pp, elem, None, buf.ctypes.data, grads, ws) == L.ERR_INVALID_ARG
            assert b"NULL" in lib.gnx_last_error()
    assert np.all(buf == 0x7fc0) and np.all(gbuf == 7.0) and np.all(ws == 0x5A)


def test_bad_elem_and_bad_dropout_are_refused_before_gpu_work(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep, buf, gbuf, ws, grads = _setup(gn)
    fake = C.c_void_p(buf.ctypes.data)  # a non-NULL "handle": refused before it is looked at
    for elem in (-1, 0, 1, 2, 4, 6, 99):
        assert elem not in (L.ELEM_F32, L.ELEM_BF16)
        for h in (None, fake):
            assert lib.gnx_core_backward_narrow_applies(h, C.byref(p), 1, elem) == 0
            assert lib.gnx_core_backward_narrow_workspace_bytes(h, C.byref(p), 1, elem) == 0
        assert _call(lib, fake, C.byref(p), elem, None, buf.ctypes.data, grads, ws) == L.ERR_INVALID_ARG
        assert b"elem" in lib.gnx_last_error()
    for prob in (-0.25, 1.5, float("nan"), float("inf")):
        for elem in (L.ELEM_F32, L.ELEM_BF16):
            drop = L.Dropout(prob, 0, 7)
            assert _call(lib, fake, C.byref(p), elem, C.byref(drop), buf.ctypes.data, grads, ws) == L.ERR_INVALID_ARG
            assert b"Dropout" in lib.gnx_last_error()
    # bfloat16 features with an active Dropout: no typed training-mode forward exists
    drop = L.Dropout(0.3, 0, 7)
    assert _call(lib, fake, C.byref(p), L.ELEM_BF16, C.byref(drop), buf.ctypes.data, grads, ws) == L.ERR_INVALID_ARG
    assert b"bf16" in lib.gnx_last_error()
    assert np.all(buf == 0x7fc0) and np.all(gbuf == 7.0) and np.all(ws == 0x5A)


def test_every_instantiation_compiles_without_scratch():
    from tools.kernel_resources import FAMILIES, HIPCC, resources
    WIDTHS = FAMILIES["core_bw_narrow"]["WIDTHS"]
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    res = resources("core_bw_narrow")
    assert sorted(res) == list(WIDTHS) == list(range(1, 17)), sorted(res)
    for d in WIDTHS:
        assert res[d]["scratch"] == 0, (d, res[d])
        assert res[d]["lds"] <= 64 * 1024, (d, res[d])
    assert 2 * res[10]["lds"] <= 160 * 1024, res[10]  # more than one workgroup per CU at README ex.3's edge width
    with open(os.path.join(ROOT, "profiles", "core_bw_narrow_resources.json")) as f:
        rec = __import__("json").load(f)
    assert sorted(int(k) for k in rec["widths"]) == list(WIDTHS) and all(v["scratch"] == 0 for v in rec["widths"].values())


def test_the_float64_anchor_draws_are_kink_free_within_the_round_limit():
    """the seeds tests/test_gpu_core_bw_narrow.py uses for its float64 case yield a kink-free draw (tests/util.py: kinkfree_core_inputs, 20 rounds)"""
    from oracle import gn_oracle as O
    from tests import util as U
    from tests.test_gpu_core_bw_narrow import ANCHOR_DIMS, RAGGED_EDGES, _seed
    rows = (sum(RAGGED_EDGES), 62, 5)  # the "ragged" batch
    for dims in ANCHOR_DIMS:
        rng = np.random.default_rng(_seed("ragged", 1, dims, "relu"))
        p = O.make_core_params(rng, dims)
        xs, rounds, _ = U.kinkfree_core_inputs(rng, p, 1, *rows)
        assert rounds <= 10, (dims, rounds)
        assert not any(U.relu_kink_rows(p, t, v).any() for t, v in zip("eng", xs))


def test_gncore_has_the_switch():
    import graphnets_jl_amd as gn
    core = gn.GNCore((10, 5, 3), device="cpu")
    assert core.narrow_backward is False and core.bf16_backward is False and core.block.narrow_backward is False
    core.narrow_backward = True
    assert core.narrow_backward is True and core.bf16_backward is False and core.block.narrow_backward is False
    core = gn.GNCore((10, 5, 3), device="cpu", narrow_backward=True)
    assert core.narrow_backward is True and core.bf16 is False and core.bf16_backward is False
    core = gn.GNCore((16, 16, 16), device="cpu", narrow_backward=True, bf16=True, bf16_backward=True)
    assert core.narrow_backward is True and core.bf16 is True and core.bf16_backward is True
    assert core.block.narrow_backward is False  # (the core's inner block is not touched)
    assert "gnx_core_backward_narrow" in gn.GNCore.__doc__
