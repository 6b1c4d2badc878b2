"""gnx_core_forward_train_typed / gnx_core_backward_train_typed on the GPU, through the ABI: a GNCore in training mode (an active Dropout)
on float32 and bfloat16 features, with the mask applied inside one FeedForward kernel per entity where the core is narrow (FUSED:
k_core_post_train, csrc/gnx_core_train_narrow.hip).

Every call runs inside one sentinel arena (tests/arena.py) with every buffer at its exact size and the workspace exactly what the query of the
entry returns; `arena.check` after every call asserts that nothing outside outputs and workspace was written and that the inputs are what
they were.  Cases, parameters and the backward's arenas are those of tests/test_gpu_core_bw_narrow.py.

Batches: "tiny", "ragged", "one", "noedges" (that file's), a single graph of N = E = rows for rows in {1, 63, 65, 257} (the 64 / 256-row
boundaries of a wave and a workgroup), and "wide": 8 graphs, 4160 nodes and 5600 edges (the matrix-core kernels of the unfused path)."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

from oracle import gn_oracle as O
from tests import arena as AR
from tests import test_gpu_core_bw_narrow as BN
from tests import test_gpu_memory_contract as MC
from tests import util as U
from tests.test_gpu_core_bw_narrow import DX, GRADS, NARROW, TRAIN, TYPED, WS_FILL, case, compare, same

pytestmark = pytest.mark.gpu

OUTS = ("ef_out", "nf_out", "gf_out")
TT, FT, FTRAIN = "train_typed", "typed", "train"  # forward entries
P = 0.3


@pytest.fixture(scope="module")
def gn():
    import torch
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def own_graphs(name):
    """"rows<k>": one graph of k nodes and k edges; "wide": 8 graphs of 520 nodes and 700 edges each"""
    import graphnets_jl_amd as gn
    sizes, edges = ((520,) * 8, (700,) * 8) if name == "wide" else ((int(name[4:]),), (int(name[4:]),))
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    cps, rvs = [], []
    for n, e in zip(sizes, edges):
        k = np.sort(rng.choice(n * n, e, replace=False))
        colptr = np.zeros(n + 1, dtype=np.int64)
        np.add.at(colptr, k // n + 1, 1)
        cps.append(np.cumsum(colptr)); rvs.append((k % n).astype(np.int64))
    g = gn.GNGraphBatch.from_csc(cps, rvs, list(sizes))
    assert g.n_edges == sum(edges) and g.n_nodes == sum(sizes) and g.n_graphs == len(sizes)
    return g


class OwnCase(BN.Case):
    """BN.Case on one of this file's batches"""

    def __init__(self, gn, batch, R, dims, act, seed, bf16=False):
        import torch
        self.gn, self.dims, self.act, self.R, self.what = gn, dims, act, R, f"{batch} R={R} {dims} {act}"
        self.g = own_graphs(batch)
        rng = np.random.default_rng(seed)
        self.p = O.make_core_params(rng, dims)
        self.rows = (self.g.n_edges, self.g.n_nodes, self.g.n_graphs)
        self.x = [torch.from_numpy((a * 4 - 2).astype(np.float32)) for a in U.packed_inputs(rng, R, *self.rows, dims)]
        self.cots = [torch.from_numpy(rng.standard_normal(tuple(t.shape)).astype(np.float32)) for t in self.x]
        if bf16:
            self.x = [t.to(torch.bfloat16).float() for t in self.x]
            self.cots = [t.to(torch.bfloat16).float() for t in self.cots]


@functools.lru_cache(maxsize=None)
def own_case(batch, R, dims, act, bf16=False):
    import graphnets_jl_amd as gn
    return OwnCase(gn, batch, R, dims, act, BN._seed(batch, R, dims, act), bf16)


def _elem(gn, bf16):
    return gn._lib.ELEM_BF16 if bf16 else gn._lib.ELEM_F32


def _active(drop):
    return drop is not None and drop.p > 0


def fwd_arena(c, entry, bf16=False, flags=0, drop=None, skew=None):
    """the arena of one forward call: (arena, call) — call(a, dropout, **overrides) -> status.  `drop` sizes the workspace of TT: the typed
    test-mode query without an active Dropout, gnx_core_train_typed_workspace_bytes with one."""
    import torch
    gn, g, R = c.gn, c.g, c.R
    L, lib = gn._lib, gn._lib.load()
    elem = _elem(gn, bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    a = AR.Arena("cuda", skew=skew)
    MC._decl_core(a, c.p)
    ins = [a.input(n, t.to(dt)) for n, t in zip(("ef", "nf", "gf"), c.x)]
    outs = [a.output(n, t.shape, dt) for n, t in zip(OUTS, c.x)]

    def query():
        cp = c.cp(a)
        if entry == FTRAIN:
            n = int(lib.gnx_core_train_workspace_bytes(g._h, C.byref(cp), R))
        elif entry == FT or not _active(drop):
            n = int(lib.gnx_core_typed_workspace_bytes(g._h, C.byref(cp), R, elem, flags))
        else:
            n = int(lib.gnx_core_train_typed_workspace_bytes(g._h, C.byref(cp), R, elem, flags))
        assert n > 0, lib.gnx_last_error()
        return n

    ws = a.workspace("ws", query)

    def call(a, dropout, **over):
        cp = c.cp(a)
        dp = None if dropout is None else C.byref(dropout)
        tail = (*map(a.ptr, ins), R, *map(a.ptr, outs), a.ptr(ws), over.get("ws_bytes", a.nbytes(ws)), over.get("flags", flags), _stream())
        if entry == FTRAIN:
            rc = lib.gnx_core_forward_train(g._h, C.byref(cp), dp, *tail)
        elif entry == FT:
            rc = lib.gnx_core_forward_typed(g._h, C.byref(cp), elem, *tail)
        else:
            rc = lib.gnx_core_forward_train_typed(g._h, C.byref(cp), over.get("elem", elem), dp, *tail)
        torch.cuda.synchronize()
        return rc

    return a, call


def fwd(c, entry, bf16=False, drop=None, flags=0, ws_fill=WS_FILL, skew=None, profile=None):
    """one forward call inside its arena: {name: a copy of the output tensor}"""
    a, call = fwd_arena(c, entry, bf16, flags, drop, skew)
    a.build(ws_fill=ws_fill)
    what = f"{c.what} forward {entry} bf16={bf16} p={None if drop is None else drop.p} flags={flags}"
    if profile is not None:
        c.gn.profile_reset(); c.gn.profile_enable(True)
    try:
        assert call(a, drop) == 0, f"{what}: {c.gn._lib.load().gnx_last_error()}"
    finally:
        if profile is not None:
            c.gn.profile_enable(False)
            profile.update(c.gn.profile_read()); c.gn.profile_reset()
    a.check(what)
    c.fwd_ws_bytes = a.nbytes("ws")
    return {n: a.view(n).clone() for n in OUTS}


def bwd_arena(c, bf16, narrow):
    """the arena of tests/test_gpu_core_bw_narrow.py for the entry whose plan this is, with gnx_core_backward_train_typed as the call"""
    import torch
    gn, g, R = c.gn, c.g, c.R
    L, lib = gn._lib, gn._lib.load()
    elem = _elem(gn, bf16)
    a, _ = c.arena(NARROW if narrow else TYPED, elem)
    names = ("ef", "nf", "gf", "g_ef_out", "g_nf_out", "g_gf_out")

    def call(a, dropout, **over):
        G = a.ptr
        gr = L.CoreGrads()
        gr.block = L.BlockGrads(*[L.DenseGrad(G(f"grad.{fn}.dW"), G(f"grad.{fn}.db")) for fn in ("edgefn", "nodefn", "graphfn")])
        for i, t in enumerate("eng"):
            gr.ln1[i].gamma, gr.ln1[i].beta = G(f"grad.ln1_{t}.gamma"), G(f"grad.ln1_{t}.beta")
            gr.ln2[i].gamma, gr.ln2[i].beta = G(f"grad.ln2_{t}.gamma"), G(f"grad.ln2_{t}.beta")
            gr.ff[i].fc1 = L.DenseGrad(G(f"grad.ff_{t}.fc1.dW"), G(f"grad.ff_{t}.fc1.db"))
            gr.ff[i].fc2 = L.DenseGrad(G(f"grad.ff_{t}.fc2.dW"), G(f"grad.ff_{t}.fc2.db"))
        cp = c.cp(a)
        assert int(lib.gnx_core_backward_train_typed_workspace_bytes(g._h, C.byref(cp), R, elem, narrow)) == a.nbytes("ws")
        dp = None if dropout is None else C.byref(dropout)
        rc = lib.gnx_core_backward_train_typed(g._h, C.byref(cp), over.get("elem", elem), dp, over.get("narrow", narrow), *map(a.ptr, names), R, *map(a.ptr, DX),
                                               C.byref(gr), a.ptr("ws"), a.nbytes("ws"), _stream())
        torch.cuda.synchronize()
        return rc

    return a, call


def bwd(c, bf16, narrow, drop, ws_fill=WS_FILL):
    a, call = bwd_arena(c, bf16, narrow)
    a.build(ws_fill=ws_fill)
    what = f"{c.what} backward train_typed bf16={bf16} narrow={narrow}"
    assert call(a, drop) == 0, f"{what}: {c.gn._lib.load().gnx_last_error()}"
    a.check(what)
    return {cv.name: a.view(cv.name).clone() for cv in a.carves if cv.kind == AR.OUTPUT}


def fused(c, bf16=False):
    a = AR.Arena("cuda")
    MC._decl_core(a, c.p)
    a.build()
    lib = c.gn._lib.load()
    cp = c.cp(a)
    r = int(lib.gnx_core_train_fused_applies(c.g._h, C.byref(cp), c.R, _elem(c.gn, bf16)))
    assert r == int(lib.gnx_core_backward_narrow_applies(c.g._h, C.byref(cp), c.R, _elem(c.gn, bf16)))  # one rule
    return r


def masks_of(c, drop):
    """the library's masks of the call, packed [R][rows][d] like the features"""
    return [c.gn.dropout_mask(drop, t, (c.dims[t], c.rows[t], c.R), "cuda").permute(2, 1, 0).contiguous() for t in range(3)]


# ---- 1. the kernel's mask is gnx_dropout_mask's, element for element ----
MASK_DIMS = [(1, 3, 10), (3, 10, 16), (10, 16, 1), (16, 1, 3)]  # every entity at every D of {1, 3, 10, 16}; never (1,1,1): tests/test_gpu_jit.py counts that
                                                               # block's run-time specialisation in the process of the suite


@pytest.mark.parametrize("dims", MASK_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_mask_identity(gn, dims):
    """the elements where y(p = 0.3) carries the bits of y(p = 1) (= x + b exactly) are exactly the zeros of gnx_dropout_mask for that entity: a wrong
    Philox index at an odd width, at a 64 / 256-row boundary or across replicas moves that set"""
    import torch
    L = gn._lib
    batches = [(f"rows{rows}", R) for rows in (1, 63, 65, 257) for R in (1, 2)] + [("ragged", 1)]  # G = 1 with replicas, and several graphs
    for batch, R in batches:
        c = case(batch, R, dims, "relu") if batch == "ragged" else own_case(batch, R, dims, "relu")
        assert fused(c) == 1
        drop, all_ = L.Dropout(P, 0, BN._seed("mask", batch, R, dims)), L.Dropout(1.0, 0, 1)
        y, y1 = fwd(c, TT, drop=drop), fwd(c, TT, drop=all_)
        for t, (n, m) in enumerate(zip(OUTS, masks_of(c, drop))):
            kept = BN._bits(y[n]).cpu() != BN._bits(y1[n]).cpu()
            assert torch.equal(kept, m.cpu() != 0), f"{c.what} {n}: {int((kept != (m.cpu() != 0)).sum())} of {m.numel()} elements disagree with gnx_dropout_mask"
            assert 0 < int(kept.sum()) < m.numel() or m.numel() < 8, (c.what, n)
    # bf16 rows: a dropped element is to_bf16(x + b) (a kept one may round to the same bits)
    c = own_case("rows257", 2, dims, "relu", bf16=True)
    drop = L.Dropout(P, 0, 99)
    y, y1 = fwd(c, TT, True, drop=drop), fwd(c, TT, True, drop=L.Dropout(1.0, 0, 1))
    for n, m in zip(OUTS, masks_of(c, drop)):
        dropped = m == 0
        assert torch.equal(BN._bits(y[n])[dropped], BN._bits(y1[n])[dropped]), (c.what, n)


# ---- 2. the fused forward against float64 ----
@pytest.mark.parametrize("dims,act", [((10, 5, 3), "relu"), ((3, 4, 5), "relu"), ((16, 16, 16), "relu"), ((2, 3, 1), "identity")],
                         ids=["10x5x3", "3x4x5", "16x16x16", "2x3x1-identity"])
def test_fused_forward_against_float64(gn, dims, act):
    """x + b + m .* f in float64 with the library's masks handed in (tests/test_gpu_dropout.py::_case); the project's bound: elementwise
    1e-5 . (1 + 2 / (1 - p)) . S with S the oracle's worst-case scale, and normwise 1e-5 . max|ref|"""
    import torch
    c = case("ragged", 1, dims, act)
    assert fused(c) == 1
    drop = gn._lib.Dropout(P, 0, 0xC0FFEE)
    seen = {}
    y = fwd(c, TT, drop=drop, profile=seen)
    assert seen["k_core_post"]["launches"] == 3 and seen["k_ln1_rows"]["launches"] == 3 and "k_dropout" not in seen and "train_ff1" not in seen, seen
    g = c.g
    csc = (*g.csc(), g.node_off, g.edge_off)
    W, Wb = MC._core_leaves(c.p)
    xs = [torch.tensor(t[0].numpy(), dtype=torch.float64) for t in c.x]
    masks = [m[0].double().cpu() for m in masks_of(c, drop)]
    hidden = {"relu": torch.relu, "identity": lambda v: v}[act]
    ref = MC._torch_core(c.p, csc, xs, W, Wb, hidden, masks)
    _, scale = O.core_forward_sparse(c.p, csc, *(t.numpy() for t in c.x), return_scale=True)
    for n, r, So in zip(OUTS, ref, scale):
        r = r.detach()
        err = (y[n][0].double().cpu() - r).abs().numpy()
        bound = 1e-5 * (1.0 + 2.0 / (1.0 - P)) * np.asarray(So[0], dtype=np.float64) + 1e-30
        print(f"BOUND {c.what} {n}: worst ratio {float((err / bound).max()):.3f}, normwise {float(err.max()) / float(r.abs().max()):.3e}")
        assert float((err / bound).max()) <= 1.0, f"{n}: worst ratio to the elementwise bound {float((err / bound).max()):.3f}"
        assert float(err.max()) <= 1e-5 * float(r.abs().max()), f"{n}: normwise {float(err.max()) / float(r.abs().max()):.3e}"


# ---- 3. the forward, bit for bit ----
def _skew4(cv):
    return 4 if cv.name in ("ef", "nf", "gf") + OUTS else 0  # the feature buffers at 256 k + 4: 4-byte but not 16-byte aligned


@pytest.mark.parametrize("batch,R,dims,act", [("ragged", 1, (10, 5, 3), "relu"), ("one", 2, (3, 4, 5), "relu"), ("ragged", 1, (2, 3, 1), "identity"),
                                              ("tiny", 1, (16, 16, 16), "relu")], ids=["ragged-10x5x3", "one-R2-3x4x5", "ragged-2x3x1", "tiny-16x16x16"])
def test_fused_bf16_is_the_rounded_f32_call(gn, batch, R, dims, act):
    import torch
    c = case(batch, R, dims, act, bf16=True)
    assert fused(c, True) == 1 and fused(c, False) == 1
    drop = gn._lib.Dropout(P, 0, 7)
    ref = fwd(c, TT, False, drop=drop)  # GNX_ELEM_F32 on the exactly widened inputs
    seen = {}
    got = fwd(c, TT, True, drop=drop, profile=seen)
    assert "k_bf16_widen" not in seen and "k_bf16_round" not in seen and "k_dropout" not in seen, sorted(seen)  # no fp32 copy of a bf16 tensor
    skewed = fwd(c, TT, True, drop=drop, skew=_skew4)
    for n in OUTS:
        same(got[n], ref[n].to(torch.bfloat16), f"{c.what} {n}")
        same(skewed[n], got[n], f"{c.what} {n} at 4-byte aligned buffers")
    f32_skewed = fwd(c, TT, False, drop=drop, skew=_skew4)
    for n in OUTS:
        same(f32_skewed[n], ref[n], f"{c.what} f32 {n} at 4-byte aligned buffers")


@pytest.mark.parametrize("batch,dims,act", [("ragged", (40, 36, 33), "tanh"), ("wide", (128, 64, 32), "relu")], ids=["40x36x33-tanh", "wide-128x64x32"])
def test_off_the_fused_path(gn, batch, dims, act):
    """bf16: bit for bit to_bf16(gnx_core_forward_train(widened inputs)); fp32: gnx_core_forward_train itself, and its workspace"""
    import torch
    c = own_case(batch, 1, dims, act, bf16=True) if batch == "wide" else case(batch, 1, dims, act, bf16=True)
    if batch == "wide":
        assert min(c.rows[0], c.rows[1]) >= 4096
    assert fused(c, True) == 0 and fused(c, False) == 0
    drop = gn._lib.Dropout(P, 0, 11)
    ref = fwd(c, FTRAIN, drop=drop)
    train_bytes = c.fwd_ws_bytes
    f32 = fwd(c, TT, False, drop=drop)
    assert c.fwd_ws_bytes == train_bytes
    seen = {}
    got = fwd(c, TT, True, drop=drop, profile=seen)
    assert "k_bf16_round" not in seen and seen["k_dropout"]["launches"] == 3 and seen["k_bf16_widen"]["launches"] >= 3, seen  # one pass stores bf16
    for n in OUTS:
        same(f32[n], ref[n], f"{c.what} f32 {n}")
        same(got[n], ref[n].to(torch.bfloat16), f"{c.what} bf16 {n}")


@pytest.mark.parametrize("dims", [(10, 5, 3), (3, 4, 5), (40, 36, 33)], ids=lambda d: "x".join(map(str, d)))
def test_without_an_active_dropout_it_is_the_typed_forward(gn, dims):
    c = case("ragged", 1, dims, "relu", bf16=True)
    for bf16 in (False, True):
        ref = fwd(c, FT, bf16)
        for drop in (None, gn._lib.Dropout(0.0, 0, 5)):
            got = fwd(c, TT, bf16, drop=drop)
            for n in OUTS:
                same(got[n], ref[n], f"{c.what} bf16={bf16} p={None if drop is None else 0} {n}")


# ---- 4. the backward, bit for bit ----
BW_CASES = [("ragged", (10, 5, 3), 0), ("ragged", (10, 5, 3), 1), ("ragged", (2, 3, 1), 0), ("ragged", (2, 3, 1), 1), ("ragged", (40, 36, 33), 0),
            ("noedges", (10, 5, 3), 0), ("noedges", (10, 5, 3), 1)]


@pytest.mark.parametrize("batch,dims,narrow", BW_CASES, ids=[f"{b}-{'x'.join(map(str, d))}-narrow{n}" for b, d, n in BW_CASES])
def test_backward_equals_its_reference(gn, batch, dims, narrow):
    """ref on the exactly widened tensors under the same dropout — narrow = 0: gnx_core_backward_train; narrow = 1: gnx_core_backward_narrow(F32) —
    d_x bit for bit to_bf16(ref's), all 30 parameter gradients bit for bit ref's; with GNX_ELEM_F32 the call is ref itself"""
    import torch
    L = gn._lib
    c = case(batch, 1, dims, "relu", bf16=True)
    drop = L.Dropout(P, 0, 0xBEEF)
    ref = c.run(NARROW, L.ELEM_F32, dropout=drop) if narrow else c.run(TRAIN, dropout=drop)
    got = bwd(c, True, narrow, drop)
    f32 = bwd(c, False, narrow, drop)
    assert set(got) == set(ref) == set(f32) == set(DX) | set(GRADS)
    for n in sorted(ref):
        same(f32[n], ref[n], f"{c.what} narrow={narrow} f32 {n}")
        same(got[n], ref[n].to(torch.bfloat16) if n in DX else ref[n], f"{c.what} narrow={narrow} bf16 {n}")
    plain = bwd(c, True, narrow, None)
    if batch != "noedges":
        assert not torch.equal(BN._bits(plain["d_ef"]), BN._bits(got["d_ef"]))  # the mask took part
    compare(plain, c.run(NARROW if narrow else TYPED, L.ELEM_BF16), f"{c.what} narrow={narrow} without dropout")


# ---- 5. memory contract ----
def _refused(a, call, rc, **kw):
    """a refused call: outputs still at their 0xFF fill, the workspace at its own, nothing else touched"""
    assert call(a, **kw) == rc
    a.check("refused", unwritten=False)
    for cv in a.carves:
        if cv.nbytes and cv.kind == AR.OUTPUT:
            assert bool((a.raw(cv.name) == AR.UNWRITTEN).all()), cv.name
        elif cv.nbytes and cv.kind == AR.WORKSPACE:
            assert bool((a.raw(cv.name) == WS_FILL).all()), cv.name


FWD_CONTRACT = [("ragged", 1, (10, 5, 3), False), ("one", 2, (16, 16, 16), True), ("ragged", 1, (40, 36, 33), True), ("noedges", 1, (10, 5, 3), False),
                ("noedges", 1, (10, 5, 3), True)]


@pytest.mark.parametrize("batch,R,dims,bf16", FWD_CONTRACT, ids=[f"{b}-R{R}-{'x'.join(map(str, d))}-{'bf16' if h else 'f32'}" for b, R, d, h in FWD_CONTRACT])
def test_forward_memory_contract(gn, batch, R, dims, bf16):
    """exact sizes, nothing outside outputs and workspace written, inputs untouched (arena.check in every run); the same outputs whatever the
    workspace held; a refused call writes nothing"""
    L = gn._lib
    c = case(batch, R, dims, "relu", bf16=True)
    drop = L.Dropout(P, 0, 21)
    runs = [fwd(c, TT, bf16, drop=drop, ws_fill=0x00), fwd(c, TT, bf16, drop=drop, ws_fill=0xFF)]
    for n in OUTS:
        same(runs[1][n], runs[0][n], f"{c.what}: {n} depends on what the workspace held")
    a, call = fwd_arena(c, TT, bf16, 0, drop)
    a.build(ws_fill=WS_FILL)
    _refused(a, call, L.ERR_INVALID_ARG, dropout=L.Dropout(1.5, 0, 1))
    _refused(a, call, L.ERR_INVALID_ARG, dropout=drop, elem=7)
    _refused(a, call, L.ERR_INVALID_ARG, dropout=drop, flags=L.FLAG_DEFER_GRAPH_UPDATE)
    _refused(a, call, L.ERR_WORKSPACE, dropout=drop, ws_bytes=a.nbytes("ws") - 1)
    assert call(a, drop) == 0  # and the arena is still good for the call itself
    a.check(c.what)


@pytest.mark.parametrize("batch,dims,narrow", [("ragged", (10, 5, 3), 0), ("ragged", (10, 5, 3), 1), ("noedges", (10, 5, 3), 1)],
                         ids=["ragged-narrow0", "ragged-narrow1", "noedges-narrow1"])
def test_backward_memory_contract(gn, batch, dims, narrow):
    L = gn._lib
    c = case(batch, 1, dims, "relu", bf16=True)
    drop = L.Dropout(P, 0, 22)
    runs = [bwd(c, True, narrow, drop, ws_fill=0x00), bwd(c, True, narrow, drop, ws_fill=0xFF)]
    for n in runs[0]:
        same(runs[1][n], runs[0][n], f"{c.what}: {n} depends on what the workspace held")
    a, call = bwd_arena(c, True, narrow)
    a.build(ws_fill=WS_FILL)
    _refused(a, call, L.ERR_INVALID_ARG, dropout=drop, narrow=2)
    _refused(a, call, L.ERR_INVALID_ARG, dropout=L.Dropout(-0.25, 0, 1))
    _refused(a, call, L.ERR_INVALID_ARG, dropout=drop, elem=99)  # (3 and 5 are the two element codes the entry takes)


# ---- 6. capture ----
def _packed_core(gn, bf16):
    import torch
    dims = (10, 5, 3)
    g = BN.graphs("ragged")
    rng = np.random.default_rng(78)
    core = U.core_from_params(gn, O.make_core_params(rng, dims))
    x = [torch.from_numpy((a * 4 - 2).astype(np.float32)).cuda() for a in U.packed_inputs(rng, 1, g.n_edges, g.n_nodes, g.n_graphs, dims)]
    cot = [torch.from_numpy(rng.standard_normal(tuple(t.shape)).astype(np.float32)).cuda() for t in x]
    if bf16:
        x, cot = [t.to(torch.bfloat16) for t in x], [t.to(torch.bfloat16) for t in cot]
    return g, core, x, cot


def _pair(gn, g, core, x, cot, drop, elem, narrow, ws_f, ws_b, outs, dxs, gs):
    """one gnx_core_forward_train_typed + gnx_core_backward_train_typed pair on the current stream"""
    lib = gn._lib.load()
    keep = []
    cp = core._c(keep)
    gr = gn.api._core_grads(core, gs)
    s = _stream()
    assert lib.gnx_core_forward_train_typed(g._h, C.byref(cp), elem, C.byref(drop), *(t.data_ptr() for t in x), 1, *(t.data_ptr() for t in outs), ws_f.data_ptr(),
                                            ws_f.numel(), 0, s) == 0, lib.gnx_last_error()
    assert lib.gnx_core_backward_train_typed(g._h, C.byref(cp), elem, C.byref(drop), narrow, *(t.data_ptr() for t in x), *(t.data_ptr() for t in cot), 1,
                                             *(t.data_ptr() for t in dxs), C.byref(gr), ws_b.data_ptr(), ws_b.numel(), s) == 0, lib.gnx_last_error()


def _pair_buffers(gn, g, core, x, elem, narrow):
    import torch
    lib = gn._lib.load()
    keep = []
    cp = core._c(keep)
    ws_f = torch.empty(int(lib.gnx_core_train_typed_workspace_bytes(g._h, C.byref(cp), 1, elem, 0)), dtype=torch.uint8, device="cuda")
    ws_b = torch.empty(int(lib.gnx_core_backward_train_typed_workspace_bytes(g._h, C.byref(cp), 1, elem, narrow)), dtype=torch.uint8, device="cuda")
    mk = lambda: ([torch.empty_like(t) for t in x], [torch.empty_like(t) for t in x],
                  [torch.empty((q.shape[1], q.shape[0]), dtype=torch.float32, device="cuda").t() if q.dim() == 2 else torch.empty_like(q) for q in core.parameters()])
    return ws_f, ws_b, mk


def test_a_captured_pair_replays_the_eager_bits(gn):
    import torch
    L = gn._lib
    g, core, x, cot = _packed_core(gn, True)
    drop = L.Dropout(P, 0, 31)
    ws_f, ws_b, mk = _pair_buffers(gn, g, core, x, L.ELEM_BF16, 1)  # (the queries, outside the capture)
    eager, graphed = mk(), mk()
    _pair(gn, g, core, x, cot, drop, L.ELEM_BF16, 1, ws_f, ws_b, *eager)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(cg, stream=side):
            _pair(gn, g, core, x, cot, drop, L.ELEM_BF16, 1, ws_f, ws_b, *graphed)
    for _ in range(2):
        for group in graphed:
            for t in group:
                t.zero_()
        cg.replay()
        torch.cuda.synchronize()
        for ge, gg in zip(eager, graphed):
            for i, (u, v) in enumerate(zip(ge, gg)):
                same(v.contiguous(), u.contiguous(), f"replayed tensor {i}")


# ---- 7. Python ----
def test_python_end_to_end(gn):
    import torch
    L, lib = gn._lib, gn._lib.load()
    g, core0, x, cot = _packed_core(gn, True)
    core = gn.GNCore((10, 5, 3), dropout=0.25, bf16=True, bf16_backward=True, typed_dropout=True, narrow_backward=True)
    for name in ("block", "gn1", "gn2"):
        setattr(core, name, getattr(core0, name))
    core.ffwd.eff, core.ffwd.nff, core.ffwd.gff = core0.ffwd.eff, core0.ffwd.nff, core0.ffwd.gff
    assert core.ffwd.dropout == 0.25
    params = core.parameters()
    for t in params:
        t.requires_grad_(True)

    def step():
        for t in params:
            t.grad = None
        leaves = [t.permute(2, 1, 0).detach().requires_grad_(True) for t in x]
        y = core(gn.NT(g, *leaves))
        sum((o.float() * c.permute(2, 1, 0).float()).sum() for o, c in zip((y.ef, y.nf, y.gf), cot)).backward()
        torch.cuda.synchronize()
        pk = lambda t: t.detach().permute(2, 1, 0).contiguous()
        return [pk(y.ef), pk(y.nf), pk(y.gf)], [pk(t.grad) for t in leaves], [t.grad.clone() for t in params]

    torch.manual_seed(5)
    out, dx, gp = step()
    drop = core.last_dropout
    assert abs(drop.p - 0.25) < 1e-7
    ws_f, ws_b, mk = _pair_buffers(gn, g, core, x, L.ELEM_BF16, 1)
    ref = mk()
    _pair(gn, g, core, x, cot, drop, L.ELEM_BF16, 1, ws_f, ws_b, *ref)
    torch.cuda.synchronize()
    for i, (u, v) in enumerate(zip(out + dx, ref[0] + ref[1])):
        same(u, v, f"feature tensor {i}")
    for i, (u, v) in enumerate(zip(gp, ref[2])):
        same(u.contiguous(), v.contiguous(), f"grad of parameter {i}")
    torch.manual_seed(5)
    again = step()
    assert again[0] is not out
    for i, (u, v) in enumerate(zip(out + dx + gp, again[0] + again[1] + again[2])):
        same(u.contiguous(), v.contiguous(), f"tensor {i} after the same torch.manual_seed")
    # testmode: gnx_core_forward_typed's bits
    gn.testmode(core)
    y = core(gn.NT(g, *(t.permute(2, 1, 0) for t in x)))
    keep = []
    cp = core._c(keep)
    ws = torch.empty(int(lib.gnx_core_typed_workspace_bytes(g._h, C.byref(cp), 1, L.ELEM_BF16, 0)), dtype=torch.uint8, device="cuda")
    outs = [torch.empty_like(t) for t in x]
    assert lib.gnx_core_forward_typed(g._h, C.byref(cp), L.ELEM_BF16, *(t.data_ptr() for t in x), 1, *(t.data_ptr() for t in outs), ws.data_ptr(), ws.numel(), 0,
                                      _stream()) == 0
    torch.cuda.synchronize()
    for n, o in zip(("ef", "nf", "gf"), outs):
        same(getattr(y, n).detach().permute(2, 1, 0).contiguous(), o, f"testmode {n}")
    gn.testmode(core, None)
    # fp32 features through the same switch: the typed pair with GNX_ELEM_F32
    xf = [t.float() for t in x]
    core.bf16 = core.bf16_backward = False
    torch.manual_seed(6)
    leaves = [t.permute(2, 1, 0).detach().requires_grad_(True) for t in xf]
    y = core(gn.NT(g, *leaves))
    drop = core.last_dropout
    ws_f, _, _ = _pair_buffers(gn, g, core, xf, L.ELEM_F32, 1)
    outs = [torch.empty_like(t) for t in xf]
    cp = core._c(keep)
    assert lib.gnx_core_forward_train_typed(g._h, C.byref(cp), L.ELEM_F32, C.byref(drop), *(t.data_ptr() for t in xf), 1, *(t.data_ptr() for t in outs),
                                            ws_f.data_ptr(), ws_f.numel(), 0, _stream()) == 0
    torch.cuda.synchronize()
    for n, o in zip(("ef", "nf", "gf"), outs):
        same(getattr(y, n).detach().permute(2, 1, 0).contiguous(), o, f"fp32 {n}")
    # the switch off: refused as before
    core.bf16 = core.bf16_backward = True
    core.typed_dropout = False
    with pytest.raises(NotImplementedError, match="Dropout"):
        core(gn.NT(g, *(t.permute(2, 1, 0).detach().requires_grad_(True) for t in x)))
