"""gnx_core_backward_typed on the GPU.  The reference of every case is built here from the public fp32 entry: gnx_core_backward on .float() of
the same six bf16 tensors, every buffer at the same byte offset modulo 16, its three input gradients rounded with .to(torch.bfloat16).  Every
comparison is torch.equal on raw bits — no tolerance: the input gradients are bit for bit the rounded reference, each of the 30 parameter
gradients bit for bit the reference's.  Every call runs inside one sentinel arena (tests/arena.py): all buffers carved at their exact sizes,
outputs pre-filled with NaN bytes, the workspace with 0xA5.  Shapes are the smallest at which the typed kernels can go wrong: odd widths (rows
that start in the middle of a dword, a lone last 16-bit element), 3001 edge rows at widths 64 / 128 (the 16-lanes-per-row LayerNorm kernels with
a partial last workgroup, the matrix-core FeedForward pullbacks) beside 300 node rows and one graph row (the one-wave-per-row kernels),
replicas, graphs without edges, a batch without edges."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

from oracle import gn_oracle as O
from tests import arena as AR
from tests import test_gpu_memory_contract as MC  # the arena descriptors of a core (_decl_core, _core_params, _decl_dense_grad, _dense_grad)
from tests import util as U

pytestmark = pytest.mark.gpu

WS_FILL = 0xA5
FEATURES = ("ef", "nf", "gf", "g_ef_out", "g_nf_out", "g_gf_out", "d_ef", "d_nf", "d_gf")
BATCHES = ["tiny", "edgeless", "small40", "one", "one-R3"]
NARROW = [(10, 5, 3), (3, 4, 5)]   # README ex.3 (odd row widths); every kernel generic / narrow
WIDE = [(64, 64, 64), (128, 64, 32)]  # on `one`: _v4 LayerNorm kernels on the edge rows (Q = 1, 2), matrix-core FeedForward pullbacks
ACTS = ("relu", "gelu")


@pytest.fixture(scope="module")
def gn():
    import torch
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


@functools.lru_cache(maxsize=None)
def _graphs(name):
    import graphnets_jl_amd as gn
    if name == "one":
        colptr, rowval = U.er_csc(np.random.default_rng(1), 300, 3001)
        g = gn.GNGraphBatch.from_csc([colptr], [rowval], [300])
        assert g.n_edges == 3001 and g.n_nodes == 300
        return g
    if name == "small40":
        rng = np.random.default_rng(2)
        adjs = U.random_graphs(rng, [1, 1, 12, 2] + list(rng.integers(1, 13, 36)), 0.3)
        adjs[2][:] = 0  # a 12-node graph without edges
        adjs[5][:] = 0
        return gn.GNGraphBatch(adjs)
    if name == "edgeless":
        return gn.GNGraphBatch([np.zeros((n, n), dtype=np.int64) for n in (3, 5, 2)])
    assert name == "tiny"
    colptr, rowval = U.er_csc(np.random.default_rng(3), 5, 9)
    g = gn.GNGraphBatch.from_csc([colptr], [rowval], [5])
    assert g.n_edges == 9 and g.n_nodes == 5
    return g


def _batch(name):
    """(graphs, R)"""
    return (_graphs("one"), 3) if name == "one-R3" else (_graphs(name), 1)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _seed(*key):
    return zlib.crc32(repr(key).encode())  # (the same in every process, unlike hash())


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b, what):
    import torch
    assert (a is None) == (b is None), what
    if a is None:
        return
    assert a.dtype == b.dtype and a.shape == b.shape, what
    x, y = _bits(a), _bits(b)
    if not torch.equal(x, y):
        bad = (x != y).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {x.numel()} values differ, first at {i}: {a[i].item()!r} vs {b[i].item()!r}")


def _grad_names():
    """the 30 parameter gradients, in the order of gnx_core_grads"""
    names = []
    for fn in ("edgefn", "nodefn", "graphfn"):
        names += [f"grad.{fn}.dW", f"grad.{fn}.db"]
    for ln in ("ln1", "ln2"):
        for t in "eng":
            names += [f"grad.{ln}_{t}.gamma", f"grad.{ln}_{t}.beta"]
    for t in "eng":
        for fc in ("fc1", "fc2"):
            names += [f"grad.ff_{t}.{fc}.dW", f"grad.ff_{t}.{fc}.db"]
    return names


GRADS = _grad_names()
assert len(GRADS) == 30


class Case:
    """A core's parameters, its three bf16 inputs and three random bf16 cotangents: the six tensors of a backward call."""

    def __init__(self, gn, batch, dims, act, seed):
        import torch
        self.gn, self.dims, self.act, self.what = gn, dims, act, f"{batch} {dims} {act}"
        self.g, self.R = _batch(batch)
        rng = np.random.default_rng(seed)
        self.p = O.make_core_params(rng, dims)  # LayerNorm gammas in [0.5, 1.5], betas in [-0.1, 0.1]
        self.rows = (self.g.n_edges, self.g.n_nodes, self.g.n_graphs)
        # values of both signs over a few binades, rounded once to bf16 (the inputs ARE bf16)
        self.x = [torch.from_numpy((a * 4 - 2).astype(np.float32)).to(torch.bfloat16)
                  for a in U.packed_inputs(rng, self.R, *self.rows, dims)]
        self.cots = [torch.from_numpy(rng.standard_normal(tuple(t.shape)).astype(np.float32)).to(torch.bfloat16) for t in self.x]

    def arena(self, elem, cots=(True,) * 3, want_d=(True,) * 3, drop=(), skew=0, ws_extra=0):
        """the arena of one call in element type `elem`: (arena, call) — call(a, **overrides) -> status.  `drop`: names of parameter gradients
        passed as NULL; `skew`: bytes by which every feature buffer starts behind its 256-byte aligned start."""
        import torch
        gn, g, R, p = self.gn, self.g, self.R, self.p
        L, lib = gn._lib, gn._lib.load()
        bf = elem == L.ELEM_BF16
        dt = torch.bfloat16 if bf else torch.float32
        a = AR.Arena("cuda", skew=(lambda c: skew if c.name in FEATURES else 0) if skew else None)
        MC._decl_core(a, p)
        ins = [a.input(n, t.to(dt)) for n, t in zip(("ef", "nf", "gf"), self.x)]
        gs = [a.input(n, t.to(dt)) if keep else None for n, t, keep in zip(("g_ef_out", "g_nf_out", "g_gf_out"), self.cots, cots)]
        dx = [a.output(n, t.shape, dt) if keep else None for n, t, keep in zip(("d_ef", "d_nf", "d_gf"), self.x, want_d)]
        pb = p["block"]
        for fn, w, b in (("edgefn", "We", "be"), ("nodefn", "Wn", "bn"), ("graphfn", "Wg", "bg")):
            MC._decl_dense_grad(a, f"grad.{fn}", pb[w], pb[b])
        for t in "eng":
            for ln in ("ln1", "ln2"):
                a.output(f"grad.{ln}_{t}.gamma", p[f"{ln}_{t}_gamma"].shape)
                a.output(f"grad.{ln}_{t}.beta", p[f"{ln}_{t}_beta"].shape)
            MC._decl_dense_grad(a, f"grad.ff_{t}.fc1", p[f"ff_{t}_W1"], p[f"ff_{t}_b1"])
            MC._decl_dense_grad(a, f"grad.ff_{t}.fc2", p[f"ff_{t}_W2"], p[f"ff_{t}_b2"])
        act = L.ACT[self.act]
        cp_of = lambda: MC._core_params(gn, a, p, act)

        def query():
            cp = cp_of()
            n = int(lib.gnx_core_backward_typed_workspace_bytes(g._h, C.byref(cp), R, elem))
            if not bf:  # GNX_ELEM_F32 is exactly the fp32 query
                assert n == int(lib.gnx_core_backward_workspace_bytes(g._h, C.byref(cp), R))
            assert n > 0, lib.gnx_last_error()
            return n + ws_extra

        ws = a.workspace("ws", query)

        def call(a, grads_null=False, typed=True, **over):
            """`over`: elem, R, cp, ws (address), ws_bytes, or the name of one of the nine feature buffers -> its address"""
            P = lambda n: None if n is None else over.get(n, a.ptr(n))
            G = lambda n: None if n in drop else a.ptr(n)
            gr = L.CoreGrads()
            gr.block = L.BlockGrads(*[L.DenseGrad(G(f"grad.{fn}.dW"), G(f"grad.{fn}.db")) for fn in ("edgefn", "nodefn", "graphfn")])
            for i, t in enumerate("eng"):
                gr.ln1[i].gamma, gr.ln1[i].beta = G(f"grad.ln1_{t}.gamma"), G(f"grad.ln1_{t}.beta")
                gr.ln2[i].gamma, gr.ln2[i].beta = G(f"grad.ln2_{t}.gamma"), G(f"grad.ln2_{t}.beta")
                gr.ff[i].fc1 = L.DenseGrad(G(f"grad.ff_{t}.fc1.dW"), G(f"grad.ff_{t}.fc1.db"))
                gr.ff[i].fc2 = L.DenseGrad(G(f"grad.ff_{t}.fc2.dW"), G(f"grad.ff_{t}.fc2.db"))
            cp = over.get("cp") or cp_of()
            tail = (over.get("R", R), *map(P, dx), None if grads_null else C.byref(gr), over.get("ws", a.ptr(ws)), over.get("ws_bytes", a.nbytes(ws)), _stream())
            if typed:
                rc = lib.gnx_core_backward_typed(g._h, C.byref(cp), over.get("elem", elem), *map(P, ins), *map(P, gs), *tail)
            else:
                rc = lib.gnx_core_backward(g._h, C.byref(cp), *map(P, ins), *map(P, gs), *tail)
            torch.cuda.synchronize()
            return rc

        return a, call

    def run(self, elem, ws_fill=WS_FILL, grads_null=False, typed=True, **kw):
        """one call inside its arena: {name: a copy of the output tensor}; names of outputs that were not asked for are absent"""
        a, call = self.arena(elem, **kw)
        a.build(ws_fill=ws_fill)
        assert call(a, grads_null=grads_null, typed=typed) == 0, f"{self.what}: {self.gn._lib.load().gnx_last_error()}"
        skip = set(kw.get("drop", ())) | (set(GRADS) if grads_null else set())
        for n in skip:  # an output passed as NULL: its carve must still hold the bytes it was given
            assert bool((a.raw(n) == AR.UNWRITTEN).all()), f"{self.what}: {n} was written although NULL was passed"
            a.raw(n)[:] = 0
        a.check(f"{self.what} elem={elem} {kw}")
        return {c.name: a.view(c.name).clone() for c in a.carves if c.kind == AR.OUTPUT and c.name not in skip}

    def check(self, what="", **kw):
        """typed bf16 call == the fp32 entry on the widened six at the same addresses modulo 16, input gradients rounded"""
        import torch
        L = self.gn._lib
        ref = self.run(L.ELEM_F32, typed=False, **kw)
        got = self.run(L.ELEM_BF16, **kw)
        assert set(ref) == set(got)
        for n in sorted(got):
            want = ref[n].to(torch.bfloat16) if n in FEATURES else ref[n]
            _same(got[n], want, f"{self.what} {what} {n}")
            assert got[n].numel() == 0 or bool(torch.isfinite(got[n].float()).all()), f"{self.what} {what} {n}: not finite"
        return got


@functools.lru_cache(maxsize=None)
def _case(batch, dims, act, seed=0):
    import graphnets_jl_amd as gn
    return Case(gn, batch, dims, act, _seed(batch, dims, act, seed))


# one-R3 at width 64: the typed _v4 LayerNorm kernels and k_bf16_widen with replicas (9003 edge rows of three replicas)
CASES = [(b, d) for b in BATCHES for d in NARROW] + [("one", d) for d in WIDE] + [("one-R3", (64, 64, 64))]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("batch,dims", CASES, ids=[f"{b}-{'x'.join(map(str, d))}" for b, d in CASES])
def test_bits_equal_the_fp32_backward_of_the_widened_tensors(gn, batch, dims, act):
    got = _case(batch, dims, act).check()
    assert {"d_ef", "d_nf", "d_gf"} | set(GRADS) == set(got)  # all 3 input gradients and all 30 parameter gradients were compared


def test_the_wide_cases_take_the_kernels_they_are_there_for(gn):
    """(64,64,64) on `one`: the LayerNorm kernels run in both forms, the upstream gradients are widened, nothing is rounded by a pass"""
    L = gn._lib
    c = _case("one", (64, 64, 64), "relu")
    a, call = c.arena(L.ELEM_BF16)
    a.build(ws_fill=WS_FILL)
    gn.profile_reset(); gn.profile_enable(True)
    try:
        assert call(a) == 0
    finally:
        gn.profile_enable(False)
    seen = gn.profile_read(); gn.profile_reset()
    assert seen["k_layernorm2"]["launches"] == 3 and seen["bw_layernorm"]["launches"] == 3, seen
    assert seen["k_bf16_widen"]["launches"] == 3 and "k_bf16_round" not in seen, sorted(seen)
    if U.default_flags(gn) == 0:  # (forms switched on for the whole process change which kernels run, not the bits)
        assert "k_dw_gemm" in seen and "bw_dx_ff2" in seen, sorted(seen)  # the matrix-core FeedForward pullbacks


@pytest.mark.parametrize("batch,dims", [("small40", (10, 5, 3)), ("one", (64, 64, 64))], ids=["small40-10x5x3", "one-64x64x64"])
def test_optional_arguments(gn, batch, dims):
    """each cotangent NULL in turn and all three NULL, each d_* NULL, grads NULL, single gradient pointers NULL — NULL for both the reference
    and the typed call; the remaining outputs keep their bits"""
    c = _case(batch, dims, "gelu")
    for k in range(3):
        c.check(f"cotangent {k} NULL", cots=tuple(i != k for i in range(3)))
    c.check("all cotangents NULL", cots=(False,) * 3)
    full = c.check("everything")
    for k in range(3):
        got = c.check(f"d {k} NULL", want_d=tuple(i != k for i in range(3)))
        for n in got:
            _same(got[n], full[n], f"{c.what} d {k} NULL: {n} changed")
    got = c.check("grads NULL", grads_null=True)
    assert set(got) == {"d_ef", "d_nf", "d_gf"}
    for n in got:
        _same(got[n], full[n], f"{c.what} grads NULL: {n} changed")
    for drop in (("grad.edgefn.dW",), ("grad.ln1_e.gamma", "grad.ln2_n.beta"), ("grad.ff_e.fc1.db", "grad.ff_e.fc2.dW", "grad.ff_g.fc1.dW"),
                 tuple(GRADS[1:])):
        got = c.check(f"NULL {drop}", drop=drop)
        for n in got:
            _same(got[n], full[n], f"{c.what} NULL {drop}: {n} changed")


def test_f32_elem_is_gnx_core_backward(gn):
    """elem = GNX_ELEM_F32 is exactly gnx_core_backward: same workspace size (asserted in every fp32 arena), same bits"""
    L = gn._lib
    for batch, dims in (("small40", (10, 5, 3)), ("one", (64, 64, 64))):
        c = Case(gn, batch, dims, "relu", 5)
        c.x = [t.float() * 1.001 for t in c.x]  # (fp32 values that are no bf16 values)
        c.cots = [t.float() * 1.001 for t in c.cots]
        ref = c.run(L.ELEM_F32, typed=False)
        got = c.run(L.ELEM_F32, typed=True)
        for n in ref:
            _same(got[n], ref[n], f"{batch} f32 {n}")


def _untouched(a, what):
    """nothing was written: guards and inputs as built, outputs still NaN bytes, the workspace still its fill"""
    a.check(what, unwritten=False)
    for c in a.carves:
        if c.nbytes and c.kind == AR.OUTPUT:
            assert bool((a.raw(c.name) == AR.UNWRITTEN).all()), f"{what}: output {c.name} was written"
        elif c.nbytes and c.kind == AR.WORKSPACE:
            assert bool((a.raw(c.name) == WS_FILL).all()), f"{what}: the workspace was written"


def test_refusals_on_a_real_handle_write_nothing(gn):
    L, lib = gn._lib, gn._lib.load()
    c = _case("one", (10, 5, 3), "relu")
    a, call = c.arena(L.ELEM_BF16, ws_extra=16)
    a.build(ws_fill=WS_FILL)
    need, wsp = a.nbytes("ws") - 16, a.ptr("ws")

    def refuse(code, what, **over):
        rc = call(a, **over)
        assert rc == code, f"{what}: status {rc}, {lib.gnx_last_error()}"
        _untouched(a, what)

    refuse(L.ERR_WORKSPACE, "short workspace", ws_bytes=need - 1)
    refuse(L.ERR_WORKSPACE, "no workspace", ws=None)
    for k in (4, 8):
        refuse(L.ERR_WORKSPACE, f"workspace at +{k}", ws=wsp + k, ws_bytes=need + 16 - k)
    for n in FEATURES:
        refuse(L.ERR_INVALID_ARG, f"{n} at +2", **{n: a.ptr(n) + 2})
        assert b"4-byte aligned" in lib.gnx_last_error(), n
    for elem in (7, -1, 0, 4):
        refuse(L.ERR_INVALID_ARG, f"elem {elem}", elem=elem)
        assert lib.gnx_core_backward_typed_workspace_bytes(c.g._h, C.byref(MC._core_params(gn, a, c.p, 1)), 1, elem) == 0
    for R in (0, -1, 65536):
        refuse(L.ERR_INVALID_ARG, f"R = {R}", R=R)
    for n in ("ef", "nf", "gf"):
        refuse(L.ERR_INVALID_ARG, f"{n} NULL", **{n: None})
    for attr in ("oe", "on", "og"):  # dims that are not dims => dims
        cp = MC._core_params(gn, a, c.p, 1)
        setattr(cp.block, attr, getattr(cp.block, attr) + 1)
        refuse(L.ERR_DIMS, f"{attr} + 1", cp=cp)
    assert call(a, ws_bytes=need) == 0, lib.gnx_last_error()  # and the same arena takes the call as it is
    a.check("the accepted call")
    # replicas need a batch of one graph
    c40 = _case("small40", (10, 5, 3), "relu")
    a, call = c40.arena(L.ELEM_BF16)
    a.build(ws_fill=WS_FILL)
    assert call(a, R=2) == L.ERR_INVALID_ARG, lib.gnx_last_error()
    _untouched(a, "R = 2 on 40 graphs")


MEM = [("small40", (10, 5, 3)), ("one", (64, 64, 64))]
MEM_IDS = ["small40-10x5x3", "one-64x64x64"]


@pytest.mark.parametrize("batch,dims", MEM, ids=MEM_IDS)
def test_memory_contract(gn, batch, dims):
    """every buffer at its exact size in one sentinel arena (every run above is checked this way too); here also: the outputs do not depend on
    what the workspace held"""
    L = gn._lib
    c = _case(batch, dims, "gelu")
    runs = [c.run(L.ELEM_BF16, ws_fill=fill) for fill in (0x00, 0xFF, WS_FILL)]
    for other in runs[1:]:
        for n in runs[0]:
            _same(other[n], runs[0][n], f"{c.what}: {n} depends on what the workspace held")


@pytest.mark.parametrize("skew", [4, 8, 12])
@pytest.mark.parametrize("batch,dims", MEM, ids=MEM_IDS)
def test_feature_buffers_at_4_byte_alignment(gn, batch, dims, skew):
    """all nine feature buffers at +4 / +8 / +12 bytes: status 0, a clean arena, and the bits of the fp32 entry on widened buffers at the SAME
    byte skew (both calls then take the one-wave-per-row LayerNorm kernels)"""
    _case(batch, dims, "gelu").check(f"features at +{skew}", skew=skew)


# ---- Python ----
def _py_batch(gn, seed, sizes, dims, dtype):
    rng = np.random.default_rng(seed)
    adjs = U.random_graphs(rng, sizes, 0.4)
    de, dn, dg = dims
    efs = [(rng.random((de, int((adj == 1).sum())), dtype=np.float32) * 2 - 1) for adj in adjs]
    nfs = [(rng.random((dn, adj.shape[0]), dtype=np.float32) * 2 - 1) for adj in adjs]
    gfs = [(rng.random((dg,), dtype=np.float32) * 2 - 1) for _ in adjs]
    return gn.batch(dict(graphs=adjs, ef=efs, nf=nfs, gf=gfs), dtype=dtype), rng


def test_python_autograd_matches_the_abi(gn):
    import torch
    lib, L = gn._lib.load(), gn._lib
    dims = (10, 5, 3)
    x, rng = _py_batch(gn, 21, (6, 9, 4, 1), dims, torch.bfloat16)
    core = U.core_from_params(gn, O.make_core_params(rng, dims))
    core.bf16 = True
    params = core.parameters()
    assert len(params) == 30
    for t in params:
        t.requires_grad_(True)
    ef, nf, gf = (t.detach().requires_grad_(True) for t in (x.ef, x.nf, x.gf))
    with pytest.raises(NotImplementedError, match="bf16_backward"):  # the default switches still raise
        core(gn.NT(x.graphs, ef, nf, gf))
    core.bf16_backward = True
    y = core(gn.NT(x.graphs, ef, nf, gf))
    assert all(t.dtype == torch.bfloat16 and t.requires_grad for t in (y.ef, y.nf, y.gf))
    node = y.ef.grad_fn
    while not hasattr(node, "saved_tensors"):  # (through the view that gives the Julia shape)
        node = node.next_functions[0][0]
    assert len(node.saved_tensors) == 3 and all(t.dtype == torch.bfloat16 for t in node.saved_tensors)
    # cotangents that are bf16 values: d(sum(y.float() * c)) / dy = c exactly
    cot = [torch.from_numpy(rng.standard_normal(tuple(t.shape)).astype(np.float32)).cuda().to(torch.bfloat16) for t in (y.ef, y.nf, y.gf)]
    sum((t.float() * c.float()).sum() for t, c in zip((y.ef, y.nf, y.gf), cot)).backward()
    assert all(t.grad.dtype == torch.bfloat16 and t.grad.shape == t.shape for t in (ef, nf, gf))
    assert all(t.grad is not None and t.grad.dtype == torch.float32 and t.grad.shape == t.shape for t in params)
    # the direct ABI call on the same (packed) tensors
    pk = lambda t: t.detach().permute(2, 1, 0).contiguous()
    g = x.graphs
    keep = []
    cp = core._c(keep)
    six = [pk(ef), pk(nf), pk(gf)] + [pk(c) for c in cot]
    d = [torch.empty_like(t) for t in six[:3]]
    gs = [torch.empty((q.shape[1], q.shape[0]), dtype=torch.float32, device="cuda").t() if q.dim() == 2 else torch.empty_like(q) for q in params]
    gr = gn.api._core_grads(core, gs)
    ws = torch.empty(int(lib.gnx_core_backward_typed_workspace_bytes(g._h, C.byref(cp), 1, L.ELEM_BF16)), dtype=torch.uint8, device="cuda")
    assert lib.gnx_core_backward_typed(g._h, C.byref(cp), L.ELEM_BF16, *(t.data_ptr() for t in six), 1, *(t.data_ptr() for t in d), C.byref(gr),
                                       ws.data_ptr(), ws.numel(), _stream()) == 0, lib.gnx_last_error()
    torch.cuda.synchronize()
    for name, t, w in zip(("ef", "nf", "gf"), (ef, nf, gf), d):
        _same(pk(t.grad), w, f"x.{name}.grad")
    for i, (t, w) in enumerate(zip(params, gs)):
        _same(t.grad.contiguous(), w.contiguous(), f"grad of parameter {i}")
    # a missing cotangent is passed as NULL: only y.nf enters the loss
    for t in [ef, nf, gf] + params:
        t.grad = None
    y = core(gn.NT(x.graphs, ef, nf, gf))
    (y.nf.float() * cot[1].float()).sum().backward()
    assert all(t.grad is not None and bool(torch.isfinite(t.grad.float()).all()) for t in (ef, nf, gf))


def _train(gn, steps=50):
    import torch
    dims = (10, 5, 3)
    x, rng = _py_batch(gn, 31, (5, 40, 17, 8, 33, 12), dims, torch.bfloat16)
    enc = U.block_from_params(gn, O.make_block_params(rng, dims, dims, act=(2, 2, 2)))
    core = U.core_from_params(gn, O.make_core_params(rng, dims))
    dec = U.block_from_params(gn, O.make_block_params(rng, dims, (3, 4, 5), act=(2, 2, 0)))
    enc.bf16_backward = dec.bf16_backward = core.bf16 = core.bf16_backward = True
    params = []
    for l in (enc.edgefn, enc.nodefn, enc.graphfn, dec.edgefn, dec.nodefn, dec.graphfn):
        params += [l.weight, l.bias]
    params += core.parameters()
    for t in params:
        t.requires_grad_(True)
    g = x.graphs
    target = [torch.from_numpy(rng.standard_normal((d, T, 1)).astype(np.float32)).cuda() for d, T in zip((3, 4, 5), (g.n_edges, g.n_nodes, g.n_graphs))]
    opt = torch.optim.AdamW(params, lr=1e-2)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        y = dec(core(enc(x)))
        loss = sum(((o.float() - t) ** 2).mean() for o, t in zip((y.ef, y.nf, y.gf), target))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def test_fifty_adamw_steps_reduce_the_loss_and_repeat_exactly(gn):
    a, b = _train(gn), _train(gn)
    assert all(np.isfinite(a))
    assert np.mean(a[-5:]) < np.mean(a[:5]), (a[:5], a[-5:])
    assert a == b  # the kernels are deterministic
