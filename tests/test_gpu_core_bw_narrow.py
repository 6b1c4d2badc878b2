"""gnx_core_backward_narrow on the GPU, through the ABI: the pullback of each FeedForward of a narrow GNCore in one kernel (k_core_bw_narrow).

The gradient w.r.t. gn2(x) is computed by the operations of the generic kernels in their order, so wherever the existing calls run their generic
kernels — every entity under 64 rows, every width with D . 4D < 64, or the whole process under GNX_BW_GENERIC — the three input gradients, the six
block gradients and the twelve LayerNorm gradients are compared bit for bit (BITS).  The twelve FeedForward gradients (FF) are the same sums in
another fixed order: they are held to the project's bound, max|got - ref| <= 1e-3 . max(1, max|ref|), against the existing call or against float64
autograd.  Every call runs inside one sentinel arena (tests/arena.py) with every buffer at its exact size.

Batches: "tiny" (3 graphs, every entity under 64 rows), "ragged" (5 graphs of 64, 65, 1, 127 and 300 edges: a full chunk, one over, a lone row, a
partial last chunk, several workgroups), "one" (one graph of 40 nodes and 150 edges, for replicas), "noedges" (E = 0)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from oracle import gn_oracle as O
from tests import arena as AR
from tests import test_gpu_memory_contract as MC  # the arena descriptors of a core (_decl_core, _core_params, _decl_dense_grad)
from tests import util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WS_FILL = 0xA5
BAR = 1e-3  # the project's bound on a gradient: max|got - ref| <= BAR . max(1, max|ref|)
DX = ("d_ef", "d_nf", "d_gf")
FEATURES = ("ef", "nf", "gf", "g_ef_out", "g_nf_out", "g_gf_out") + DX
CORE, TRAIN, TYPED, NARROW = "core", "train", "typed", "narrow"


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
FF = tuple(n for n in GRADS if n.startswith("grad.ff_"))  # the twelve FeedForward gradients: the bound
BITS = DX + tuple(n for n in GRADS if n not in FF)        # 3 + 6 + 12: bit for bit
LN1_AND_BLOCK = tuple(n for n in BITS if n not in DX and "ln2" not in n)  # what does not depend on dz2
assert len(GRADS) == 30 and len(FF) == 12 and len(BITS) == 21 and len(LN1_AND_BLOCK) == 12
RAGGED_EDGES = (64, 65, 1, 127, 300)


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
def graphs(name):
    import graphnets_jl_amd as gn
    if name == "noedges":
        g = gn.GNGraphBatch([np.zeros((n, n), dtype=np.int64) for n in (3, 5, 2)])
        assert g.n_edges == 0
        return g
    sizes, edges = {"tiny": ((4, 5, 3), (7, 11, 4)), "ragged": ((12, 12, 3, 15, 20), RAGGED_EDGES), "one": ((40,), (150,))}[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))

    def csc_of(n, e):  # exactly e distinct directed pairs of an n-node graph, sorted by destination then source (tests/util.py: er_csc)
        k = np.sort(rng.choice(n * n, e, replace=False))
        colptr = np.zeros(n + 1, dtype=np.int64)
        np.add.at(colptr, k // n + 1, 1)
        return np.cumsum(colptr), (k % n).astype(np.int64)

    csc = [csc_of(n, e) for n, e in zip(sizes, edges)]
    g = gn.GNGraphBatch.from_csc([c[0] for c in csc], [c[1] for c in csc], list(sizes))
    assert g.n_edges == sum(edges) and g.n_nodes == sum(sizes) and g.n_graphs == len(sizes)
    if name == "tiny":
        assert max(g.n_edges, g.n_nodes, g.n_graphs) < 64
    return g


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _seed(*key):
    return zlib.crc32(repr(key).encode())  # (the same in every process, unlike hash())


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same(a, b, what):
    import torch
    assert a.dtype == b.dtype and a.shape == b.shape, what
    x, y = _bits(a), _bits(b)
    if not torch.equal(x, y):
        bad = (x != y).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {x.numel()} values differ, first at {i}: {a[i].item()!r} vs {b[i].item()!r}")


def close(got, ref, what):
    """the project's bound (tests/test_gpu_backward.py's `close`); prints the figure before it asserts"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.size == 0:
        return
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    print(f"BOUND {what}: max err {err:.3e}, bar {BAR * scale:.3e}")
    assert np.isfinite(got).all() and err <= BAR * scale, f"{what}: max err {err:.3e} (scale {scale:.3g})"


def compare(got, ref, what, names=None):
    """BITS bit for bit, FF within the bound — over the outputs both runs have (`names`: only these)"""
    assert set(got) == set(ref), (what, sorted(set(got) ^ set(ref)))
    for n in sorted(got):
        if names is not None and n not in names:
            continue
        if n in FF:
            close(got[n].float().cpu().numpy(), ref[n].float().cpu().numpy(), f"{what} {n}")
        else:
            same(got[n], ref[n], f"{what} {n}")
    return set(got)


class Case:
    """A core's parameters, its three inputs and three random cotangents (fp32 values; `bf16`: values that are bf16 values)."""

    def __init__(self, gn, batch, R, dims, act, seed, bf16=False, kinkfree=False):
        import torch
        self.gn, self.dims, self.act, self.R, self.what = gn, dims, act, R, f"{batch} R={R} {dims} {act}"
        self.g = graphs(batch)
        rng = np.random.default_rng(seed)
        self.p = O.make_core_params(rng, dims)
        self.rows = (self.g.n_edges, self.g.n_nodes, self.g.n_graphs)
        if kinkfree:  # fp32 in [0, 1) without a hidden pre-activation near the relu kink (tests/util.py)
            xs, self.rounds, _ = U.kinkfree_core_inputs(rng, self.p, R, *self.rows)
            self.x = [torch.from_numpy(a) for a in xs]
        else:  # values of both signs over a few binades
            self.x = [torch.from_numpy((a * 4 - 2).astype(np.float32)) for a in U.packed_inputs(rng, R, *self.rows, dims)]
        self.cots = [torch.from_numpy(rng.standard_normal(tuple(t.shape)).astype(np.float32)) for t in self.x]
        if bf16:
            self.x = [t.to(torch.bfloat16).float() for t in self.x]
            self.cots = [t.to(torch.bfloat16).float() for t in self.cots]

    def cp(self, a):
        return MC._core_params(self.gn, a, self.p, self.gn._lib.ACT[self.act])

    def arena(self, entry, elem=None, cots=(True,) * 3, drop=()):
        """the arena of one call: (arena, call) — call(a, dropout=None, grads_null=False, **overrides) -> status"""
        import torch
        gn, g, R, p = self.gn, self.g, self.R, self.p
        L, lib = gn._lib, gn._lib.load()
        elem = L.ELEM_F32 if elem is None else elem
        bf = elem == L.ELEM_BF16
        assert not bf or entry in (TYPED, NARROW)
        dt = torch.bfloat16 if bf else torch.float32
        a = AR.Arena("cuda")
        MC._decl_core(a, p)
        ins = [a.input(n, t.to(dt)) for n, t in zip(("ef", "nf", "gf"), self.x)]
        gs = [a.input(n, t.to(dt)) if keep else None for n, t, keep in zip(("g_ef_out", "g_nf_out", "g_gf_out"), self.cots, cots)]
        dx = [a.output(n, t.shape, dt) for n, t in zip(DX, self.x)]
        pb = p["block"]
        for fn, w, b in (("edgefn", "We", "be"), ("nodefn", "Wn", "bn"), ("graphfn", "Wg", "bg")):
            MC._decl_dense_grad(a, f"grad.{fn}", pb[w], pb[b])
        for t in "eng":
            for ln in ("ln1", "ln2"):
                a.output(f"grad.{ln}_{t}.gamma", p[f"{ln}_{t}_gamma"].shape)
                a.output(f"grad.{ln}_{t}.beta", p[f"{ln}_{t}_beta"].shape)
            MC._decl_dense_grad(a, f"grad.ff_{t}.fc1", p[f"ff_{t}_W1"], p[f"ff_{t}_b1"])
            MC._decl_dense_grad(a, f"grad.ff_{t}.fc2", p[f"ff_{t}_W2"], p[f"ff_{t}_b2"])

        def query():
            cp = self.cp(a)
            if entry == NARROW:
                n = int(lib.gnx_core_backward_narrow_workspace_bytes(g._h, C.byref(cp), R, elem))
            elif entry == TYPED:
                n = int(lib.gnx_core_backward_typed_workspace_bytes(g._h, C.byref(cp), R, elem))
            else:
                n = int(lib.gnx_core_backward_workspace_bytes(g._h, C.byref(cp), R))
            assert n > 0, lib.gnx_last_error()
            return n

        ws = a.workspace("ws", query)

        def call(a, dropout=None, grads_null=False, **over):
            G = lambda n: None if n in drop else a.ptr(n)
            gr = L.CoreGrads()
            gr.block = L.BlockGrads(*[L.DenseGrad(G(f"grad.{fn}.dW"), G(f"grad.{fn}.db")) for fn in ("edgefn", "nodefn", "graphfn")])
            for i, t in enumerate("eng"):
                gr.ln1[i].gamma, gr.ln1[i].beta = G(f"grad.ln1_{t}.gamma"), G(f"grad.ln1_{t}.beta")
                gr.ln2[i].gamma, gr.ln2[i].beta = G(f"grad.ln2_{t}.gamma"), G(f"grad.ln2_{t}.beta")
                gr.ff[i].fc1 = L.DenseGrad(G(f"grad.ff_{t}.fc1.dW"), G(f"grad.ff_{t}.fc1.db"))
                gr.ff[i].fc2 = L.DenseGrad(G(f"grad.ff_{t}.fc2.dW"), G(f"grad.ff_{t}.fc2.db"))
            cp = self.cp(a)
            six = (*map(a.ptr, ins), *map(a.ptr, gs))
            tail = (R, *map(a.ptr, dx), None if grads_null else C.byref(gr), a.ptr(ws), a.nbytes(ws), _stream())
            dp = None if dropout is None else C.byref(dropout)
            if entry == NARROW:
                rc = lib.gnx_core_backward_narrow(g._h, C.byref(cp), over.get("elem", elem), dp, *six, *tail)
            elif entry == TYPED:
                rc = lib.gnx_core_backward_typed(g._h, C.byref(cp), elem, *six, *tail)
            elif entry == TRAIN:
                rc = lib.gnx_core_backward_train(g._h, C.byref(cp), dp, *six, *tail)
            else:
                rc = lib.gnx_core_backward(g._h, C.byref(cp), *six, *tail)
            torch.cuda.synchronize()
            return rc

        return a, call

    def run(self, entry, elem=None, ws_fill=WS_FILL, dropout=None, grads_null=False, cots=(True,) * 3, drop=(), profile=None, twice=False):
        """one call inside its arena: {name: a copy of the output tensor}; outputs passed as NULL are absent (and were not written)"""
        a, call = self.arena(entry, elem, cots, drop)
        a.build(ws_fill=ws_fill)
        what = f"{self.what} {entry} elem={elem} cots={cots} drop={drop}"
        if profile is not None:
            self.gn.profile_reset(); self.gn.profile_enable(True)
        try:
            assert call(a, dropout, grads_null) == 0, f"{what}: {self.gn._lib.load().gnx_last_error()}"
        finally:
            if profile is not None:
                self.gn.profile_enable(False)
                profile.update(self.gn.profile_read()); self.gn.profile_reset()
        skip = set(drop) | (set(GRADS) if grads_null else set())

        def collect():
            for n in skip:  # an output passed as NULL: its carve must still hold the bytes it was given
                assert bool((a.raw(n) == AR.UNWRITTEN).all()), f"{what}: {n} was written although NULL was passed"
                a.raw(n)[:] = 0
            a.check(what)
            return {c.name: a.view(c.name).clone() for c in a.carves if c.kind == AR.OUTPUT and c.name not in skip}

        out = collect()
        if twice:  # a second call into the same arena (the workspace now holds what the first left): the same bits
            a.refill(0x3C)
            assert call(a, dropout, grads_null) == 0
            again = collect()
            for n in out:
                same(again[n], out[n], f"{what}: {n} differs on the second call")
        self.ws_bytes = a.nbytes("ws")
        return out

    def applies(self, elem=None):
        L, lib = self.gn._lib, self.gn._lib.load()
        a = AR.Arena("cuda")
        MC._decl_core(a, self.p)
        a.build()
        return int(lib.gnx_core_backward_narrow_applies(self.g._h, C.byref(self.cp(a)), self.R, L.ELEM_F32 if elem is None else elem))


@functools.lru_cache(maxsize=None)
def case(batch, R, dims, act, bf16=False, kinkfree=False):
    import graphnets_jl_amd as gn
    return Case(gn, batch, R, dims, act, _seed(batch, R, dims, act), bf16, kinkfree)


# ---- 1. bits, in process: the existing call is generic there without any environment variable ----
TINY_DIMS = [(10, 5, 3), (16, 1, 7), (16, 16, 16)]  # and (1, 1, 1): in a process of its own, below
SMALL_DIMS = [(3, 3, 3), (2, 3, 1), (1, 2, 3)]  # every D . 4D < 64
IN_PROCESS = [("tiny", 1, d) for d in TINY_DIMS] + [("ragged", 1, d) for d in SMALL_DIMS] + [("one", R, d) for R in (1, 2, 3) for d in SMALL_DIMS]
IDS = lambda cs: [f"{b}-R{R}-{'x'.join(map(str, d))}" for b, R, d in cs]


@pytest.mark.parametrize("act", ["relu", "identity"])
@pytest.mark.parametrize("batch,R,dims", IN_PROCESS, ids=IDS(IN_PROCESS))
def test_bits_equal_gnx_core_backward(gn, batch, R, dims, act):
    c = case(batch, R, dims, act)
    assert c.applies() == 1
    seen = {}
    ref, got = c.run(CORE), c.run(NARROW, profile=seen)
    assert compare(got, ref, c.what) == set(DX) | set(GRADS)
    assert "bw_delta" in seen and "bw_fw_dense_generic" not in seen, sorted(seen)


def _child(mode, env):
    r = subprocess.run([sys.executable, "-m", "tests.core_bw_narrow_child", mode], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"child {mode}: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bits_equal_gnx_core_backward_at_width_one(gn):
    """"tiny" at (1,1,1), relu and identity, the comparison of the test above in the default environment — in a child process: a core at
    (1,1,1) specialises the block's forward kernel for (1,1,1) => (1,1,1) at run time, once per process, and tests/test_gpu_jit.py counts that
    compilation in the process of the suite."""
    env = {k: v for k, v in os.environ.items() if k != "GNX_BW_GENERIC"}
    out = _child("width_one", env)
    assert out == dict(cases=2, applies=[1, 1], fused=True), out


# ---- 2. bits at real sizes: one child process under GNX_BW_GENERIC (read once per process) ----
CHILD_DIMS = [(10, 5, 3), (16, 16, 16), (7, 4, 9)]
CHILD_CASES = [("ragged", 1), ("one", 2)]


def test_bits_at_real_widths_in_a_generic_child(gn):
    out = _child("generic", dict(os.environ, GNX_BW_GENERIC="1"))
    assert out["cases"] == len(CHILD_DIMS) * len(CHILD_CASES) * 2 and out["generic"] is True, out


# ---- 3. float64 anchor, default environment ----
ANCHOR_DIMS = [(10, 5, 3), (16, 16, 16), (5, 16, 2)]


@pytest.mark.parametrize("dims", ANCHOR_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_every_gradient_against_float64_autograd(gn, dims):
    """torch float64 autograd of the restatement of tests/test_gpu_backward.py::_core_backward_case (tests/test_gpu_memory_contract.py's _torch_core is
    that restatement; tests/test_gpu_backward_replicas.py's _core_reference differentiates it in the layout of the ABI)"""
    import torch
    from tests import test_gpu_backward_replicas as BR
    c = case("ragged", 1, dims, "relu", kinkfree=True)
    assert c.rounds <= 20
    xs = [t.numpy() for t in c.x]
    for t, v in zip("eng", xs):
        assert not U.relu_kink_rows(c.p, t, v).any(), (dims, t)
    g = c.g
    ref = BR._core_reference(c.p, (*g.csc(), g.node_off, g.edge_off), xs, [t.numpy() for t in c.cots], "relu", None, torch.float64)
    assert c.applies() == 1
    got = c.run(NARROW)
    assert set(got) == set(ref) == set(DX) | set(GRADS)
    for n in sorted(got):
        close(got[n].cpu().numpy(), ref[n], f"{c.what} {n}")
    old = c.run(CORE)
    for n in LN1_AND_BLOCK:  # they do not depend on dz2
        same(got[n], old[n], f"{c.what} {n}")


# ---- 4. optional arguments ----
@pytest.mark.parametrize("batch,dims", [("ragged", (2, 3, 1)), ("tiny", (10, 5, 3))], ids=["ragged-2x3x1", "tiny-10x5x3"])
def test_optional_arguments(gn, batch, dims):
    c = case(batch, 1, dims, "relu")
    both = lambda what, **kw: compare(c.run(NARROW, **kw), c.run(CORE, **kw), f"{c.what} {what}")
    for k in range(3):
        assert both(f"cotangent {k} NULL", cots=tuple(i != k for i in range(3))) == set(DX) | set(GRADS)
    assert both("grads NULL", grads_null=True) == set(DX)
    for t in "eng":
        for fc in ("fc1", "fc2"):
            for part in ("dW", "db"):  # weight without bias and bias without weight, per Dense
                got = both(f"NULL grad.ff_{t}.{fc}.{part}", drop=(f"grad.ff_{t}.{fc}.{part}",))
                assert len(got) == 32
    both("no FeedForward gradient at all", drop=FF)


@pytest.mark.parametrize("dims", [(10, 5, 3), (2, 3, 1)], ids=lambda d: "x".join(map(str, d)))
def test_a_batch_without_edges(gn, dims):
    c = case("noedges", 1, dims, "relu")
    assert c.applies() == 1
    got = c.run(NARROW)
    compare(got, c.run(CORE), c.what)
    for n in ("grad.ff_e.fc1.dW", "grad.ff_e.fc1.db", "grad.ff_e.fc2.dW", "grad.ff_e.fc2.db"):
        assert bool((got[n] == 0).all()), n  # sums over nothing


# ---- 5. dropout, fp32 ----
def test_dropout(gn):
    import torch
    L, lib = gn._lib, gn._lib.load()
    c = case("tiny", 1, (10, 5, 3), "relu")
    drop = L.Dropout(0.3, 0, 0xC0FFEE)
    ref, got = c.run(TRAIN, dropout=drop), c.run(NARROW, dropout=drop)
    compare(got, ref, f"{c.what} p=0.3")
    plain = c.run(NARROW)
    assert not torch.equal(_bits(plain["d_ef"]), _bits(got["d_ef"]))  # the mask took part
    zero = c.run(NARROW, dropout=L.Dropout(0.0, 0, 0xC0FFEE))
    for n in plain:  # p = 0 and dropout = NULL are the same call
        same(zero[n], plain[n], f"{c.what} p=0 {n}")
    # bfloat16 with an active dropout: refused, nothing written
    cb = case("tiny", 1, (10, 5, 3), "relu", bf16=True)
    a, call = cb.arena(NARROW, L.ELEM_BF16)
    a.build(ws_fill=WS_FILL)
    assert call(a, dropout=drop) == L.ERR_INVALID_ARG and b"bf16" in lib.gnx_last_error()
    a.check("bf16 with dropout", unwritten=False)
    for cv in a.carves:
        if cv.nbytes and cv.kind == AR.OUTPUT:
            assert bool((a.raw(cv.name) == AR.UNWRITTEN).all()), cv.name
        elif cv.nbytes and cv.kind == AR.WORKSPACE:
            assert bool((a.raw(cv.name) == WS_FILL).all()), cv.name
    assert call(a, dropout=L.Dropout(0.0, 0, 1)) == 0, lib.gnx_last_error()  # (p = 0: test mode, accepted)


# ---- 6. bf16 ----
@pytest.mark.parametrize("dims", [(10, 5, 3)] + SMALL_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_bf16_equals_the_typed_call(gn, dims):
    L = gn._lib
    c = case("tiny", 1, dims, "relu", bf16=True)
    assert c.applies(L.ELEM_BF16) == 1
    assert compare(c.run(NARROW, L.ELEM_BF16), c.run(TYPED, L.ELEM_BF16), f"{c.what} bf16") == set(DX) | set(GRADS)
    f32 = c.run(NARROW, L.ELEM_F32)  # GNX_ELEM_F32 through the new entry: the fp32 result
    ref = c.run(NARROW)
    for n in ref:
        same(f32[n], ref[n], f"{c.what} f32 {n}")
    compare(f32, c.run(CORE), f"{c.what} f32")


# ---- 7. fallback ----
@pytest.mark.parametrize("dims,act", [((20, 5, 3), "relu"), ((10, 5, 3), "tanh"), ((10, 5, 3), "gelu")], ids=["20x5x3", "tanh", "gelu"])
def test_where_it_does_not_apply_it_is_the_typed_call(gn, dims, act):
    L = gn._lib
    for bf16 in (False, True):
        elem = L.ELEM_BF16 if bf16 else L.ELEM_F32
        c = case("ragged", 1, dims, act, bf16=bf16)
        assert c.applies(elem) == 0
        seen = {}
        got = c.run(NARROW, elem, profile=seen)
        n_bytes = c.ws_bytes
        ref = c.run(TYPED, elem)
        assert n_bytes == c.ws_bytes
        assert set(got) == set(ref) == set(DX) | set(GRADS)
        for n in got:
            same(got[n], ref[n], f"{c.what} bf16={bf16} {n}")
        assert "bw_fw_dense_generic" in seen or "bw_ff1_recompute" in seen, sorted(seen)
    c = case("ragged", 1, dims, act)
    drop = L.Dropout(0.3, 0, 11)
    got, ref = c.run(NARROW, dropout=drop), c.run(TRAIN, dropout=drop)
    for n in got:
        same(got[n], ref[n], f"{c.what} p=0.3 {n}")


# ---- 8. memory contract ----
@pytest.mark.parametrize("batch,R,dims", [("ragged", 1, (10, 5, 3)), ("one", 3, (16, 16, 16))], ids=["ragged-10x5x3", "one-R3-16x16x16"])
def test_memory_contract(gn, batch, R, dims):
    """buffers at their exact sizes and the workspace exactly the query's (every run's arena); nothing outside outputs and workspace written, inputs
    untouched (arena.check in every run); results do not depend on what the workspace held, and repeat on a second call"""
    lib = gn._lib.load()
    c = case(batch, R, dims, "relu")
    seen = {}
    runs = [c.run(NARROW, ws_fill=0x00, profile=seen, twice=True), c.run(NARROW, ws_fill=0xFF)]
    for n in runs[0]:
        same(runs[1][n], runs[0][n], f"{c.what}: {n} depends on what the workspace held")
    assert "bw_delta" in seen and "bw_dw_generic" in seen, sorted(seen)
    assert seen["bw_delta"]["launches"] >= 3 and seen["bw_dw_generic"]["launches"] >= 6, seen
    assert not {"bw_ff1_recompute", "bw_dx_ff2", "bw_dx_ff1", "bw_fw_dense_generic"} & set(seen), sorted(seen)
    narrow_bytes = c.ws_bytes
    a = AR.Arena("cuda")
    MC._decl_core(a, c.p)
    a.build()
    assert narrow_bytes < int(lib.gnx_core_backward_workspace_bytes(c.g._h, C.byref(c.cp(a)), R))


# ---- 9. Python ----
def _py_setup(gn, bf16):
    import torch
    dims = (10, 5, 3)
    g = graphs("ragged")
    rng = np.random.default_rng(77)
    core = U.core_from_params(gn, O.make_core_params(rng, dims))
    ef, nf, gf = (torch.from_numpy((a * 4 - 2).astype(np.float32)).cuda() for a in U.packed_inputs(rng, 1, g.n_edges, g.n_nodes, g.n_graphs, dims))
    if bf16:
        ef, nf, gf = (t.to(torch.bfloat16) for t in (ef, nf, gf))
        core.bf16 = core.bf16_backward = True
    return g, rng, core, (ef, nf, gf)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_python_autograd_matches_the_abi(gn, bf16):
    import torch
    lib, L = gn._lib.load(), gn._lib
    g, rng, core, packed = _py_setup(gn, bf16)
    elem = L.ELEM_BF16 if bf16 else L.ELEM_F32
    assert core.narrow_backward is False
    core.narrow_backward = True
    params = core.parameters()
    for t in params:
        t.requires_grad_(True)
    ef, nf, gf = (t.permute(2, 1, 0).detach().requires_grad_(True) for t in packed)
    y = core(gn.NT(g, ef, nf, gf))
    cot = [torch.from_numpy(rng.standard_normal(tuple(t.shape)).astype(np.float32)).cuda().to(t.dtype) for t in (y.ef, y.nf, y.gf)]
    gn.profile_reset(); gn.profile_enable(True)
    try:
        sum((t.float() * c.float()).sum() for t, c in zip((y.ef, y.nf, y.gf), cot)).backward()
        torch.cuda.synchronize()
    finally:
        gn.profile_enable(False)
    seen = gn.profile_read(); gn.profile_reset()
    assert "bw_delta" in seen and "bw_fw_dense_generic" not in seen and "bw_ff1_recompute" not in seen, sorted(seen)
    pk = lambda t: t.detach().permute(2, 1, 0).contiguous()
    keep = []
    cp = core._c(keep)
    assert lib.gnx_core_backward_narrow_applies(g._h, C.byref(cp), 1, elem) == 1
    six = [pk(ef), pk(nf), pk(gf)] + [pk(c) for c in cot]
    d = [torch.empty_like(t) for t in six[:3]]
    gs = [torch.empty((q.shape[1], q.shape[0]), dtype=torch.float32, device="cuda").t() if q.dim() == 2 else torch.empty_like(q) for q in params]
    gr = gn.api._core_grads(core, gs)
    ws = torch.empty(int(lib.gnx_core_backward_narrow_workspace_bytes(g._h, C.byref(cp), 1, elem)), dtype=torch.uint8, device="cuda")
    assert lib.gnx_core_backward_narrow(g._h, C.byref(cp), elem, None, *(t.data_ptr() for t in six), 1, *(t.data_ptr() for t in d), C.byref(gr), ws.data_ptr(),
                                        ws.numel(), _stream()) == 0, lib.gnx_last_error()
    torch.cuda.synchronize()
    for name, t, w in zip(("ef", "nf", "gf"), (ef, nf, gf), d):
        same(pk(t.grad), w, f"x.{name}.grad")
    for i, (t, w) in enumerate(zip(params, gs)):
        same(t.grad.contiguous(), w.contiguous(), f"grad of parameter {i}")


def _train(gn, bf16, steps=20):
    import torch
    g, rng, core, packed = _py_setup(gn, bf16)
    core.narrow_backward = True
    params = core.parameters()
    for t in params:
        t.requires_grad_(True)
    x = gn.NT(g, *(t.permute(2, 1, 0) for t in packed))
    target = [torch.from_numpy(rng.standard_normal((d, T, 1)).astype(np.float32)).cuda() for d, T in zip((10, 5, 3), (g.n_edges, g.n_nodes, g.n_graphs))]
    opt = torch.optim.AdamW(params, lr=1e-2)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        y = core(x)
        loss = sum(((o.float() - t) ** 2).mean() for o, t in zip((y.ef, y.nf, y.gf), target))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_twenty_adamw_steps_reduce_the_loss_and_repeat_exactly(gn, bf16):
    a, b = _train(gn, bf16), _train(gn, bf16)
    assert all(np.isfinite(a))
    assert np.mean(a[-3:]) < np.mean(a[:3]), (a[:3], a[-3:])
    assert a == b  # the kernels are deterministic
