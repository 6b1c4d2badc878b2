"""gnx_chain_block_backward_narrow: the pullback of a GNBlock whose update functions are Chains with every update function inside the rule in ONE
kernel (csrc/gnx_chain_bw_narrow.hip) — against float64 torch autograd through the Python switch, against the generic entry through the ABI
(max|narrow - ref| <= max(4 max|generic - ref|, 1e-5 max(1, max|ref|)) per gradient tensor: a NORMWISE bound whose yardstick is the generic
entry's own error — it does not have the margin of tests/test_gpu_bw_x6_stress.py, whose factor 4 is on a mean error against a float32 evaluation;
the elementwise bar |got - ref| <= 1e-5 . S against the float64 pullback oracle, for both entries, is tests/test_gpu_chain_bw_stress.py's),
structural batches, what happens outside the rule, the launch structure, the
memory contract on exactly sized 4-byte-aligned buffers, stream capture, the Python switch and a seeded sweep.  Small batches throughout: five
graphs of 3..40 nodes."""
import ctypes as C
import gc
import json
import os

import numpy as np
import pytest

from oracle import gn_oracle as O
from tests import arena as AR
from tests import util as U
from tests import test_gpu_chain as TC
from tests import test_gpu_chain_narrow as CN
from tests.test_chain_bw_narrow_abi import formula_takes
from tests.test_gpu_memory_contract import _chain_params, _decl, _decl_chains, _decl_dense_grad, _dense_grad

pytestmark = pytest.mark.gpu
EXTRA = int(os.environ.get("GNX_FUZZ_EXTRA", "0"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_CASES = [
    ((10, 5, 0), [16, 3], [8, 4], [6, 5], (1, 2, 0)),
    ((2, 2, 1), [8, 8, 1], [3], [2], None),
    ((3, 2, 1), [9, 17, 4], [16, "ln", 5], ["ln", 9, 4, "ln"], (4, 3, 1)),
    ((8, 8, 8), [32, 32, 7], [32, 9], [32, "ln", 4], (1, 2, 0)),
    ((0, 4, 2), [8, 5], [5], [], None),
    ((6, 0, 0), [4, 3], [], [], None),
    ((10, 5, 3), ["ln", 12, 7], [6, "ln"], [4], None),
    ((3, 2, 1), [8] * 8, [8, 8, 8], [8, 8], None),
]
ANY_MASK_CASE = ((8, 8, 8), [32, "ln", 32, 32, 7], ["ln", 32, 32, 9], [32, "ln", 17, 4], (1, 2, 0))


@pytest.fixture(scope="module")
def gn():
    import torch
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


def _want_mask(case, g):
    """the mask the formula of include/gnx.h gives (tests/test_chain_bw_narrow_abi.py restates it).  Every case had the full mask while one wave's
    LDS was the budget; after the measurement the one-wave class is cut from the rule, and the functions of these cases that need more than
    half of the LDS per wave — the 32-wide chains of the fourth case — run the generic launches: a mixed call, checked in the same way."""
    (de, dn, dg), chains = case[0], case[1:4]
    k_in, mask, outs = de + 2 * dn + dg, 0, []
    for t, ws in enumerate(chains):
        if t == 1:
            k_in = outs[0] + dn + dg
        elif t == 2:
            k_in = outs[0] + outs[1] + dg
        widths, ln, k = [], [], k_in
        for w in ws:
            if w == "ln":
                ln.append(len(widths))
                widths.append(k)
            else:
                k = w
                widths.append(w)
        outs.append(k if ws else 0)
        rows = (g.n_edges, g.n_nodes, g.n_graphs)[t]
        if ws and formula_takes(k_in, widths, tuple(ln), rows):
            mask |= 1 << t
    return mask


class BwCall(CN.Call):
    """one block on one batch: the inputs, cotangents, the float64 gradients of tests.test_gpu_chain._torch_chain_block (summed over the replicas
    for the parameters), and either backward entry through the ABI on a workspace of exactly the queried size"""

    def __init__(self, gn, adjs, p, R=1, seed=0):
        super().__init__(gn, adjs, p, R, seed)
        import torch
        self.ok = True
        rng = np.random.default_rng(12000 + seed)
        csc = (*self.g.csc(), self.g.node_off, self.g.edge_off)
        T = lambda v: torch.tensor(v, dtype=torch.float64, requires_grad=True)
        W = {name: [(w, T(b), T(c)) if isinstance(w, str) else (T(w), T(b), c) for w, b, c in p[name]] for name in ("edge", "node", "graph")}
        dx = [None if v is None else np.zeros(v.shape) for v in self.x]
        cots = [[], [], []]
        for r in range(R):
            xs = [None if v is None else T(v[r]) for v in self.x]
            outs, pre = TC._torch_chain_block(csc, *xs, W)
            if any(a == 1 and float(z.detach().abs().min()) < 5e-6 for z, a in pre if z.numel()):
                self.ok = False  # a relu pre-activation within fp32 rounding of its kink: re-draw
                return
            cot = [None if o is None else rng.standard_normal(tuple(o.shape)) for o in outs]
            sum((o * torch.from_numpy(c)).sum() for o, c in zip(outs, cot) if o is not None).backward()
            for t in range(3):
                if xs[t] is not None:
                    dx[t][r] = xs[t].grad.numpy() if xs[t].grad is not None else 0.0
                if cot[t] is not None:
                    cots[t].append(cot[t].astype(np.float32))
        self.cot = [torch.from_numpy(np.stack(c)).to(self.g.device) if c else None for c in cots]
        self.ref = {n: v for n, v in zip(("d_ef", "d_nf", "d_gf"), dx) if v is not None}
        zero = lambda q: np.zeros(tuple(q.shape)) if q.grad is None else q.grad.numpy()
        for name in ("edge", "node", "graph"):
            for i, (w, b, c) in enumerate(W[name]):
                if isinstance(w, str):
                    self.ref[f"{name}{i}.dW"], self.ref[f"{name}{i}.db"] = zero(b), zero(c)
                else:
                    self.ref[f"{name}{i}.dW"], self.ref[f"{name}{i}.db"] = zero(w).T, zero(b)

    def mask(self):
        return self.lib.gnx_chain_block_backward_narrow_applies(self.g._h, C.byref(self.cp), self.R)

    def query(self, narrow=True):
        q = self.lib.gnx_chain_block_backward_narrow_workspace_bytes if narrow else self.lib.gnx_chain_block_backward_workspace_bytes
        return q(self.g._h, C.byref(self.cp), self.R)

    def grads(self, skip=()):
        """NaN-filled gradient tensors by name (those in `skip` are not wanted: NULL)"""
        import torch
        out = {}
        for n, t in zip(("d_ef", "d_nf", "d_gf"), self.xt):
            if t is not None and n not in skip:
                out[n] = torch.full_like(t, float("nan"))
        for n, r in self.ref.items():
            if "." in n and n not in skip:
                out[n] = torch.full(r.shape, float("nan"), dtype=torch.float32, device=self.g.device)
        return out

    def run(self, narrow=True, outs=None, ws=None, fill=0xA5, stream=None, skip=(), nbytes=None):
        import torch
        L = self.L
        nbytes = self.query(narrow) if nbytes is None else nbytes  # (inside a capture the caller passes the size: the query belongs outside)
        assert nbytes > 0, self.lib.gnx_last_error()
        if ws is None:
            ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=self.g.device)
        outs = self.grads(skip) if outs is None else outs
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        arrays = []
        for name in ("edge", "node", "graph"):
            arr = (L.DenseGrad * max(len(self.p[name]), 1))()
            for i in range(len(self.p[name])):
                arr[i] = L.DenseGrad(ptr(outs.get(f"{name}{i}.dW")), ptr(outs.get(f"{name}{i}.db")))
            arrays.append(arr)
        gr = L.ChainBlockGrads(*[C.cast(a, C.POINTER(L.DenseGrad)) for a in arrays])
        entry = self.lib.gnx_chain_block_backward_narrow if narrow else self.lib.gnx_chain_block_backward
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        xin = [None if t is None else t.data_ptr() for t in self.xt]
        rc = entry(self.g._h, C.byref(self.cp), *xin, *[None if c is None else c.data_ptr() for c in self.cot], self.R,
                   *[None if outs.get(n) is None else outs[n].data_ptr() for n in ("d_ef", "d_nf", "d_gf")], C.byref(gr), ws.data_ptr(), nbytes, s)
        assert rc == 0, self.lib.gnx_last_error()
        return outs

    def check(self, what, narrow_outs=None, only=None):
        """the item-2 check of every gradient tensor (or those `only` selects); returns the worst ratio to the bound"""
        import torch
        a = self.run(True) if narrow_outs is None else narrow_outs
        b = self.run(False)
        torch.cuda.synchronize()
        worst = 0.0
        for n, r in self.ref.items():
            if n not in a or r.size == 0 or (only is not None and not only(n)):
                continue
            en = float(np.max(np.abs(a[n].cpu().numpy().astype(np.float64) - r)))
            eg = float(np.max(np.abs(b[n].cpu().numpy().astype(np.float64) - r)))
            bound = max(4.0 * eg, 1e-5 * max(1.0, float(np.abs(r).max())))
            worst = max(worst, en / bound)
            assert np.isfinite(en) and en <= bound, f"{what} {n}: narrow err {en:.3e}, generic err {eg:.3e}, bound {bound:.3e}"
        print(f"chain bw narrow {what}: worst narrow err / bound = {worst:.3e}")
        return worst


def make(gn, adjs, case, R=1, seed=0):
    """a kink-free draw of the case's parameters and inputs on the batch"""
    for attempt in range(20):
        c = BwCall(gn, adjs, CN._params(np.random.default_rng(13000 + 101 * seed + 1000 * attempt), case), R, seed + 1000 * attempt)
        if c.ok:
            return c
    pytest.fail("no kink-free draw in 20 attempts")


def _switched(monkeypatch, made, narrow_chain):
    plain = TC._block

    def switched(gn_, p):
        blk = plain(gn_, p)
        blk.narrow_chain_backward = True
        blk.narrow_chain = narrow_chain
        made.append(blk)
        return blk

    monkeypatch.setattr(TC, "_block", switched)


def _er_batch(gn, rng):
    sizes = rng.integers(3, 30, 5)
    cs = [U.er_csc(rng, int(n), int(0.2 * n * n) + 1) for n in sizes]
    return gn.GNGraphBatch.from_csc([c[0] for c in cs], [c[1] for c in cs], [int(n) for n in sizes])


# ---- 1. against float64 autograd, through the switch ----
@pytest.mark.parametrize("narrow_chain", (False, True), ids=("forward-generic", "forward-narrow"))
@pytest.mark.parametrize("i", range(len(FULL_CASES) + 1), ids=[str(c[:4]) for c in FULL_CASES] + ["any-mask"])
def test_against_float64_autograd(gn, monkeypatch, i, narrow_chain):
    made = []
    _switched(monkeypatch, made, narrow_chain)
    case = FULL_CASES[i] if i < len(FULL_CASES) else ANY_MASK_CASE
    in_dims, ew, nw, gw, acts = case
    acts = (1, 2, 0) if acts is None else acts  # (the oracle's default)
    lib = gn._lib.load()
    for attempt in range(20):
        rng = np.random.default_rng(800 + i + 1000 * attempt)
        g = _er_batch(gn, rng)
        if i < len(FULL_CASES):
            keep = []
            cp = TC._block(gn, O.make_chain_block_params(np.random.default_rng(0), in_dims, ew, nw, gw, acts=acts))._chain_params(keep)[0]
            assert lib.gnx_chain_block_backward_narrow_applies(g._h, C.byref(cp), 1) == _want_mask(case, g), case
            made.clear()
        if TC.chain_block_backward_case(gn, g, rng, in_dims, ew, nw, gw, acts):
            assert len(made) == 1 and made[0].narrow_chain_backward is True and made[0].narrow_chain is narrow_chain
            return
        made.clear()
    pytest.fail("no kink-free draw in 20 attempts")


# ---- 2. against the generic entry, through the ABI ----
@pytest.mark.parametrize("i", range(len(FULL_CASES) + 1), ids=[str(c[:4]) for c in FULL_CASES] + ["any-mask"])
def test_against_the_generic_entry(gn, i):
    rng = np.random.default_rng(200 + i)
    case = FULL_CASES[i] if i < len(FULL_CASES) else ANY_MASK_CASE
    c = make(gn, CN._adjs(rng), case, seed=i)
    if i < len(FULL_CASES):
        assert c.mask() == _want_mask(case, c.g), (case, c.mask())
    c.check(str(case[:4]))


# ---- 3. structural ----
def _structural(kind, rng):
    if kind == "hub":  # one node with more than 128 in-edges
        adjs = CN._adjs(rng, [150, 7, 12])
        adjs[0][:, 3] = 1
        assert int(adjs[0][:, 3].sum()) > 128
        return adjs, 1
    return CN._structural(kind, rng)


STRUCTURAL = CN.STRUCTURAL + ["hub"]


@pytest.mark.parametrize("wi", (0, 3), ids=("16-3", "32-32-7"))
@pytest.mark.parametrize("kind", STRUCTURAL)
def test_structural(gn, kind, wi):
    import torch
    rng = np.random.default_rng(400 + STRUCTURAL.index(kind) * 2 + wi)
    adjs, R = _structural(kind, rng)
    case = FULL_CASES[wi]
    c = make(gn, adjs, case, R, seed=50 + STRUCTURAL.index(kind))
    assert c.mask() == _want_mask(case, c.g), (kind, c.mask())
    outs = c.run(True)
    c.check(f"{kind} {case[1]}", narrow_outs=outs)
    if kind == "edgeless-batch":  # bit 0 clear; the edge layers' gradients exactly zero; the node and graph levels fused as the rule says
        assert c.mask() & 1 == 0 and c.mask() & 2 and (c.mask() == 6 or wi == 3)
        torch.cuda.synchronize()
        for n, t in outs.items():
            if n.startswith("edge"):
                assert bool((t == 0).all()), n
        if U.default_flags(gn) == 0 and c.mask() == 6:
            prof = CN._profiled(gn, lambda: c.run(True))
            assert prof["bw_delta"]["kernels"] == 2 and "bw_dx_generic" not in prof and "bw_chain_fw_g" not in prof, sorted(prof)


# ---- 4. outside the rule ----
def test_outside_the_rule(gn):
    import torch
    rng = np.random.default_rng(2)
    adjs = CN._adjs(rng)
    # 33 in every function: mask 0, the call IS gnx_chain_block_backward
    c = make(gn, adjs, ((10, 5, 3), [33, 3], [33, 4], [33, 5], (2, 3, 2)), seed=1)
    assert c.mask() == 0 and c.query(True) == c.query(False)
    a, b = c.run(True), c.run(False)
    torch.cuda.synchronize()
    assert sorted(a) == sorted(b)
    for n in a:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n
    # the node chain alone: the graph chain's parameter gradients keep the generic bits, the rest passes the item-2 check
    c = make(gn, adjs, ((10, 5, 3), [33, 3], [8, 4], [40, 5], (2, 3, 2)), seed=2)
    assert c.mask() == 2
    a, b = c.run(True), c.run(False)
    torch.cuda.synchronize()
    for n in a:
        if n.startswith("graph"):
            assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n
    c.check("mask 2", narrow_outs=a, only=lambda n: not n.startswith("graph"))
    # the edge and graph chains
    c = make(gn, adjs, ((10, 5, 3), [16, 3], [40, 4], [5], (2, 3, 2)), seed=3)
    assert c.mask() == 5
    c.check("mask 5")


# ---- 5. launch structure ----
def test_launch_structure(gn):
    rng = np.random.default_rng(1)
    c = make(gn, CN._adjs(rng), ((10, 5, 3), [16, 3], [8, "ln", 4], [6, 5], (4, 2, 1)), seed=4)
    assert c.mask() == 7
    assert 0 < c.query(True) < c.query(False), (c.query(True), c.query(False))
    if U.default_flags(gn) != 0:
        return  # (forms switched on for the whole process change which kernels the generic entry runs)
    c.run(True)
    new = CN._profiled(gn, lambda: c.run(True))
    old = CN._profiled(gn, lambda: c.run(False))
    assert new["bw_delta"]["kernels"] == 2 and new["bw_delta_edge"]["kernels"] == 1, new
    for n in new:
        assert n not in ("bw_dx_generic", "bw_dx_chain", "bw_layernorm", "bw_gelu_preact", "bw_chain_fw_g") and not n.startswith("k_rows_gemm"), sorted(new)
    total = lambda prof: sum(v["kernels"] for v in prof.values())
    assert total(new) < total(old), (total(new), total(old))
    print(f"chain bw narrow launch structure: {total(new)} kernels (generic: {total(old)}), workspace {c.query(True)} B (generic: {c.query(False)} B)")


# ---- 6. memory contract ----
@pytest.mark.parametrize("i,some_null", ((0, False), (2, False), (3, False), (6, False), (0, True)), ids=lambda v: str(v))
def test_memory_contract(gn, i, some_null):
    """every buffer carved at its exact size (4-byte aligned only: a skew of 4 bytes on every fp32 carve), the workspace exactly the query's;
    nothing but the requested outputs and the workspace is written; the bits depend neither on what the workspace held nor on the run"""
    import torch
    L, lib = gn._lib, gn._lib.load()
    case = FULL_CASES[i]
    src = make(gn, CN._adjs(np.random.default_rng(300 + i)), case, seed=70 + i)  # (the kink-free draw and its float64 gradients)
    p, g = src.p, src.g
    a = AR.Arena("cuda", skew=lambda c: 0 if c.kind == AR.WORKSPACE else 4)
    _decl_chains(a, p)
    ins = [_decl(a, n, v) for n, v in zip(("ef", "nf", "gf"), src.x)]
    gs = [None if c is None else _decl(a, n, c.cpu().numpy()) for n, c in zip(("g_ef_out", "g_nf_out", "g_gf_out"), src.cot)]
    null = {"d_nf", "edge0.dW", "node1.db", "graph0.dW", "graph0.db"} if some_null else set()
    dx = [a.output(n, v.shape) if v is not None and n not in null else None for n, v in zip(("d_ef", "d_nf", "d_gf"), src.x)]
    for name in ("edge", "node", "graph"):
        for k, (w, b, c) in enumerate(p[name]):
            if isinstance(w, str):
                a.output(f"grad.{name}{k}.dW", b.shape)
                a.output(f"grad.{name}{k}.db", c.shape)
            else:
                _decl_dense_grad(a, f"grad.{name}{k}", w, b)
    keep = []
    ws = a.workspace("ws", lambda: lib.gnx_chain_block_backward_narrow_workspace_bytes(g._h, C.byref(_chain_params(gn, a, p, keep)), 1))
    a.build(ws_fill=0x00)
    assert a.nbytes(ws) > 0, lib.gnx_last_error()
    assert all(a.ptr(n) % 8 == 4 for n in ins + gs + dx if n is not None)
    P = a.ptr

    def call(nbytes):
        arrays = []
        for name in ("edge", "node", "graph"):
            arr = (L.DenseGrad * max(len(p[name]), 1))()
            for k in range(len(p[name])):
                d = _dense_grad(gn, a, f"grad.{name}{k}")
                if f"{name}{k}.dW" in null:
                    d.weight = None
                if f"{name}{k}.db" in null:
                    d.bias = None
                arr[k] = d
            arrays.append(arr)
        gr = L.ChainBlockGrads(*[C.cast(x_, C.POINTER(L.DenseGrad)) for x_ in arrays])
        rc = lib.gnx_chain_block_backward_narrow(g._h, C.byref(_chain_params(gn, a, p, keep)), *map(P, ins), *map(P, gs), 1, *map(P, dx), C.byref(gr),
                                                 P(ws), nbytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    bits = []
    for fill in (0x00, 0xFF, 0xFF):
        a.refill(fill)
        torch.cuda.synchronize()
        assert call(a.nbytes(ws)) == 0, lib.gnx_last_error()
        if some_null:  # the carves of the gradients not asked for must stay as they were: checked as "unwritten" by not naming them outputs
            a.check(f"workspace {fill:#04x}", unwritten=False)
        else:
            a.check(f"workspace {fill:#04x}")
        for n, r in src.ref.items():
            if n in null or r.size == 0:
                continue
            got = a.numpy(n if n.startswith("d_") else "grad." + n).astype(np.float64)
            got = got[0] if n.startswith("d_") else got
            ref = r[0] if n.startswith("d_") else r
            assert np.max(np.abs(got - ref)) <= 1e-3 * max(1.0, float(np.abs(ref).max())), n
        bits.append(a.output_bits())
    for k in bits[0]:
        assert torch.equal(bits[0][k], bits[1][k]), f"'{k}' depends on what the workspace held"
        assert torch.equal(bits[1][k], bits[2][k]), f"'{k}' differs between two calls"
    if some_null:  # a gradient that was not asked for keeps the fill of its carve
        for n in ("grad.edge0.dW", "grad.node1.db", "grad.graph0.dW", "grad.graph0.db"):
            assert bool((bits[1][n].view(torch.uint8) == 0xFF).all()), n
    a.refill(0x00)
    torch.cuda.synchronize()
    before, ws_before = a.output_bits(), a.raw(ws).clone()
    assert call(a.nbytes(ws) - 1) == L.ERR_WORKSPACE and b"gnx_chain_block_backward_narrow_workspace_bytes()" in lib.gnx_last_error()
    a.check("refused", unwritten=False)
    after = a.output_bits()
    assert all(torch.equal(before[k], after[k]) for k in before) and torch.equal(ws_before, a.raw(ws)), "a refused call wrote an output or the workspace"


# ---- 7. capture ----
def test_a_captured_call_replays_the_eager_bits(gn):
    import torch
    rng = np.random.default_rng(4)
    c = make(gn, CN._adjs(rng), FULL_CASES[6], seed=5)
    nbytes = c.query()  # (builds the tables the call reads, outside the capture)
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device=c.g.device)
    eager = c.run(ws=ws)
    torch.cuda.synchronize()
    graphed = c.grads()
    side = torch.cuda.Stream()
    cg = torch.cuda.CUDAGraph()
    # nothing may free device memory while the capture is open: garbage of earlier tests (an arena and its batch handle sit in a reference cycle)
    # is collected now, and the collector rests until the capture has ended
    gc.collect()
    gc.disable()
    try:
        with torch.cuda.stream(side):
            with torch.cuda.graph(cg, stream=side):
                c.run(outs=graphed, ws=ws, stream=side.cuda_stream, nbytes=nbytes)
    finally:
        gc.enable()
    for t in graphed.values():
        t.zero_()
    cg.replay()
    torch.cuda.synchronize()
    for n in eager:
        assert torch.equal(eager[n].view(torch.int32), graphed[n].view(torch.int32)), n


# ---- 8. the Python switch ----
def test_python_switch_gives_the_entrys_bits(gn):
    import torch
    rng = np.random.default_rng(5)
    c = make(gn, CN._adjs(rng), FULL_CASES[2], seed=6)
    want = c.run(True)
    blk = c.blk
    assert blk.narrow_chain_backward is False
    blk.narrow_chain_backward = True
    leaves = []
    for ch in (blk.edgefn, blk.nodefn, blk.graphfn):
        for l in ch.layers:
            l.weight.requires_grad_(True); l.bias.requires_grad_(True)
            leaves.append((l.weight, l.bias))
    xt = [None if t is None else t.clone().requires_grad_(True) for t in c.xt]
    y = blk(gn.NT(c.g, *(None if t is None else t.permute(2, 1, 0) for t in xt)))
    sum((o.permute(2, 1, 0) * ct).sum() for o, ct in zip((y.ef, y.nf, y.gf), c.cot) if o is not None).backward()
    torch.cuda.synchronize()
    same = lambda u, v: torch.equal(u.contiguous().view(torch.int32), v.contiguous().view(torch.int32))
    for n, t in zip(("d_ef", "d_nf", "d_gf"), xt):
        if t is not None:
            assert same(t.grad, want[n]), n
    k = 0
    for name in ("edge", "node", "graph"):
        for i in range(len(c.p[name])):
            w, b = leaves[k]; k += 1
            gw = w.grad if w.grad.dim() == 1 else w.grad.t()
            assert same(gw, want[f"{name}{i}.dW"]) and same(b.grad, want[f"{name}{i}.db"]), (name, i)


# ---- 9. seeded sweep ----
def _ln_widths(case):
    """the width every LayerNorm of the case normalises over"""
    (de, dn, dg), ew, nw, gw, _ = case
    out, outs = [], []
    for t, ws in enumerate((ew, nw, gw)):
        k = de + 2 * dn + dg if t == 0 else (outs[0] + dn + dg if t == 1 else outs[0] + outs[1] + dg)
        for w in ws:
            if w == "ln":
                out.append(k)
            else:
                k = w
        outs.append(k if ws else 0)
    return out


def _random_bw_block(rng):
    """tests.test_gpu_chain_narrow._random_block's draws that have a pullback to compare with: an edge output (the backward refuses a block
    without one) and no LayerNorm over fewer than 3 elements.  Over one element the normalised value is the constant 0 and float64 autograd
    of the restatement returns NaN (the derivative of sqrt at 0); over two it is +-(1 - eps / (sigma + eps)), whose derivative is the
    difference of two terms of size 1 / sigma that cancel to eps / (sigma + eps)^2 — in fp32 nothing of it is left, for any summation order:
    gnx_chain_block_backward misses the bar on such draws as well.  test_tiny_layernorms pins both widths against the generic entry."""
    while True:
        case = CN._random_block(rng)
        if case[1] and all(k >= 3 for k in _ln_widths(case)):
            return case


@pytest.mark.parametrize("seed", range(24 + EXTRA))
def test_seeded_sweep(gn, monkeypatch, seed):
    made = []
    _switched(monkeypatch, made, seed % 2 == 1)
    for attempt in range(40):  # (a relu pre-activation on its kink is drawn again, never skipped)
        rng = np.random.default_rng(7000 + seed + 1000 * attempt)
        in_dims, ew, nw, gw, acts = _random_bw_block(rng)
        g = _er_batch(gn, rng)
        if TC.chain_block_backward_case(gn, g, rng, in_dims, ew, nw, gw, acts, fp32_yardstick=True):
            assert made and made[-1].narrow_chain_backward is True
            return
    pytest.fail("no kink-free draw in 40 attempts")


def test_the_committed_record_supports_the_rule():
    """profiles/chain_bw_narrow.json, as tools/time_chain_bw_narrow.py wrote it on an MI355X: the times were measured, every case under the
    committed rule met the bar (narrow median <= parent median + the parent's spread), and the worst ratio of the item-2 check was below 1"""
    with open(os.path.join(ROOT, "profiles", "chain_bw_narrow.json")) as f:
        rec = json.load(f)
    assert rec["measured"] is True and len(rec["cases"]) == 8
    assert 0.0 <= rec["worst_ratio_to_bound"] <= 1.0 and rec["ratio_checks"] >= 20
    assert rec["slower_than_parent_beyond_spread"] == [] and all(c["not_slower_beyond_spread"] for c in rec["cases"])
    for c in rec["cases"]:  # the recorded masks are the committed rule's
        case = (tuple(c["in_dims"]), c["edge"], c["node"], c["graph"])
        counts = type("G", (), dict(n_edges=c["E"], n_nodes=c["N"], n_graphs=c["G"]))
        assert c["applies"] == _want_mask(case, counts), (case, c["applies"])


# ---- 10. LayerNorms over one and two elements (the sweep draws none: see _random_bw_block) ----
def test_tiny_layernorms(gn):
    """Over two elements, all three functions fused: the item-2 check.  Over one element the normalised value is the constant 0: float64 autograd
    of the restatement is NaN there, the kernel's `q > 0 ? ... : 0` branch gives dx = 0 — every gradient in front of that LayerNorm is exactly
    0, its gamma gradient too, nothing is NaN, and the tensors that have a reference pass the item-2 check."""
    import torch
    case = ((0, 10, 5), [2, "ln"], [1, 16, 8], [15, 17, 32], (3, 3, 3))
    c = BwCall(gn, CN._adjs(np.random.default_rng(21)), CN._params(np.random.default_rng(21), case), 1, 21)
    assert c.ok and c.mask() == _want_mask(case, c.g) == 7
    c.check("layernorm over 2")
    case = ((0, 0, 7), [5, "ln", 3, 1, "ln", 12], [], [31, "ln", 3, 7, "ln"], (2, 3, 3))
    c = BwCall(gn, CN._adjs(np.random.default_rng(23)), CN._params(np.random.default_rng(23), case), 1, 23)
    assert c.ok and c.mask() == _want_mask(case, c.g) and c.mask() & 1
    a = c.run(True)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in a.values())
    for n in ("edge0.dW", "edge0.db", "edge1.dW", "edge1.db", "edge2.dW", "edge2.db", "edge3.dW", "edge3.db", "edge4.dW"):
        assert bool((a[n] == 0).all()), n
    c.check("layernorm over 1", narrow_outs=a, only=lambda n: not np.isnan(c.ref[n]).any())
