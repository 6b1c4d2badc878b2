"""gnx_chain_block_forward_narrow: a GNBlock whose update functions are Chains with every update function of narrow widths in ONE kernel
(csrc/gnx_chain_narrow.hip) — against the float64 oracle at every register-width bucket edge and source form, that the fused form ran, what
happens outside the rule, the memory contract on exactly sized 4-byte-aligned buffers, stream capture, the Python switch and a seeded sweep."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import gn_oracle as O
from tests import arena as AR
from tests import util as U
from tests import test_gpu_chain as TC
from tests.test_gpu_memory_contract import _chain_out_widths, _chain_params, _decl, _decl_chains, _decl_outputs

pytestmark = pytest.mark.gpu
EXTRA = int(os.environ.get("GNX_FUZZ_EXTRA", "0"))
NAMES = ("k_rows_gemm_chain_e", "k_rows_gemm_chain_n", "k_rows_gemm_chain_g")


@pytest.fixture(scope="module")
def gn():
    import torch
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


def _adjs(rng, sizes=None):
    """five graphs of 3..40 nodes at density 0.3, as tests/test_gpu_chain.py draws them"""
    sizes = rng.integers(3, 40, 5) if sizes is None else sizes
    return [(rng.random((n, n)) < 0.3).astype(np.int64) for n in sizes]


class Call:
    """one block on one batch, on torch tensors: the parameters, the inputs, and either entry on a workspace of exactly the queried size"""

    def __init__(self, gn, adjs, p, R=1, seed=0):
        import torch
        self.gn, self.L, self.lib, self.p, self.R = gn, gn._lib, gn._lib.load(), p, R
        self.g = gn.GNGraphBatch(adjs)
        self.csc = O.csc_from_adj(adjs)
        self.x = U.packed_inputs(np.random.default_rng(9000 + seed), R, self.g.n_edges, self.g.n_nodes, self.g.n_graphs, p["in_dims"])
        dev = self.g.device
        self.xt = [None if a is None else torch.from_numpy(a).to(dev) for a in self.x]
        self.blk = TC._block(gn, p)
        self.keep = []
        self.cp, _, self.outw = self.blk._chain_params(self.keep)

    def mask(self):
        return self.lib.gnx_chain_block_forward_narrow_applies(self.g._h, C.byref(self.cp), self.R)

    def query(self, narrow=True):
        q = self.lib.gnx_chain_block_forward_narrow_workspace_bytes if narrow else self.lib.gnx_chain_block_workspace_bytes
        return q(self.g._h, C.byref(self.cp), self.R)

    def outputs(self):
        import torch
        rows = (self.g.n_edges, self.g.n_nodes, self.g.n_graphs)
        return [torch.full((self.R, T, d), float("nan"), dtype=torch.float32, device=self.g.device) if d > 0 else None for T, d in zip(rows, self.outw)]

    def run(self, narrow=True, outs=None, ws=None, fill=0xA5, stream=None):
        import torch
        nbytes = self.query(narrow)
        assert nbytes > 0, self.lib.gnx_last_error()
        if ws is None:
            ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=self.g.device)
        outs = self.outputs() if outs is None else outs
        ptr = lambda t: None if t is None else t.data_ptr()
        entry = self.lib.gnx_chain_block_forward_narrow if narrow else self.lib.gnx_chain_block_forward
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        rc = entry(self.g._h, C.byref(self.cp), *map(ptr, self.xt), self.R, *map(ptr, outs), ws.data_ptr(), nbytes, 0, s)
        assert rc == 0, self.lib.gnx_last_error()
        return outs

    def check(self, outs, what):
        """against the float64 oracle at the project's 1e-5 . scale; returns the worst ratio to that bound"""
        import torch
        torch.cuda.synchronize()
        ref, scale = O.chain_block_forward_sparse(self.p, self.csc, *self.x, return_scale=True)
        worst = 0.0
        for name, got, r, s in zip(("ef", "nf", "gf"), outs, ref, scale):
            got = None if got is None else got.cpu().numpy()
            if r is not None and r.size:
                worst = max(worst, float(np.max(np.abs(got.astype(np.float64) - r) / (U.RTOL * s + 1e-30))))
            U.assert_close(got, r, s, f"{what} {name}")
        print(f"chain narrow {what}: worst |diff| / (1e-5 scale) = {worst:.3e}")
        return worst


WIDTH_CASES = [
    ((10, 5, 0), [16, 3], [8, 4], [6, 5], None),                                         # gf nothing
    ((2, 2, 1), [8, 8, 1], [3], [2], None),                                              # all widths <= 8
    ((3, 2, 1), [9, 17, 4], [16, "ln", 5], ["ln", 9, 4, "ln"], (4, 3, 1)),               # gelu, sigmoid, relu; the 16 / 32 buckets by one
    ((8, 8, 8), [32, "ln", 32, 32, 7], ["ln", 32, 32, 9], [32, "ln", 17, 4], (1, 2, 0)),  # K_e = 32, layer widths up to 32
    ((0, 4, 2), [8, 5], [5], [], None),                                                  # ef nothing, no graph output
    ((6, 0, 0), [4, 3], [], [], None),                                                   # edge function only
    ((10, 5, 3), ["ln", 12, 7], [6], [4], None),                                         # LayerNorm as the edge function's first layer
    ((3, 2, 1), [8] * 8, [8, 8, 8], [8, 8], None),                                       # long chains
]


def _params(rng, case):
    in_dims, ew, nw, gw, acts = case
    return O.make_chain_block_params(rng, in_dims, ew, nw, gw) if acts is None else O.make_chain_block_params(rng, in_dims, ew, nw, gw, acts=acts)


def _structural(kind, rng):
    """(adjacency matrices, R) of the structural cases"""
    if kind == "isolated-column":
        adjs = _adjs(rng)
        adjs[2][:, 1] = 0   # node 1 of graph 2 has no incoming edge: an empty sum
        adjs[0][:, 0] = 0   # ... and the first node of the batch
        return adjs, 1
    if kind == "graph-without-edges":
        adjs = _adjs(rng)
        adjs[3][:] = 0
        return adjs, 1
    if kind == "partial-workgroup":
        adjs = _adjs(rng, [37, 5, 29, 33, 11])
        E = int(sum(a.sum() for a in adjs))
        assert E > 256 and E % 64 != 0, E
        return adjs, 1
    if kind == "edgeless-batch":
        return [np.zeros((n, n), dtype=np.int64) for n in (3, 5, 1, 2)], 1
    if kind in ("replicas-2", "replicas-3"):
        return _adjs(rng, [31]), int(kind[-1])
    raise KeyError(kind)


STRUCTURAL = ["isolated-column", "graph-without-edges", "partial-workgroup", "edgeless-batch", "replicas-2", "replicas-3"]


@pytest.mark.parametrize("i", range(len(WIDTH_CASES) + len(STRUCTURAL)), ids=[str(c[:4]) for c in WIDTH_CASES] + STRUCTURAL)
def test_against_the_float64_oracle(gn, i):
    rng = np.random.default_rng(100 + i)
    if i < len(WIDTH_CASES):
        case, adjs, R, what = WIDTH_CASES[i], _adjs(rng), 1, str(WIDTH_CASES[i][:4])
    else:
        kind = STRUCTURAL[i - len(WIDTH_CASES)]
        case, what = WIDTH_CASES[3 if kind == "partial-workgroup" else 0], kind
        adjs, R = _structural(kind, rng)
    c = Call(gn, adjs, _params(rng, case), R, seed=i)
    want = (1 if case[1] and c.g.n_edges > 0 else 0) | (2 if case[2] else 0) | (4 if case[3] else 0)
    assert c.mask() == want, (what, c.mask(), want)
    c.check(c.run(), what)
    if what == "edgeless-batch":  # no edge launch; the node and graph functions still run
        prof = _profiled(gn, c.run)
        assert sorted(prof) == sorted(NAMES[1:]), sorted(prof)


def _profiled(gn, f):
    import torch
    gn.profile_reset(); gn.profile_enable(True)
    try:
        f()
        torch.cuda.synchronize()
    finally:
        gn.profile_enable(False)
    out = gn.profile_read(); gn.profile_reset()
    return out


def test_the_fused_form_ran(gn):
    """one launch per update function under the three chain names, nothing of the block forward, a smaller workspace"""
    rng = np.random.default_rng(1)
    c = Call(gn, _adjs(rng), _params(rng, WIDTH_CASES[0]))
    assert c.mask() == 7
    assert 0 < c.query(True) < c.query(False), (c.query(True), c.query(False))
    if U.default_flags(gn) != 0:
        return  # (forms switched on for the whole process change which kernels the old entry runs)
    c.run()
    prof = _profiled(gn, c.run)
    assert sorted(prof) == sorted(NAMES), f"other kernels than the three fused launches ran: {sorted(prof)}"
    for n in NAMES:
        assert prof[n]["launches"] == 1 and prof[n]["kernels"] == 1, (n, prof[n])
    old = _profiled(gn, lambda: c.run(narrow=False))
    assert set(NAMES) < set(old), sorted(old)  # gnx_chain_block_forward: the block forward's kernels + one launch per further layer
    assert (old[NAMES[0]]["kernels"], old[NAMES[1]]["kernels"], old[NAMES[2]]["kernels"]) == (1, 2, 2), old


def test_outside_the_rule(gn):
    import torch
    rng = np.random.default_rng(2)
    adjs = _adjs(rng)
    # a width of 33 in every function: mask 0, the call IS gnx_chain_block_forward
    c = Call(gn, adjs, O.make_chain_block_params(rng, (10, 5, 3), [33, 3], [33, 4], [33, 5]))
    assert c.mask() == 0 and c.query(True) == c.query(False)
    a, b = c.run(True), c.run(False)
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    # a 33-wide hidden layer in the edge chain, an eligible node chain (and a graph chain outside the rule): mask 2, ef' keeps its bits
    c = Call(gn, adjs, O.make_chain_block_params(rng, (10, 5, 3), [33, 3], [8, 4], [40, 5]))
    assert c.mask() == 2 and c.query(True) < c.query(False)
    a, b = c.run(True), c.run(False)
    torch.cuda.synchronize()
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    c.check(a, "mask 2")
    # the edge chain alone is eligible
    c = Call(gn, adjs, O.make_chain_block_params(rng, (10, 5, 3), [16, 3], [40, 4], [5]))
    assert c.mask() == 5
    c.check(c.run(), "mask 5")


@pytest.mark.parametrize("i", (0, 2, 3, 6), ids=lambda i: str(WIDTH_CASES[i][:4]))
def test_memory_contract(gn, i):
    """every buffer carved at its exact size (4-byte aligned only: a skew of 4 bytes on every fp32 carve), the workspace exactly the query's;
    nothing but the outputs and the workspace is written; the bits depend neither on what the workspace held nor on the run"""
    import torch
    L, lib = gn._lib, gn._lib.load()
    rng = np.random.default_rng(300 + i)
    adjs = _adjs(rng)
    R = 1
    g, csc = gn.GNGraphBatch(adjs), O.csc_from_adj(adjs)
    p = _params(rng, WIDTH_CASES[i])
    a = AR.Arena("cuda", skew=lambda c: 0 if c.kind == AR.WORKSPACE else 4)
    _decl_chains(a, p)
    x = U.packed_inputs(rng, R, g.n_edges, g.n_nodes, g.n_graphs, p["in_dims"])
    ins = [_decl(a, n, v) for n, v in zip(("ef", "nf", "gf"), x)]
    outs = _decl_outputs(a, "", R, (g.n_edges, g.n_nodes, g.n_graphs), _chain_out_widths(p))
    keep = []
    ws = a.workspace("ws", lambda: lib.gnx_chain_block_forward_narrow_workspace_bytes(g._h, C.byref(_chain_params(gn, a, p, keep)), R))
    a.build(ws_fill=0x00)
    assert a.nbytes(ws) > 0, lib.gnx_last_error()
    assert all(a.ptr(n) % 8 == 4 for n in ins + outs if n is not None)
    ref = O.chain_block_forward_sparse(p, csc, *x, return_scale=True)
    bits = []
    for fill in (0x00, 0xFF, 0xFF):
        a.refill(fill)
        torch.cuda.synchronize()
        P = a.ptr
        rc = lib.gnx_chain_block_forward_narrow(g._h, C.byref(_chain_params(gn, a, p, keep)), *map(P, ins), R, *map(P, outs), P(ws), a.nbytes(ws), 0,
                                                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0, lib.gnx_last_error()
        a.check(f"workspace {fill:#04x}")
        for n, r, s in zip(outs, *ref):
            if n is not None:
                U.assert_close(a.numpy(n), r, s, n)
        bits.append(a.output_bits())
    for k in bits[0]:
        assert torch.equal(bits[0][k], bits[1][k]), f"'{k}' depends on what the workspace held"
        assert torch.equal(bits[1][k], bits[2][k]), f"'{k}' differs between two calls"
    # one byte less than the query: refused in the query's name, nothing written
    a.refill(0x00)
    rc = lib.gnx_chain_block_forward_narrow(g._h, C.byref(_chain_params(gn, a, p, keep)), *map(a.ptr, ins), R, *map(a.ptr, outs), a.ptr(ws), a.nbytes(ws) - 1, 0,
                                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == L.ERR_WORKSPACE and b"gnx_chain_block_forward_narrow_workspace_bytes()" in lib.gnx_last_error()
    a.check("refused", unwritten=False)


def test_a_captured_call_replays_the_eager_bits(gn):
    import torch
    rng = np.random.default_rng(4)
    c = Call(gn, _adjs(rng), _params(rng, WIDTH_CASES[6]))
    nbytes = c.query()  # (builds the tables the call reads, outside the capture)
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device=c.g.device)
    eager = c.run(ws=ws)
    torch.cuda.synchronize()
    graphed = c.outputs()
    side = torch.cuda.Stream()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(cg, stream=side):
            c.run(outs=graphed, ws=ws, stream=side.cuda_stream)
    for t in graphed:
        t.zero_()
    cg.replay()
    torch.cuda.synchronize()
    for u, v in zip(eager, graphed):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_python_switch_gives_the_entrys_bits(gn):
    import torch
    rng = np.random.default_rng(5)
    c = Call(gn, _adjs(rng), _params(rng, WIDTH_CASES[2]))
    want = c.run()
    x = U.to_nt(gn, c.g, *c.x)
    assert c.blk.narrow_chain is False
    off = _profiled(gn, lambda: c.blk(x))
    c.blk.narrow_chain = True
    with torch.no_grad():
        y = c.blk(x)
        on = _profiled(gn, lambda: c.blk(x))
    torch.cuda.synchronize()
    for got, w in zip((y.ef, y.nf, y.gf), want):
        assert torch.equal(got.permute(2, 1, 0).contiguous().view(torch.int32), w.view(torch.int32))
    if U.default_flags(gn) == 0:  # off: one launch per further layer; on: one per function
        assert [off[n]["kernels"] for n in NAMES] == [2, 2, 2] and off["k_chain_layernorm"]["kernels"] == 3, off  # (Dense layers; the three LayerNorms of the node and graph chains)
        assert sorted(on) == sorted(NAMES) and [on[n]["kernels"] for n in NAMES] == [1, 1, 1], on


def test_backward_through_the_switch(gn, monkeypatch):
    """loss.backward() through _ChainBlockFn with the forward on the fused entry: every input and parameter gradient against float64 torch autograd
    of tests.test_gpu_chain._torch_chain_block, at that file's tolerance, smooth activations"""
    made = []
    plain = TC._block

    def switched(gn_, p):
        blk = plain(gn_, p)
        blk.narrow_chain = True
        made.append(blk)
        return blk

    monkeypatch.setattr(TC, "_block", switched)
    rng = np.random.default_rng(6)
    sizes = rng.integers(3, 30, 5)
    cs = [U.er_csc(rng, int(n), int(0.2 * n * n) + 1) for n in sizes]
    g = gn.GNGraphBatch.from_csc([c[0] for c in cs], [c[1] for c in cs], [int(n) for n in sizes])
    assert TC.chain_block_backward_case(gn, g, rng, (10, 5, 3), [16, "ln", 3], [8, 4], ["ln", 6, 5], (2, 3, 4))
    assert len(made) == 1 and made[0].narrow_chain is True


def _random_block(rng):
    """widths 0..32, 1..4 layers per function, LayerNorms at random places, random `nothing` inputs"""
    while True:
        in_dims = tuple(int(v) if rng.random() < 0.75 else 0 for v in rng.integers(1, 11, 3))
        if sum(in_dims) == 0 or in_dims[0] + 2 * in_dims[1] + in_dims[2] > 32:
            continue
        chains, k_in, outs = [], in_dims[0] + 2 * in_dims[1] + in_dims[2], []
        for t in range(3):
            if t == 1:
                k_in = outs[0] + in_dims[1] + in_dims[2]
            elif t == 2:
                k_in = outs[0] + outs[1] + in_dims[2]
            ws, k = [], k_in
            if rng.random() < 0.85:  # (else: no such output — a width of 0)
                for _ in range(int(rng.integers(1, 5))):
                    if k > 0 and rng.random() < 0.25:
                        ws.append("ln")
                    k = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 24, 31, 32]))
                    ws.append(k)
                if rng.random() < 0.2:
                    ws.append("ln")
            chains.append(ws)
            outs.append(k if ws else 0)
        if sum(outs) > 0:
            acts = tuple(int(v) for v in rng.integers(0, 5, 3))
            return in_dims, chains[0], chains[1], chains[2], acts


@pytest.mark.parametrize("seed", range(24 + EXTRA))
def test_seeded_sweep(gn, seed):
    rng = np.random.default_rng(7000 + seed)
    case = _random_block(rng)
    R = 1
    adjs = _adjs(rng)
    if seed % 6 == 5:
        adjs, R = _adjs(rng, [int(rng.integers(3, 40))]), int(rng.integers(2, 4))
    c = Call(gn, adjs, _params(rng, case), R, seed=seed)
    assert c.mask() != 0, case
    c.check(c.run(), f"sweep {seed} {case}")
