"""gnx_chain_block_forward_wave: a Chain block's edge and node function in one wave-per-tile kernel, the graph function from its partial rows
(csrc/gnx_chain_wave.hip).  Inside the rule: `_applies` is 1, ef' and nf' are byte for byte gnx_chain_block_forward_narrow's, gf' is within
1e-5 . scale of the float64 oracle, NaN-filled outputs are fully written and the bytes do not depend on what the workspace held.  Outside it:
`_applies` is 0 and all three outputs are the narrow entry's bytes.  The rule cuts register width 32 on batches of several graphs
(csrc/gnx_chain_plan.h: chain_wave_cut), so every width case runs on the five-graph batch and on one graph."""
import ctypes as C

import numpy as np
import pytest

from oracle import gn_oracle as O
from tests import test_gpu_chain as TC
from tests import util as U
from tests.test_gpu_chain_narrow import WIDTH_CASES, Call, _adjs, _params, gn  # noqa: F401  (gn: the module's fixture)

pytestmark = pytest.mark.gpu
CAP = 128  # the default wave-tile edge cap
W16 = ((3, 2, 1), [9, 12, 4], [16, "ln", 5], ["ln", 9, 4, "ln"], (4, 3, 1))  # register width 16: inside the rule on a batch of several graphs


def wide(case):
    """an input or layer width of the edge or the node function beyond 16: the kernel's 32-wide instantiation"""
    (de, dn, dg), ew, nw = case[:3]
    num = lambda ws: [w for w in ws if w != "ln"]
    ke = de + 2 * dn + dg
    oe = (num(ew) or [ke])[-1]
    return max([ke, oe + dn + dg] + num(ew) + num(nw)) > 16


class CscCall(Call):
    """Call on graphs given as (colptr, rowval, nodes) — sizes no dense adjacency matrix reaches"""

    def __init__(self, gn, graphs, p, seed=0):
        import torch
        self.gn, self.L, self.lib, self.p, self.R = gn, gn._lib, gn._lib.load(), p, 1
        self.g = gn.GNGraphBatch.from_csc([c for c, _, _ in graphs], [r for _, r, _ in graphs], [n for _, _, n in graphs])
        node_off = np.cumsum([0] + [n for _, _, n in graphs])
        colptr = np.concatenate([[0]] + [c[1:] + e for (c, _, _), e in zip(graphs, np.cumsum([0] + [len(r) for _, r, _ in graphs]))])
        rowval = np.concatenate([r + o for (_, r, _), o in zip(graphs, node_off)])
        self.csc = (colptr, rowval, node_off, colptr[node_off])
        self.x = U.packed_inputs(np.random.default_rng(9000 + seed), 1, self.g.n_edges, self.g.n_nodes, self.g.n_graphs, p["in_dims"])
        self.xt = [None if a is None else torch.from_numpy(a).to(self.g.device) for a in self.x]
        self.blk = TC._block(gn, p)
        self.keep = []
        self.cp, _, self.outw = self.blk._chain_params(self.keep)


def wave(c, fill=0xA5, outs=None, ws=None, stream=None):
    """the wave entry on a workspace of exactly the queried size, filled with `fill`; the outputs start as NaN"""
    import torch
    nbytes = c.lib.gnx_chain_block_forward_wave_workspace_bytes(c.g._h, C.byref(c.cp), c.R)
    assert nbytes > 0, c.lib.gnx_last_error()
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=c.g.device) if ws is None else ws
    outs = c.outputs() if outs is None else outs
    ptr = lambda t: None if t is None else t.data_ptr()
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    rc = c.lib.gnx_chain_block_forward_wave(c.g._h, C.byref(c.cp), *map(ptr, c.xt), c.R, *map(ptr, outs), ws.data_ptr(), nbytes, 0, s)
    assert rc == 0, c.lib.gnx_last_error()
    return outs


def same(u, v):
    import torch
    return (u is None and v is None) or torch.equal(u.view(torch.int32), v.view(torch.int32))


def verify(c, inside, what):
    import torch
    assert c.lib.gnx_chain_block_forward_wave_applies(c.g._h, C.byref(c.cp), c.R) == int(inside), what
    a, b, narrow = wave(c, 0x00), wave(c, 0xA5), c.run()
    torch.cuda.synchronize()
    assert all(t is None or not bool(torch.isnan(t).any()) for t in a), f"{what}: an output keeps NaN"
    assert all(same(u, v) for u, v in zip(a, b)), f"{what}: the bytes depend on what the workspace held"
    assert same(a[0], narrow[0]) and same(a[1], narrow[1]), f"{what}: ef' / nf' are not the narrow entry's bytes"
    if inside:
        c.check(a, what)
    else:
        assert same(a[2], narrow[2]), f"{what}: outside the rule gf' is not the narrow entry's bytes"
    return a


@pytest.mark.parametrize("graphs", [5, 1])
@pytest.mark.parametrize("i", range(len(WIDTH_CASES)), ids=[str(c[:4]) for c in WIDTH_CASES])
def test_widths(gn, i, graphs):
    rng = np.random.default_rng(100 + i)
    case = WIDTH_CASES[i]
    adjs = _adjs(rng) if graphs == 5 else _adjs(rng, [40])
    verify(Call(gn, adjs, _params(rng, case), seed=i), inside=bool(case[2]) and (graphs == 1 or not wide(case)), what=str(case[:4]))


def _tiles(kind, rng):
    """(adjacency matrices, R, inside the rule)"""
    if kind == "node-and-edge-cap":  # 70 nodes with one in-edge (a tile of 64 nodes), then ~15 in-edges per node (tiles of ~8 nodes: the edge cap)
        a = (rng.random((150, 150)) < 0.1).astype(np.int64)
        a[:, :70] = 0
        a[rng.integers(0, 150, 70), np.arange(70)] = 1
        return [a] + _adjs(rng, [4, 9]), 1, True
    if kind == "empty-columns":  # no in-edges at the first and the last node of a graph's first / last tile and inside; a graph without edges
        a = (rng.random((40, 40)) < 0.3).astype(np.int64)
        a[:, [0, 1, 17, 38, 39]] = 0
        return [a, np.zeros((5, 5), dtype=np.int64)] + _adjs(rng, [12]), 1, True
    if kind in ("degree-cap", "degree-cap+1"):  # one node with CAP (inside the rule) / CAP + 1 in-edges (outside)
        a = (rng.random((CAP + 2, CAP + 2)) < 0.02).astype(np.int64)
        deg = CAP + (kind == "degree-cap+1")
        a[:, 3] = 0
        a[:deg, 3] = 1
        return [a], 1, deg <= CAP
    if kind == "replicas-3":
        return _adjs(rng, [31]), 3, True
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["node-and-edge-cap", "empty-columns", "degree-cap", "degree-cap+1", "replicas-3"])
def test_tiles(gn, kind):
    rng = np.random.default_rng(200)
    adjs, R, inside = _tiles(kind, rng)
    c = Call(gn, adjs, _params(rng, WIDTH_CASES[2] if len(adjs) == 1 else W16), R)  # (one graph: the 32-wide instantiation)
    if kind.startswith("degree-cap"):
        assert c.g.max_in_degree == CAP + (not inside)
    verify(c, inside, kind)


def _ring(tiles):
    """64 . tiles nodes, in-edges from both ring neighbours: every wave tile ends on the node cap with exactly CAP edges"""
    n = 64 * tiles
    j = np.arange(n)
    rowval = np.sort(np.stack([(j - 1) % n, (j + 1) % n], axis=1), axis=1).reshape(-1)
    return 2 * np.arange(n + 1, dtype=np.int64), rowval.astype(np.int64), n


@pytest.mark.parametrize("tiles", [(256,), (257,), (1023,), (1024,), (257, 2)], ids=str)
def test_graph_level(gn, tiles):
    """either side of the finishing kernel's thresholds (one wavefront per graph up to 256 partial rows, 256 threads, 1024 from 1024 rows on)"""
    rng = np.random.default_rng(300)
    c = CscCall(gn, [_ring(t) for t in tiles], _params(rng, WIDTH_CASES[2] if len(tiles) == 1 else W16))
    verify(c, True, f"ring {tiles}")


@pytest.mark.parametrize("edge, inside", [([16, 32], True), ([32] * 8, False)], ids=["two-waves", "refused"])
def test_lds_rule(gn, edge, inside):
    """oe = 32: a slice of 128 x 33 floats per wave — 952 parameter floats leave room for two waves (3.65 slices); 7680 + 264 = 7944 > 16384 - 2 x 4224"""
    rng = np.random.default_rng(400)
    verify(Call(gn, _adjs(rng, [40]), O.make_chain_block_params(rng, (6, 0, 0), edge, [8], [])), inside, str(edge))


def test_a_captured_call_replays_the_eager_bytes(gn):
    import torch
    rng = np.random.default_rng(500)
    c = Call(gn, _adjs(rng), _params(rng, W16))
    nbytes = c.lib.gnx_chain_block_forward_wave_workspace_bytes(c.g._h, C.byref(c.cp), c.R)  # (builds the tables the call reads, outside the capture)
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device=c.g.device)
    eager = wave(c, ws=ws)
    torch.cuda.synchronize()
    graphed, side, cg = c.outputs(), torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(cg, stream=side):
            wave(c, outs=graphed, ws=ws, stream=side.cuda_stream)
    for _ in range(3):
        for t in graphed:
            t.fill_(float("nan"))
        cg.replay()
        torch.cuda.synchronize()
        assert all(same(u, v) for u, v in zip(eager, graphed))


def test_python_switch(gn):
    """GNBlock(..., wave_chain=True): the forward is the direct entry's; a gradient call gives narrow_chain's gradients byte for byte"""
    import torch
    rng = np.random.default_rng(600)
    c = Call(gn, _adjs(rng), _params(rng, W16))
    assert c.lib.gnx_chain_block_forward_wave_applies(c.g._h, C.byref(c.cp), c.R) == 1
    want = wave(c)
    assert c.blk.wave_chain is False and gn.GNBlock((3, 2, 1), (1, 1, 1), device="cpu", wave_chain=True).wave_chain is True
    c.blk.wave_chain = True
    with torch.no_grad():
        y = c.blk(U.to_nt(gn, c.g, *c.x))
    torch.cuda.synchronize()
    assert all(same(got.permute(2, 1, 0).contiguous(), w) for got, w in zip((y.ef, y.nf, y.gf), want))

    leaves = [t for ch in (c.blk.edgefn, c.blk.nodefn, c.blk.graphfn) for l in ch.layers for t in (l.weight, l.bias)]
    for t in leaves:
        t.requires_grad_(True)

    def grads(switch):
        c.blk.wave_chain, c.blk.narrow_chain = switch == "wave_chain", switch == "narrow_chain"
        xt = [torch.from_numpy(a).to(c.g.device).requires_grad_(True) for a in c.x]
        for t in leaves:
            t.grad = None
        y = c.blk(gn.NT(c.g, *(t.permute(2, 1, 0) for t in xt)))
        (y.ef.sum() + 2 * y.nf.sum() + 3 * y.gf.sum()).backward()
        torch.cuda.synchronize()
        return [t.grad.clone() for t in xt + leaves]

    assert all(same(u, v) for u, v in zip(grads("wave_chain"), grads("narrow_chain")))
