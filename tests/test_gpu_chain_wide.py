"""gnx_chain_block_forward_wide: each update function of a Chain block at matrix-core widths in one kernel (csrc/gnx_chain_wide.hip).  Every case:
`_applies` is the expected mask, NaN-filled outputs come back fully written, the bytes do not depend on what a workspace of exactly the queried
size held, every output is within 1e-5 . scale of the float64 oracle, and a function outside the mask that reads nothing of a function inside it
gives the narrow entry's bytes.  The rule cuts a Dense layer beyond 64 columns after measurement (csrc/gnx_chain_plan.h: chain_wide_cut): the
issue's cases of that class stay, outside the mask.  Tiles: a wave owns 32 rows, the edge function [64, 64, 3] runs four waves per workgroup (a tile of 128 rows)."""
import ctypes as C

import numpy as np
import pytest

from oracle import gn_oracle as O
from tests import test_gpu_chain as TC
from tests import util as U
from tests.test_gpu_chain_narrow import Call, _adjs, gn  # noqa: F401  (gn: the module's fixture)
from tests.test_gpu_chain_wave import same

pytestmark = pytest.mark.gpu
W64 = ((10, 5, 0), [64, 64, 3], [64, 4], [16, 5], (1, 2, 0), None, 3)
# (in_dims, edge, node, graph widths, hidden activations, last activations, the mask)
WIDTHS = [
    ((10, 5, 1), [33, 3], [8, 4], [6, 5], (1, 2, 0), None, 1),                                   # k_in 21, one column past a 32-block
    W64,
    ((10, 5, 3), [40, "ln", 65, 1], [128, 4], [5], (4, 3, 1), None, 0),                          # a Dense beyond 64: the class cut after measurement
    ((10, 5, 3), ["ln", 48, 48], ["ln_sqrt", 40, 4], [64, 8], (2, 1, 3), None, 7),               # LayerNorm first: on the gathered row / on input rows
    ((32, 32, 32), [128, 128, 128], [16], [], (1, 1, 1), None, 0),                                # k_in 128, the cut class; K_n = 192: outside by width
    ((3, 2, 1), [40, "ln_sqrt", 6], [36, 36], [33, "ln", 2], (3, 4, 2), (4, 2, 3), 7),           # last-layer activations, both eps modes
]


def call(gn, adjs, case, R=1, seed=0):
    in_dims, ew, nw, gw, acts, last, _ = case
    c = Call(gn, adjs, O.make_chain_block_params(np.random.default_rng(50 + seed), in_dims, ew, nw, gw, acts=acts, last_acts=last), R, seed)
    for ch, name in ((c.cp.edgefn, "edge"), (c.cp.nodefn, "node"), (c.cp.graphfn, "graph")):  # (the Python LayerNorm has the default mode only)
        for i, layer in enumerate(c.p[name]):
            if isinstance(layer[0], str) and layer[0] == O.LN_SQRT_EPS:
                ch.layers[i].kind = c.L.LAYER_LAYERNORM | c.L.LAYER_LN_SQRT_EPS
    return c


def wide(c, fill=0xA5):
    """the wide entry on a workspace of exactly the queried size, filled with `fill`; the outputs start as NaN"""
    import torch
    nbytes = c.lib.gnx_chain_block_forward_wide_workspace_bytes(c.g._h, C.byref(c.cp), c.R)
    assert nbytes > 0, c.lib.gnx_last_error()
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=c.g.device)
    outs = c.outputs()
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = c.lib.gnx_chain_block_forward_wide(c.g._h, C.byref(c.cp), *map(ptr, c.xt), c.R, *map(ptr, outs), ws.data_ptr(), nbytes, 0,
                                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, c.lib.gnx_last_error()
    return outs


def verify(c, mask, what):
    import torch
    assert c.lib.gnx_chain_block_forward_wide_applies(c.g._h, C.byref(c.cp), c.R) == mask, what
    a, b, narrow = wide(c, 0x00), wide(c, 0xA5), c.run()
    torch.cuda.synchronize()
    assert all(t is None or not bool(torch.isnan(t).any()) for t in a), f"{what}: an output keeps NaN"
    assert all(same(u, v) for u, v in zip(a, b)), f"{what}: the bytes depend on what the workspace held"
    c.check(a, what)
    for t in range(3):  # (a function behind one of the mask reads that one's output: within the bar above, not the narrow entry's bytes)
        if not mask & ((2 << t) - 1):
            assert same(a[t], narrow[t]), f"{what}: function {t} is outside the mask and not the narrow entry's bytes"
    return a


@pytest.mark.parametrize("graphs", [5, 1])
@pytest.mark.parametrize("i", range(len(WIDTHS)), ids=[str(c[1:4]) for c in WIDTHS])
def test_widths(gn, i, graphs):
    rng = np.random.default_rng(100 + i)
    verify(call(gn, _adjs(rng) if graphs == 5 else _adjs(rng, [40]), WIDTHS[i], seed=i), WIDTHS[i][6], str(WIDTHS[i][:4]))


@pytest.mark.parametrize("edges", [127, 128, 129])
def test_row_tails(gn, edges):
    a = np.zeros(400, dtype=np.int64)
    a[np.random.default_rng(edges).permutation(400)[:edges]] = 1
    c = call(gn, [a.reshape(20, 20)], W64)
    assert c.g.n_edges == edges
    verify(c, 3, f"{edges} edges")


def test_a_graph_without_edges(gn):
    adjs = _adjs(np.random.default_rng(7))
    adjs[3][:] = 0
    verify(call(gn, adjs, W64), 3, "graph without edges")


@pytest.mark.parametrize("case, sizes", [
    (((10, 5, 3), [16, 3], [64, "ln", 4], [6, 5], (1, 2, 0), None, 2), None),      # a narrow edge function, a wide node function
    (((10, 5, 3), [64, 3], [8, 4], [40, 5], (1, 2, 0), None, 5), [30, 12]),        # wide edge, narrow node, wide graph function on G = 2 rows
    (((10, 5, 3), [40], [], [], (1, 2, 0), None, 0), None),                        # one layer: outside the rule
    (((10, 5, 3), [129, 3], [8, 4], [], (1, 2, 0), None, 0), None),                # width 129: outside the rule
], ids=["narrow-edge+wide-node", "wide-edge+narrow-node+wide-graph", "one-layer", "width-129"])
def test_mixed_masks(gn, case, sizes):
    verify(call(gn, _adjs(np.random.default_rng(8), sizes), case), case[6], str(case[:4]))


def test_replicas(gn):
    verify(call(gn, _adjs(np.random.default_rng(9), [31]), W64, R=3), 3, "R = 3")


def test_python_switch(gn, monkeypatch):
    """GNBlock(..., wide_chain=True): the forward is the entry's bytes, off it is gnx_chain_block_forward's; backward() through the switch against
    float64 torch autograd of the restatement (tests/test_gpu_chain.py's case and bar)"""
    import torch
    rng = np.random.default_rng(10)
    c = call(gn, _adjs(rng), ((10, 5, 3), [64, "ln", 64, 3], [8, 4], [40, 5], (1, 2, 0), None, 5))
    want, generic = wide(c), c.run(narrow=False)
    x = U.to_nt(gn, c.g, *c.x)
    assert c.blk.wide_chain is False and gn.GNBlock((3, 2, 1), (1, 1, 1), device="cpu", wide_chain=True).wide_chain is True
    for switch, ref in ((False, generic), (True, want)):
        c.blk.wide_chain = switch
        with torch.no_grad():
            y = c.blk(x)
        torch.cuda.synchronize()
        assert all(same(got.permute(2, 1, 0).contiguous(), w) for got, w in zip((y.ef, y.nf, y.gf), ref)), switch
    made, plain = [], TC._block

    def switched(gn_, p):
        made.append(plain(gn_, p))
        made[-1].wide_chain = True
        return made[-1]

    monkeypatch.setattr(TC, "_block", switched)
    cs = [U.er_csc(rng, int(n), int(0.2 * n * n) + 1) for n in (25, 9, 17)]
    g = gn.GNGraphBatch.from_csc([k[0] for k in cs], [k[1] for k in cs], [25, 9, 17])
    assert TC.chain_block_backward_case(gn, g, rng, (10, 5, 3), [64, "ln", 3], [8, 4], ["ln", 40, 5], (2, 3, 4))
    assert len(made) == 1 and made[0].wide_chain is True
