"""gnx_chain_block_backward_wide: the pullback of a Chain block with every update function at matrix-core widths in one persistent kernel
(csrc/gnx_chain_bw_wide.hip).  Per case: `_applies` is the expected mask, NaN-filled outputs are fully written, the bytes do not depend on what
the workspace held, and every gradient meets the bar of tests/test_gpu_chain_bw_narrow.py against float64 autograd with the generic
gnx_chain_block_backward as yardstick: max|got - ref| <= max(4 max|yardstick - ref|, 1e-5 max(1, max|ref|)) per tensor.  With mask 0 every
output is byte for byte gnx_chain_block_backward_narrow's."""
import numpy as np
import pytest

from tests import test_gpu_chain_bw_wave as WV
from tests.test_gpu_chain_narrow import _adjs, gn  # noqa: F401  (gn: the module's fixture)

pytestmark = pytest.mark.gpu
# (in_dims, edge, node, graph, hidden activations, last-layer activations), the expected mask
CASES = [
    (((10, 5, 0), [64, 64, 3], [64, 4], [16, 5], None, None), 3),                      # wide edge and node, narrow graph, dg = 0
    (((10, 5, 3), ["ln", 48, 48], ["ln_sqrt", 40, 4], [64, 8], None, None), 7),        # LayerNorm first on the gathered row and on input rows
    (((10, 5, 3), [40, 48, 3], [40, 24, 20, 4], [40, 8], (4, 2, 3), ("gelu", "tanh", "sigmoid")), 7),  # gelu, tanh, sigmoid hidden; activated last
    (((10, 5, 3), [16, 3], [64, "ln", 4], [6, 5], None, None), 2),                     # a narrow edge function beside a wide node function
    (((10, 5, 3), [40, "ln", 65, 1], [128, 4], [5], None, None), 0),                   # the class chain_wide_cut cuts: the narrow entry's call
]


class WideLib(WV.WaveLib):
    """the library with the wide pullback's trio under the narrow trio's names"""

    def __getattr__(self, name):
        return getattr(self.lib, name.replace("backward_narrow", "backward_wide") if name.startswith("gnx_chain_block_backward_narrow") else name)


def full(n, e):
    """one graph of n nodes whose first e entries of the adjacency matrix (row-major) are edges"""
    a = np.zeros(n * n, dtype=np.int64)
    a[:e] = 1
    return [a.reshape(n, n)]


def verify(c, mask, what, skip=()):
    import torch
    lib, c.lib = c.lib, WideLib(c.lib)
    try:
        assert c.mask() == mask, (what, c.mask())
        a, b = c.run(True, fill=0x00, skip=skip), c.run(True, fill=0xA5, skip=skip)
    finally:
        c.lib = lib
    narrow, generic = c.run(True, skip=skip), c.run(False, skip=skip)
    torch.cuda.synchronize()
    assert all(not bool(torch.isnan(t).any()) for t in a.values()), f"{what}: an output keeps NaN"
    assert WV.same(a, b), f"{what}: the bytes depend on what the workspace held"
    if mask:
        WV.held(c, a, generic, what)
    else:
        assert WV.same(a, narrow), f"{what}: with mask 0 the gradients are not the narrow entry's bytes"
    return a


@pytest.mark.parametrize("i", range(len(CASES)), ids=[str(c[0][:4]) for c in CASES])
def test_against_float64_autograd(gn, i):
    case, mask = CASES[i]
    verify(WV.make(gn, _adjs(np.random.default_rng(100 + i)), case, seed=i), mask, str(case[:4]))


# 512: kChainBwWideGrid (csrc/gnx_chain_plan.h), the persistent grid's cap; the first case's edge function runs two waves of 32 rows per tile,
# so 512 * 64 + 32 edges give one workgroup two tiles, the last of them with one live and one idle wave
SHAPES = {"E=1": (full(2, 1), 1), "E=33": (full(6, 33), 1), "tile+1": (full(9, 65), 1), "replicas-3": (_adjs(np.random.default_rng(201), [30]), 3),
          "edgeless-graph": ([np.zeros((4, 4), dtype=np.int64)], 1), "grid-cap": (full(182, 512 * 64 + 32), 1)}


@pytest.mark.parametrize("kind", list(SHAPES))
def test_shapes(gn, kind):
    rng = np.random.default_rng(200)
    adjs, R = SHAPES[kind]
    if kind == "edgeless-graph":
        adjs = _adjs(rng)[:2] + adjs + _adjs(rng)[:1]
    case = CASES[0][0]
    if kind == "grid-cap":  # (tanh for relu: among 32800 x 64 relu pre-activations every draw has one within fp32 rounding of the kink)
        case = case[:4] + ((2, 3, 0), None)
    c = WV.make(gn, adjs, case, R, seed=20)
    if kind == "grid-cap":
        assert c.g.n_edges == 512 * 64 + 32
    verify(c, 3, kind)


@pytest.mark.parametrize("skip", [("d_nf",), "grads"])
def test_null_outputs(gn, skip):
    """d_nf not wanted / no parameter gradient wanted (grads = NULL is every pair NULL for the kernels: no partial rows, no finishers)"""
    c = WV.make(gn, _adjs(np.random.default_rng(300)), CASES[1][0], seed=30)
    if skip == "grads":
        skip = tuple(n for n in c.ref if "." in n)
    got = verify(c, 7, "NULLs", skip)
    assert not set(skip) & set(got)


def test_python_switch(gn):
    """GNBlock(..., wide_chain_backward=True) under torch.autograd gives the entry's bytes; with the switch off the generic entry's"""
    import torch
    c = WV.make(gn, _adjs(np.random.default_rng(400)), CASES[1][0], seed=40)
    want, off = verify(c, 7, "switch"), c.run(False)
    blk = c.blk
    names = [f"{name}{i}" for name in ("edge", "node", "graph") for i in range(len(c.p[name]))]
    eq = lambda u, v: torch.equal(u.contiguous().view(torch.int32), v.contiguous().view(torch.int32))
    leaves = [(l.weight.requires_grad_(True), l.bias.requires_grad_(True)) for ch in (blk.edgefn, blk.nodefn, blk.graphfn) for l in ch.layers]
    for on, ref in ((True, want), (False, off)):
        blk.wide_chain_backward = on
        for t in (q for wb in leaves for q in wb):
            t.grad = None
        xt = [t.clone().requires_grad_(True) for t in c.xt]
        y = blk(gn.NT(c.g, *(t.permute(2, 1, 0) for t in xt)))
        sum((o.permute(2, 1, 0) * ct).sum() for o, ct in zip((y.ef, y.nf, y.gf), c.cot)).backward()
        torch.cuda.synchronize()
        assert all(eq(t.grad, ref[n]) for n, t in zip(("d_ef", "d_nf", "d_gf"), xt)), on
        for n, (w, b) in zip(names, leaves):
            assert eq(w.grad if w.grad.dim() == 1 else w.grad.t(), ref[n + ".dW"]) and eq(b.grad, ref[n + ".db"]), (on, n)
