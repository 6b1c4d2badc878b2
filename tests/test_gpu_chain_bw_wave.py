"""gnx_chain_block_backward_wave: the pullback of a Chain block with the node and the edge function in one wave-per-tile kernel
(csrc/gnx_chain_bw_wave.hip).  Inside the rule: `_applies` is 1, every gradient meets the bar of tests/test_gpu_chain_bw_narrow.py against float64
autograd (max|got - ref| <= max(4 max|yardstick - ref|, 1e-5 max(1, max|ref|)) per tensor), NaN-filled outputs are fully written and the bytes
do not depend on what the workspace held.  Outside it: `_applies` is 0 and every output is byte for byte gnx_chain_block_backward_narrow's.  The
forward's cut (register width 32 on several graphs) and the pullback's own (register width 8 on several graphs; csrc/gnx_chain_plan.h:
chain_bw_wave_cut, with its figures) apply, so every width case runs on five graphs and on one."""
import numpy as np
import pytest

from oracle import gn_oracle as O
from tests import test_gpu_chain_bw_narrow as BW
from tests import test_gpu_chain_wave as TW
from tests.test_gpu_chain_narrow import _adjs, gn  # noqa: F401  (gn: the module's fixture)

pytestmark = pytest.mark.gpu
# (in_dims, edge, node, graph, hidden activations, last-layer activations)
CASES = [
    ((2, 2, 1), [8, 8, 1], [3], [2], None, None),                                # register width 8; relu and tanh hidden layers
    TW.W16 + (None,),                                                            # 16; LayerNorms between layers and last; gelu, sigmoid, relu hidden
    ((10, 5, 0), [16, 3], [8, 4], [6, 5], (1, 2, 0), None),                      # 32 (K_e = 20); dg = 0
    ((4, 3, 2), ["ln", 8, 5], [6], [4], None, ("gelu", "tanh", "sigmoid")),      # 16; LayerNorm first in the edge function; activations on the last layers
    ((0, 4, 2), [8, 5], [5], [], None, None),                                    # 16; no graph function, de = 0
]


def narrow8(case):
    """every input and layer width of the edge and the node function at most 8: the kernel's 8-wide instantiation"""
    (de, dn, dg), ew, nw = case[:3]
    num = lambda ws: [w for w in ws if w != "ln"]
    ke = de + 2 * dn + dg
    return max([ke, (num(ew) or [ke])[-1] + dn + dg] + num(ew) + num(nw)) <= 8


class WaveLib:
    """the library with the wave pullback's trio under the narrow trio's names: BwCall.mask / .query / .run(True) then reach the new entry"""

    def __init__(self, lib):
        self.lib = lib

    def __getattr__(self, name):
        return getattr(self.lib, name.replace("backward_narrow", "backward_wave") if name.startswith("gnx_chain_block_backward_narrow") else name)


def make(gn, adjs, case, R=1, seed=0):
    """tests.test_gpu_chain_bw_narrow.make with the case's last-layer activations"""
    if case[5] is None:
        return BW.make(gn, adjs, case[:5], R, seed)
    acts = {} if case[4] is None else dict(acts=case[4])
    last = tuple(getattr(O, "ACT_" + a.upper()) for a in case[5])
    for attempt in range(20):
        p = O.make_chain_block_params(np.random.default_rng(13000 + 101 * seed + 1000 * attempt), *case[:4], last_acts=last, **acts)
        c = BW.BwCall(gn, adjs, p, R, seed + 1000 * attempt)
        if c.ok:
            return c
    pytest.fail("no kink-free draw in 20 attempts")


def same(a, b):
    import torch
    return sorted(a) == sorted(b) and all(torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)) for n in a)


def held(c, got, yard, what):
    """the bar of tests/test_gpu_chain_bw_narrow.py with `yard` (another entry's gradients) as the yardstick"""
    for n, r in c.ref.items():
        if n in got and r.size:
            en = float(np.max(np.abs(got[n].cpu().numpy().astype(np.float64) - r)))
            ey = float(np.max(np.abs(yard[n].cpu().numpy().astype(np.float64) - r)))
            bound = max(4.0 * ey, 1e-5 * max(1.0, float(np.abs(r).max())))
            print(f"chain bw wave {what} {n}: err {en:.3e}, yardstick err {ey:.3e}, bound {bound:.3e}")
            assert np.isfinite(en) and en <= bound, (what, n, en, ey, bound)


def verify(c, inside, what, skip=()):
    """`_applies`, fully written outputs, bytes independent of the workspace; inside the rule the bar against the narrow and the generic entry,
    outside the narrow entry's bytes.  Returns the wave entry's gradients."""
    import torch
    lib, c.lib = c.lib, WaveLib(c.lib)
    try:
        assert c.mask() == int(inside), (what, c.mask())
        a, b = c.run(True, fill=0x00, skip=skip), c.run(True, fill=0xA5, skip=skip)
    finally:
        c.lib = lib
    narrow, generic = c.run(True, skip=skip), c.run(False, skip=skip)
    torch.cuda.synchronize()
    assert all(not bool(torch.isnan(t).any()) for t in a.values()), f"{what}: an output keeps NaN"
    assert same(a, b), f"{what}: the bytes depend on what the workspace held"
    if inside:
        held(c, a, narrow, what + " / narrow")
        held(c, a, generic, what + " / generic")
    else:
        assert same(a, narrow), f"{what}: outside the rule the gradients are not the narrow entry's bytes"
    return a


@pytest.mark.parametrize("graphs", [5, 1])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[str(c[:4]) for c in CASES])
def test_against_float64_autograd(gn, i, graphs):
    rng = np.random.default_rng(100 + i)
    case = CASES[i]
    c = make(gn, _adjs(rng) if graphs == 5 else _adjs(rng, [40]), case, seed=i)
    verify(c, inside=graphs == 1 or not (TW.wide(case) or narrow8(case)), what=str(case[:4]))


@pytest.mark.parametrize("kind", ["node-and-edge-cap", "empty-columns", "degree-cap", "degree-cap+1", "replicas-3"])
def test_tiles(gn, kind):
    rng = np.random.default_rng(200)
    adjs, R, inside = TW._tiles(kind, rng)
    c = make(gn, adjs, CASES[2] if len(adjs) == 1 else CASES[1], R, seed=20)  # (one graph: the 32-wide instantiation)
    if kind.startswith("degree-cap"):
        assert c.g.max_in_degree == TW.CAP + (not inside)
    if kind == "node-and-edge-cap":  # a tile of 64 one-in-edge nodes, tiles of two edge chunks with a partly live second one
        assert c.g.n_edges > 64 + TW.CAP
    verify(c, inside, kind)


def test_null_outputs(gn):
    """d_nf and one layer's parameter-gradient pair not wanted, no upstream gradient of gf': the narrow entry under the same NULLs is the
    reference (no float64 gradients exist for this cotangent), at the absolute term of the bar: 1e-5 max(1, max|narrow|)"""
    import torch
    rng = np.random.default_rng(300)
    c = make(gn, _adjs(rng), CASES[1], seed=30)
    c.cot[2] = None
    skip = ("d_nf", "edge1.dW", "edge1.db")
    lib, c.lib = c.lib, WaveLib(c.lib)
    try:
        assert c.mask() == 1
        a, b = c.run(True, fill=0x00, skip=skip), c.run(True, fill=0xA5, skip=skip)
    finally:
        c.lib = lib
    narrow = c.run(True, skip=skip)
    torch.cuda.synchronize()
    assert same(a, b) and not set(skip) & set(a)
    for n in a:
        err, scale = float((a[n] - narrow[n]).abs().max()), max(1.0, float(narrow[n].abs().max()))
        print(f"chain bw wave NULLs {n}: |wave - narrow| {err:.3e}, scale {scale:.3e}")
        assert np.isfinite(err) and err <= 1e-5 * scale, (n, err, scale)


def test_python_switch(gn):
    """GNBlock(..., wave_chain_backward=True) under torch.autograd gives the entry's bytes"""
    import torch
    rng = np.random.default_rng(400)
    c = make(gn, _adjs(rng), CASES[1], seed=40)
    want = verify(c, True, "switch")
    blk = c.blk
    assert blk.wave_chain_backward is False and gn.GNBlock((3, 2, 1), (1, 1, 1), device="cpu", wave_chain_backward=True).wave_chain_backward is True
    blk.wave_chain_backward = blk.narrow_chain_backward = True  # (the wave switch wins)
    leaves = [(l.weight.requires_grad_(True), l.bias.requires_grad_(True)) for ch in (blk.edgefn, blk.nodefn, blk.graphfn) for l in ch.layers]
    xt = [t.clone().requires_grad_(True) for t in c.xt]
    y = blk(gn.NT(c.g, *(t.permute(2, 1, 0) for t in xt)))
    sum((o.permute(2, 1, 0) * ct).sum() for o, ct in zip((y.ef, y.nf, y.gf), c.cot)).backward()
    torch.cuda.synchronize()
    eq = lambda u, v: torch.equal(u.contiguous().view(torch.int32), v.contiguous().view(torch.int32))
    assert all(eq(t.grad, want[n]) for n, t in zip(("d_ef", "d_nf", "d_gf"), xt))
    names = [f"{name}{i}" for name in ("edge", "node", "graph") for i in range(len(c.p[name]))]
    for n, (w, b) in zip(names, leaves):
        assert eq(w.grad if w.grad.dim() == 1 else w.grad.t(), want[n + ".dW"]) and eq(b.grad, want[n + ".db"]), n
