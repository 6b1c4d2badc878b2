"""gnx_chain_block_forward_wide_typed: Chain blocks at matrix-core widths on bfloat16 features (csrc/gnx_chain_wide_bf16.hip).  Every comparison
is exact: in every form the bf16 outputs are the bits of to_bf16(gnx_chain_block_forward_wide on the exactly widened inputs).  Derived, not
measured: the gathered bf16 row is its own high plane, so three of x6_mma's six instructions add exact zeros to an accumulator that starts at +0
and the other three run in the same order; everything behind the first Dense is one text, and later functions read unrounded fp32 rows in both
forms.  Also: `_applies`, NaN-filled outputs fully written, independence of what an exactly sized workspace held, the workspace bounds, and the
flat bf16 store on exactly sized 4-byte-aligned buffers in a sentinel arena.  A wave owns 32 rows; [64, 64, 3] runs four waves per workgroup."""
import ctypes as C

import numpy as np
import pytest

from oracle import gn_oracle as O
from tests import arena as AR
from tests import test_gpu_chain_typed as T
from tests import test_gpu_chain_wide as GW
from tests.test_gpu_chain_narrow import _adjs
from tests.test_gpu_chain_typed import gn  # noqa: F401  (the module's fixture)
from tests.test_gpu_memory_contract import _chain_params, _decl, _decl_chains, _decl_outputs

pytestmark = pytest.mark.gpu


class WCall(T.TCall):
    def h(self, cp=None):
        return self.g._h, C.byref(self.cp if cp is None else cp)

    def wapplies(self, elem=None):
        return self.lib.gnx_chain_block_forward_wide_typed_applies(*self.h(), self.R, self.L.ELEM_BF16 if elem is None else elem)

    def wquery(self, elem=None):
        return self.lib.gnx_chain_block_forward_wide_typed_workspace_bytes(*self.h(), self.R, self.L.ELEM_BF16 if elem is None else elem)

    def wrun(self, ins, outs, ws, nbytes, cp=None, elem=None):
        import torch
        rc = self.lib.gnx_chain_block_forward_wide_typed(*self.h(cp), self.L.ELEM_BF16 if elem is None else elem, *ins, self.R, *outs, ws, nbytes, 0,
                                                         torch.cuda.current_stream().cuda_stream)
        assert nbytes > 0 and rc == 0, self.lib.gnx_last_error()

    def direct(self, fill=0xA5, elem=None):
        """the entry on torch tensors, the workspace exactly the query's and filled with `fill`; the outputs start as NaN"""
        import torch
        bf16 = elem in (None, self.L.ELEM_BF16)
        outs, ws = self.touts(None if bf16 else torch.float32), torch.full((self.wquery(elem),), fill, dtype=torch.uint8, device=self.g.device)
        ptr = lambda t: None if t is None else t.data_ptr()
        self.wrun(map(ptr, self.xb if bf16 else self.xt), map(ptr, outs), ws.data_ptr(), ws.numel(), elem=elem)
        return outs

    def want(self):
        """to_bf16(gnx_chain_block_forward_wide on the widened inputs)"""
        import torch
        ref = GW.wide(self)
        torch.cuda.synchronize()
        return [None if t is None else t.to(torch.bfloat16) for t in ref]


def make(gn, adjs, case, R=1, seed=0):
    """GW.call on bfloat16 features"""
    in_dims, ew, nw, gw, acts, last, _ = case
    c = WCall(gn, adjs, O.make_chain_block_params(np.random.default_rng(50 + seed), in_dims, ew, nw, gw, acts=acts, last_acts=last), R, seed)
    for ch, name in ((c.cp.edgefn, "edge"), (c.cp.nodefn, "node"), (c.cp.graphfn, "graph")):  # (the Python LayerNorm has the default mode only)
        for i, layer in enumerate(c.p[name]):
            if isinstance(layer[0], str) and layer[0] == O.LN_SQRT_EPS:
                ch.layers[i].kind = c.L.LAYER_LAYERNORM | c.L.LAYER_LN_SQRT_EPS
    return c


def same(got, want, what):
    import torch
    torch.cuda.synchronize()
    for n, u, v in zip(("ef", "nf", "gf"), got, want):
        assert (u is None) == (v is None) and (u is None or not bool(torch.isnan(v.float()).any())), (what, n)
        bad = 0 if u is None else int((T._bits(u) != T._bits(v)).sum())
        assert bad == 0, f"{what} {n}: {bad} of {u.numel()} elements differ"


def verify(c, mask, what):
    """mask: gnx_chain_block_forward_wide_applies' for the block.  Native: the mask is non-zero and every function that runs is in it or in the
    narrow mask — then _applies is the mask; staged (a generic function) and mask 0 (the typed entry with narrow = 1): _applies is 0"""
    import torch
    runs = [t for t in range(3) if c.outw[t] > 0 and c.rows[t] > 0]
    native = mask != 0 and all((mask | c.mask()) >> t & 1 for t in runs)
    assert c.lib.gnx_chain_block_forward_wide_applies(*c.h(), c.R) == mask, what
    assert c.wapplies() == (mask if native else 0), what
    a, b = c.direct(0x00), c.direct(0xA5)
    torch.cuda.synchronize()
    assert all(t is None or not bool(torch.isnan(t.float()).any()) for t in a), f"{what}: an output keeps NaN"
    same(a, b, what + ": the bytes depend on what the workspace held")
    same(a, c.want(), what)
    if mask == 0:
        assert c.wquery() == c.tquery(1), what
        same(a, c.trun(1), what + ": not the typed entry's bytes")
    if native:  # the fp32 wide layout and the carves of chain_native_counts behind it: ef' for node / graph, nf' and the widened gf for graph
        oe, on, og = c.outw
        E, N, G = c.rows
        counts = (E * oe if on or og else 0, N * on if og else 0, G * c.p["in_dims"][2] if og else 0)
        carves = sum(-(-4 * c.R * n // 256) * 256 for n in counts)
        fp32 = c.lib.gnx_chain_block_forward_wide_workspace_bytes(*c.h(), c.R)
        assert 0 < c.wquery() <= fp32 + carves and c.wquery() < c.tquery(1), (what, c.wquery(), fp32, carves, c.tquery(1))
    return a


@pytest.mark.parametrize("graphs", [5, 1])
@pytest.mark.parametrize("i", range(len(GW.WIDTHS)), ids=[str(c[1:4]) for c in GW.WIDTHS])
def test_widths(gn, i, graphs):
    rng = np.random.default_rng(100 + i)
    case = GW.WIDTHS[i]
    verify(make(gn, _adjs(rng) if graphs == 5 else _adjs(rng, [40]), case, seed=i), case[6], f"{case[:4]} graphs={graphs}")


@pytest.mark.parametrize("edges", [127, 128, 129])
def test_row_tails(gn, edges):
    a = np.zeros(400, dtype=np.int64)
    a[np.random.default_rng(edges).permutation(400)[:edges]] = 1
    c = make(gn, [a.reshape(20, 20)], GW.W64)
    assert c.g.n_edges == edges
    verify(c, 3, f"{edges} edges")


def test_a_graph_without_edges(gn):
    adjs = _adjs(np.random.default_rng(7))
    adjs[3][:] = 0
    verify(make(gn, adjs, GW.W64), 3, "graph without edges")


@pytest.mark.parametrize("case, sizes", [
    (((10, 5, 3), [16, 3], [64, "ln", 4], [6, 5], (1, 2, 0), None, 2), None),      # a narrow edge function, a wide node function
    (((10, 5, 3), [64, 3], [8, 4], [40, 5], (1, 2, 0), None, 5), [30, 12]),        # wide edge, narrow node, wide graph function on G = 2 rows
    (((10, 5, 3), [64, 3], [40], [], (1, 2, 0), None, 1), None),                   # a generic node function behind a wide edge function: staged
], ids=["narrow-edge+wide-node", "wide-edge+narrow-node+wide-graph", "staged"])
def test_mixed_masks(gn, case, sizes):
    c = make(gn, _adjs(np.random.default_rng(8), sizes), case)
    verify(c, case[6], str(case[:4]))
    assert (c.wapplies() == 0) == (len(case[2]) == 1)


def test_odd_runs_under_replicas_in_a_sentinel_arena(gn):
    """[64, 64, 3] / [64, 5] / [16, 5] on one graph with odd N and E, odd de, dn, dg and R = 3: replicas 1 and 2 of every bf16 tensor start on odd
    elements.  Exactly sized buffers at ptr % 8 == 4: nothing outside an output is written, every output element is"""
    import torch
    case, adjs, R = T._structural("odd-everything-replicas-3", np.random.default_rng(200))
    p = O.make_chain_block_params(np.random.default_rng(201), case[0], [64, 64, 3], [64, 5], [16, 5], acts=(1, 2, 0))
    src = WCall(gn, adjs, p, R)
    assert src.wapplies() == 3 and all((t.shape[1] * t.shape[2]) % 2 == 1 for t in src.xb + src.touts())
    want = src.want()
    a = AR.Arena("cuda", skew=lambda c: 0 if c.kind == AR.WORKSPACE else 4)
    _decl_chains(a, p)
    ins = [_decl(a, n, v) for n, v in zip(("ef", "nf", "gf"), src.xb)]
    outs = _decl_outputs(a, "", R, src.rows, src.outw, torch.bfloat16)
    ws = a.workspace("ws", src.wquery())
    a.build(ws_fill=0x00)
    assert all(a.ptr(n) % 8 == 4 for n in ins + outs)
    bits, keep = [], []
    for fill in (0x00, 0xFF):
        a.refill(fill)
        src.wrun(map(a.ptr, ins), map(a.ptr, outs), a.ptr(ws), a.nbytes(ws), _chain_params(gn, a, p, keep))
        torch.cuda.synchronize()
        a.check(f"workspace {fill:#04x}")
        bits.append(a.output_bits())
    assert all(torch.equal(bits[0][k], bits[1][k]) for k in bits[0]), "the outputs depend on what the workspace held"
    same([a.view(n) for n in outs], want, "arena")


def test_elem_f32_is_the_fp32_wide_entry(gn):
    c = make(gn, _adjs(np.random.default_rng(11)), GW.W64)
    F32 = c.L.ELEM_F32
    assert c.wquery(F32) == c.lib.gnx_chain_block_forward_wide_workspace_bytes(*c.h(), c.R) > 0 and c.wapplies(F32) == 3
    same(c.direct(elem=F32), GW.wide(c), "F32")


def test_python_switch(gn):
    """GNBlock(..., bf16_chain=True, wide_chain=True) on a bf16 batch returns the entry's bytes; with wide_chain off, the typed entry's"""
    import torch
    c = make(gn, _adjs(np.random.default_rng(12)), GW.W64)
    c.blk.bf16_chain = c.blk.narrow_chain = True
    for switch, want in ((True, c.direct()), (False, c.trun(1))):
        c.blk.wide_chain = switch
        with torch.no_grad():
            y = c.blk(T._nt(gn, c, c.xb))
        same([t.permute(2, 1, 0).contiguous() for t in (y.ef, y.nf, y.gf)], want, f"wide_chain={switch}")
