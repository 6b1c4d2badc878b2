"""gnx_chain_block_forward_wave_typed: the wave-per-tile Chain block on bfloat16 features (csrc/gnx_chain_wave_bf16.hip).  Every comparison is
exact.  Inside the rule the bf16 outputs are the bits of to_bf16(gnx_chain_block_forward_wave on the exactly widened inputs) and the workspace
is no larger than that entry's; outside it they are gnx_chain_block_forward_typed(narrow = 1)'s bytes on its workspace size.  The flat store —
a tile's ef' / nf' as one run of packed dwords with 16-bit odd ends — runs on exactly sized, 4-byte-aligned outputs in a sentinel arena."""
import ctypes as C

import numpy as np
import pytest

from oracle import gn_oracle as O
from tests import arena as AR
from tests import test_gpu_chain_narrow as CN
from tests import test_gpu_chain_typed as T
from tests import test_gpu_chain_wave as GW
from tests.test_gpu_chain_typed import gn  # noqa: F401  (the module's fixture)
from tests.test_gpu_memory_contract import _chain_params, _decl, _decl_chains, _decl_outputs

pytestmark = pytest.mark.gpu


class WCall(T.TCall):
    def h(self, cp=None):
        return self.g._h, C.byref(self.cp if cp is None else cp)

    def wapplies(self):
        return self.lib.gnx_chain_block_forward_wave_typed_applies(*self.h(), self.R, self.L.ELEM_BF16)

    def wquery(self):
        return self.lib.gnx_chain_block_forward_wave_typed_workspace_bytes(*self.h(), self.R, self.L.ELEM_BF16)

    def wrun(self, ins, outs, ws, nbytes, cp=None):
        import torch
        rc = self.lib.gnx_chain_block_forward_wave_typed(*self.h(cp), self.L.ELEM_BF16, *ins, self.R, *outs, ws, nbytes, 0, torch.cuda.current_stream().cuda_stream)
        assert nbytes > 0 and rc == 0, self.lib.gnx_last_error()

    def direct(self):
        """the entry on torch tensors, the workspace exactly the query's"""
        import torch
        outs, ws = self.touts(), torch.full((self.wquery(),), 0xA5, dtype=torch.uint8, device=self.g.device)
        ptr = lambda t: None if t is None else t.data_ptr()
        self.wrun(map(ptr, self.xb), map(ptr, outs), ws.data_ptr(), ws.numel())
        return outs

    def want(self, inside):
        """inside the rule: to_bf16(the fp32 wave entry on the widened inputs); outside: the typed entry's bytes; and the workspace bound"""
        import torch
        assert self.wapplies() == int(inside)
        if not inside:
            assert self.wquery() == self.tquery(1)
            return self.trun(1)
        assert 0 < self.wquery() <= self.lib.gnx_chain_block_forward_wave_workspace_bytes(*self.h(), self.R)
        return [None if t is None else t.to(torch.bfloat16) for t in GW.wave(self)]


def same(got, want, what):
    import torch
    torch.cuda.synchronize()
    for n, u, v in zip(("ef", "nf", "gf"), got, want):
        assert (u is None) == (v is None) and (u is None or not bool(torch.isnan(v.float()).any())), (what, n)
        bad = 0 if u is None else int((T._bits(u) != T._bits(v)).sum())
        assert bad == 0, f"{what} {n}: {bad} of {u.numel()} elements differ"


@pytest.mark.parametrize("graphs", [5, 1])
@pytest.mark.parametrize("i", range(len(T.WIDTH_CASES)), ids=[str(c[:4]) for c in T.WIDTH_CASES])
def test_widths(gn, i, graphs):
    rng = np.random.default_rng(100 + i)
    case = T.WIDTH_CASES[i]
    c = WCall(gn, CN._adjs(rng) if graphs == 5 else CN._adjs(rng, [40]), CN._params(rng, case), seed=i)
    inside = bool(case[2]) and (graphs == 1 or not GW.wide(case))  # a node function; register width 32 on one graph only (every LDS term is far)
    same(c.direct(), c.want(inside), f"{case[:4]} graphs={graphs}")


def _flat_case(kind, rng):
    """(adjacency matrices, parameters, R, inside the rule)"""
    if kind == "odd-replicas-3":  # odd de, dn, oe, on, E and N: the runs of replicas 1 and 2 start on odd elements
        case, adjs, R = T._structural("odd-everything-replicas-3", rng)
        return adjs, CN._params(rng, case), R, True
    if kind == "oe1-on31":  # a slice of 128 x 1 floats for ef', of 64 x 31 for the nf' rows
        return CN._adjs(rng, [40]), O.make_chain_block_params(rng, (3, 2, 0), [8, 1], [31], [4]), 1, True
    adjs, R, inside = GW._tiles(kind, rng)
    return adjs, CN._params(rng, T.WIDTH_CASES[2] if len(adjs) == 1 else GW.W16), R, inside


@pytest.mark.parametrize("kind", ["odd-replicas-3", "empty-columns", "node-and-edge-cap", "degree-cap", "degree-cap+1", "oe1-on31"])
def test_flat_store_in_a_sentinel_arena(gn, kind):
    import torch
    adjs, p, R, inside = _flat_case(kind, np.random.default_rng(200))
    src = WCall(gn, adjs, p, R)
    want = src.want(inside)
    a = AR.Arena("cuda", skew=lambda c: 0 if c.kind == AR.WORKSPACE else 4)
    _decl_chains(a, p)
    ins = [_decl(a, n, v) for n, v in zip(("ef", "nf", "gf"), src.xb)]
    outs = _decl_outputs(a, "", R, src.rows, src.outw, torch.bfloat16)
    ws = a.workspace("ws", src.wquery())
    a.build(ws_fill=0x00)
    assert all(a.ptr(n) % 8 == 4 for n in ins + outs if n is not None)
    bits, keep = [], []
    for fill in (0x00, 0xFF):
        a.refill(fill)
        src.wrun(map(a.ptr, ins), map(a.ptr, outs), a.ptr(ws), a.nbytes(ws), _chain_params(gn, a, p, keep))
        torch.cuda.synchronize()
        a.check(f"{kind} workspace {fill:#04x}")  # nothing outside an output is written, every output element is
        bits.append(a.output_bits())
    assert all(torch.equal(bits[0][k], bits[1][k]) for k in bits[0]), "the outputs depend on what the workspace held"
    same([None if n is None else a.view(n) for n in outs], want, kind)


def test_python_switch(gn):
    """GNBlock(..., wave_chain=True, bf16_chain=True) on a bf16 batch returns the direct entry's bytes"""
    import torch
    rng = np.random.default_rng(600)
    c = WCall(gn, CN._adjs(rng), CN._params(rng, GW.W16))
    assert c.wapplies() == 1
    want = c.direct()
    c.blk.wave_chain = c.blk.bf16_chain = True
    with torch.no_grad():
        y = c.blk(T._nt(gn, c, c.xb))
    same([t.permute(2, 1, 0).contiguous() for t in (y.ef, y.nf, y.gf)], want, "python")
