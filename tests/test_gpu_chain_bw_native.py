"""gnx_chain_block_backward_narrow_typed: the pullback of a GNBlock whose update functions are Chains on bfloat16 features, natively — each update
function in one launch of k_chain_mlp_bw_bf16 (csrc/gnx_chain_bw_narrow_bf16.hip) that reads the bf16 rows and upstream gradients and writes the
bf16 d_ef itself, with no edge- or node-sized fp32 copy.  Every comparison is exact: the three input gradients and every parameter gradient are
the bits of gnx_chain_block_backward_typed(narrow = 1) — the staged call, i.e. to_bf16 of the fp32 narrow pullback on the widened tensors — on
the same nine tensors.  Also: `_applies` against the rule restated here, that the native form ran (conversions and launches counted), the
workspace bound, the two identities (GNX_ELEM_F32 is gnx_chain_block_backward_narrow; bf16 outside the rule is the staged call), the memory
contract on exactly sized 4-byte-aligned buffers, stream capture, the Python switch and a seeded sweep.  The batches, width cases and structural
cases are those of tests/test_gpu_chain_typed.py."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

from tests import arena as AR
from tests import util as U
from tests import test_gpu_chain_narrow as CN
from tests import test_gpu_chain_typed as TY
from tests.test_gpu_memory_contract import _chain_params, _decl, _decl_chains, _decl_dense_grad, _dense_grad

pytestmark = pytest.mark.gpu
EXTRA = int(os.environ.get("GNX_FUZZ_EXTRA", "0"))
WIDTH_CASES, STRUCTURAL = TY.WIDTH_CASES, TY.STRUCTURAL
SWEEP = list(range(len(WIDTH_CASES))) + STRUCTURAL
# No class is cut from the native rule (profiles/chain_bw_native.json: the native call is never slower than the staged one beyond its spread), so
# every case whose functions are all inside the narrow pullback's rule is expected native.
NATIVE = [0, 1, 2, 4, 5, 6, 7, 8, "isolated-column", "graph-without-edges", "replicas-2", "replicas-3", "odd-everything-replicas-3"]
STAGED = [3, "partial-workgroup", "edgeless-batch"]  # [32,ln,32,32,7] is outside the pullback's LDS rule (a mixed mask); no edges: no edge launch
# every name a pullback launch may run under (no new one: tests/test_gpu_memory_contract.py covers these)
PROFILE_NAMES = {"bw_chain_fw_e", "bw_chain_fw_n", "bw_delta", "bw_delta_edge", "bw_dw_generic", "bw_dnf", "bw_dgf", "k_bf16_widen", "k_bf16_round"}
# the node and rows forms at register width 32 (the width cases above reach 32 natively in the edge form alone): [32,5] at k_in 9, [24,3] at k_in 12
WIDE_NODE_GRAPH = ((4, 2, 1), [8, 6], [32, 5], [24, 3], (2, 3, 1))
SKIP = {"d_nf", "edge0.dW", "node0.db", "graph0.dW", "graph0.db"}  # test_gpu_chain_typed.py::test_backward_bits' set


@pytest.fixture(scope="module")
def gn():
    import torch
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


class NCall(TY.TCall):
    """TY.TCall with the new entry and its two queries"""

    def bw_mask(self):
        return self.lib.gnx_chain_block_backward_narrow_applies(self.g._h, C.byref(self.cp), self.R)

    def rule(self):
        """include/gnx.h: the edge function has an output and E > 0, and every function with an output and rows is in the pullback's mask"""
        m = self.bw_mask()
        return int(self.outw[0] > 0 and self.rows[0] > 0 and all(m >> t & 1 for t in range(3) if self.outw[t] > 0 and self.rows[t] > 0))

    def napplies(self, elem=None):
        return self.lib.gnx_chain_block_backward_narrow_typed_applies(self.g._h, C.byref(self.cp), self.R, self.L.ELEM_BF16 if elem is None else elem)

    def nquery(self, elem=None):
        return self.lib.gnx_chain_block_backward_narrow_typed_workspace_bytes(self.g._h, C.byref(self.cp), self.R, self.L.ELEM_BF16 if elem is None else elem)

    def nrun(self, elem=None, skip=(), no_cot=(), fill=0xA5, no_grads=False, outs=None, ws=None, stream=None, sync=True):
        """the new entry on the bf16 (elem BF16) or the widened tensors, on a workspace of exactly the queried size"""
        import torch
        L, lib = self.L, self.lib
        elem = L.ELEM_BF16 if elem is None else elem
        bf16 = elem == L.ELEM_BF16
        nbytes = self.nquery(elem)
        assert nbytes > 0, lib.gnx_last_error()
        if ws is None:
            ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=self.g.device)
        assert ws.numel() == nbytes
        outs = self.grads(bf16, skip) if outs is None else outs
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        arrays = []
        for name in ("edge", "node", "graph"):
            arr = (L.DenseGrad * max(len(self.p[name]), 1))()
            for i in range(len(self.p[name])):
                arr[i] = L.DenseGrad(ptr(outs.get(f"{name}{i}.dW")), ptr(outs.get(f"{name}{i}.db")))
            arrays.append(arr)
        gr = L.ChainBlockGrads(*[C.cast(a, C.POINTER(L.DenseGrad)) for a in arrays])
        xin = [ptr(t) for t in (self.xb if bf16 else self.xt)]
        cot = [None if k in no_cot else ptr(t) for k, t in enumerate(self.cb if bf16 else self.cw)]
        dx = [ptr(outs.get(n)) for n in ("d_ef", "d_nf", "d_gf")]
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        rc = lib.gnx_chain_block_backward_narrow_typed(self.g._h, C.byref(self.cp), elem, *xin, *cot, self.R, *dx, None if no_grads else C.byref(gr),
                                                       ws.data_ptr(), nbytes, s)
        assert rc == 0, lib.gnx_last_error()
        if sync:
            torch.cuda.synchronize()
        return outs, nbytes

    def param_names(self):
        return [n for n in self.grad_names() if not n.startswith("d_")]

    def check_bits(self, what, skip=(), no_cot=(), no_grads=False):
        """the new entry against the staged typed call (narrow = 1) on the same nine tensors, bit for bit"""
        import torch
        skip = set(skip) | (set(self.param_names()) if no_grads else set())
        got, _ = self.nrun(skip=skip, no_cot=no_cot, no_grads=no_grads)
        ref, _ = self.brun(1, skip=skip, no_cot=no_cot)
        assert sorted(got) == sorted(ref) and not set(got) & skip
        for n in got:
            if got[n].numel() == 0:
                continue
            assert not bool(torch.isnan(ref[n].float()).any()), (what, n)
            assert got[n].dtype == ref[n].dtype == (torch.bfloat16 if n.startswith("d_") else torch.float32), (what, n)
            bad = int((TY._bits(got[n]) != TY._bits(ref[n])).sum())
            assert bad == 0, f"{what} {n}: {bad} of {got[n].numel()} elements differ from gnx_chain_block_backward_typed(narrow = 1)"
        return got


def _case(gn, which):
    """a width case by index, or a structural case by name, drawn as tests/test_gpu_chain_typed.py::test_native_bits draws it"""
    i = which if isinstance(which, int) else len(WIDTH_CASES) + STRUCTURAL.index(which) if isinstance(which, str) else 40
    rng = np.random.default_rng(100 + i)
    if isinstance(which, tuple):
        case, adjs, R = which, CN._adjs(rng), 1
    elif isinstance(which, int):
        case, adjs, R = WIDTH_CASES[which], CN._adjs(rng), 1
    else:
        case, adjs, R = TY._structural(which, rng)
    return NCall(gn, adjs, CN._params(rng, case), R, seed=i)


# ---- 1. the rule ----
def test_applies_is_the_rule(gn):
    native, staged = [], []
    for which in SWEEP:
        c = _case(gn, which)
        assert c.napplies() == c.rule(), (which, c.napplies(), c.rule(), c.bw_mask())
        assert c.napplies(c.L.ELEM_F32) == 0, which
        assert c.napplies(7) == 0 and c.nquery(7) == 0, which  # a bad elem
        (native if c.napplies() else staged).append(which)
        if which in (2, 7):  # by hand: [9,17,4] at k_in 8 needs 7626 of 16384 floats, eight 8-wide layers at k_in 8 need 11072
            assert c.bw_mask() == 7, (which, c.bw_mask())
    assert native == NATIVE and staged == STAGED, (native, staged)
    assert len(native) >= 8 and len(staged) >= 2 and 3 in staged and "edgeless-batch" in staged


def test_the_two_hand_counts():
    """the pullback's LDS need of the two cases test_applies_is_the_rule asserts inside the rule, by include/gnx.h's formula: par + 2 (64 ld + P)"""
    ceil4 = lambda x: (x + 3) & ~3

    def need(k_in, widths):
        par = P = 0
        k = k_in
        for w in widths:
            par += ceil4(k) * ceil4(w) + ceil4(w)
            P += w * (k + 1)
            k = w
        ld = (k_in + sum(widths[:-1]) + max(widths)) | 1
        return par + 2 * (64 * ld + P)

    assert need(3 + 2 * 2 + 1, [9, 17, 4]) == 7626 and need(3 + 2 * 2 + 1, [8] * 8) == 11072
    assert max(need(3 + 2 * 2 + 1, [9, 17, 4]), need(8, [8] * 8)) <= 16384


# ---- 2. bit for bit ----
def _check_all_forms(c, what):
    c.check_bits(what)
    c.check_bits(f"{what} optional", skip=SKIP, no_cot=(1,))                                 # unwanted gradients, a NULL upstream gradient
    c.check_bits(f"{what} d_ef only", skip=set(c.grad_names()) - {"d_ef"})
    c.check_bits(f"{what} grads NULL", no_grads=True)


@pytest.mark.parametrize("which", NATIVE + [WIDE_NODE_GRAPH], ids=lambda w: "node-and-rows-32-wide" if isinstance(w, tuple) else str(w))
def test_native_bits(gn, which):
    c = _case(gn, which)
    assert c.napplies() == 1 and c.bw_mask() == sum(1 << t for t in range(3) if c.outw[t] > 0), which
    if which == "odd-everything-replicas-3":  # the replicas 1 and 2 of every bf16 tensor start on a 2-byte boundary
        odd = [t for t in c.xb + c.cb if t is not None]
        assert len(odd) == 6 and all((t.shape[1] * t.shape[2]) % 2 == 1 and (t.data_ptr() + 2 * t.shape[1] * t.shape[2]) % 4 == 2 for t in odd)
    _check_all_forms(c, str(which))


def test_native_bits_on_a_partial_last_chunk(gn):
    """E and N are no multiples of 64 or 128: the last wave of the edge and node launches has a partial chunk, the last workgroup idle waves"""
    rng = np.random.default_rng(31)
    adjs = CN._adjs(rng, [37, 5, 29, 33, 11])
    c = NCall(gn, adjs, CN._params(rng, WIDTH_CASES[6]), 1, seed=31)
    E, N = c.rows[0], c.rows[1]
    assert E > 256 and E % 128 != 0 and E % 64 != 0 and N % 128 != 0 and N % 64 != 0, (E, N)
    assert c.napplies() == 1
    _check_all_forms(c, "partial chunk")


# ---- 3. the native form ran ----
def _count(prof, name):
    return prof[name]["kernels"] if name in prof else 0


def _check_native_profile(c, prof):
    assert set(prof) <= PROFILE_NAMES, sorted(set(prof) - PROFILE_NAMES)
    assert _count(prof, "k_bf16_widen") <= 2 and _count(prof, "k_bf16_round") <= 1, prof  # graph-sized; the staged call: six and three
    assert _count(prof, "bw_delta_edge") == 1, prof
    assert _count(prof, "bw_delta") == sum(1 for t in (1, 2) if c.outw[t] > 0), prof  # one launch per fused node / graph function


def test_the_native_form_ran(gn):
    for which in (6, 0, 5):  # all widths non-zero; gf nothing; the edge function alone
        c = _case(gn, which)
        assert c.napplies() == 1
        c.nrun()
        prof = CN._profiled(gn, c.nrun)
        _check_native_profile(c, prof)
        if which == 6:  # gf is widened for the graph function's input rows, d_gf rounded once
            assert _count(prof, "k_bf16_widen") == 1 and _count(prof, "k_bf16_round") == 1, prof
            staged = CN._profiled(gn, lambda: c.brun(1))
            assert _count(staged, "k_bf16_widen") == 6 and _count(staged, "k_bf16_round") == 3, staged
            for n in ("bw_delta", "bw_delta_edge", "bw_dw_generic", "bw_dnf", "bw_dgf", "bw_chain_fw_e", "bw_chain_fw_n"):
                assert _count(prof, n) == _count(staged, n), (n, prof, staged)
        if which == 0:
            assert _count(prof, "k_bf16_widen") == 0 and _count(prof, "k_bf16_round") == 0, prof


# ---- 4. workspace ----
@pytest.mark.parametrize("which", NATIVE, ids=str)
def test_workspace_bound(gn, which):
    c = _case(gn, which)
    narrow = c.lib.gnx_chain_block_backward_narrow_workspace_bytes(c.g._h, C.byref(c.cp), c.R)
    carve = -(-4 * c.R * c.rows[2] * max(c.p["in_dims"][2], c.outw[2]) // 256) * 256
    assert 0 < narrow <= c.nquery() <= narrow + 3 * carve, (narrow, c.nquery(), carve)
    assert c.nquery() < c.bquery(1, c.L.ELEM_BF16), (c.nquery(), c.bquery(1, c.L.ELEM_BF16))


# ---- 5. identities ----
def test_elem_f32_is_the_narrow_entry(gn):
    c = _case(gn, 2)
    F32 = c.L.ELEM_F32
    ga, na = c.nrun(elem=F32)
    gb, nb = c.brun(1, plain=True)
    assert na == nb == c.lib.gnx_chain_block_backward_narrow_workspace_bytes(c.g._h, C.byref(c.cp), c.R) > 0
    assert sorted(ga) == sorted(gb)
    for n in ga:
        assert TY._same(ga[n], gb[n]), n


@pytest.mark.parametrize("which", (3, "edgeless-batch"), ids=str)
def test_bf16_outside_the_rule_is_the_staged_call(gn, which):
    c = _case(gn, which)
    assert c.napplies() == 0 and c.nquery() == c.bquery(1, c.L.ELEM_BF16) > 0
    c.check_bits(str(which))
    c.check_bits(f"{which} optional", skip=SKIP, no_cot=(1,))


# ---- 6. memory contract ----
@pytest.mark.parametrize("which", (0, 2, 6, "odd-everything-replicas-3"), ids=str)
def test_memory_contract(gn, which):
    """every buffer carved at its exact size, 4-byte aligned only (a skew of 4 bytes on every bf16 and fp32 carve), the workspace exactly the
    query's; nothing but the outputs and the workspace is written, the inputs are untouched; the bits depend neither on what the workspace held
    nor on the run nor on the addresses; one byte less than the query is refused in the query's name with nothing written"""
    import torch
    L, lib = gn._lib, gn._lib.load()
    src = _case(gn, which)
    p, g, R = src.p, src.g, src.R
    BF = L.ELEM_BF16
    a = AR.Arena("cuda", skew=lambda c: 0 if c.kind == AR.WORKSPACE else 4)
    _decl_chains(a, p)
    ins = [_decl(a, n, v) for n, v in zip(("ef", "nf", "gf"), src.xb)]
    keep = []
    P = a.ptr
    gs = [_decl(a, n, v) for n, v in zip(("g_ef_out", "g_nf_out", "g_gf_out"), src.cb)]
    dx = [a.output(n, v.shape, torch.bfloat16) if v is not None else None for n, v in zip(("d_ef", "d_nf", "d_gf"), src.xb)]
    for name in ("edge", "node", "graph"):
        for k, (w, b, c) in enumerate(p[name]):
            if isinstance(w, str):
                a.output(f"grad.{name}{k}.dW", b.shape)
                a.output(f"grad.{name}{k}.db", c.shape)
            else:
                _decl_dense_grad(a, f"grad.{name}{k}", w, b)
    qname = b"gnx_chain_block_backward_narrow_typed_workspace_bytes()"
    ws = a.workspace("ws", lambda: lib.gnx_chain_block_backward_narrow_typed_workspace_bytes(g._h, C.byref(_chain_params(gn, a, p, keep)), R, BF))

    def call(nbytes):
        arrays = []
        for name in ("edge", "node", "graph"):
            arr = (L.DenseGrad * max(len(p[name]), 1))()
            for k in range(len(p[name])):
                arr[k] = _dense_grad(gn, a, f"grad.{name}{k}")
            arrays.append(arr)
        gr = L.ChainBlockGrads(*[C.cast(x_, C.POINTER(L.DenseGrad)) for x_ in arrays])
        rc = lib.gnx_chain_block_backward_narrow_typed(g._h, C.byref(_chain_params(gn, a, p, keep)), BF, *map(P, ins), *map(P, gs), R, *map(P, dx), C.byref(gr),
                                                       P(ws), nbytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    a.build(ws_fill=0x00)
    assert a.nbytes(ws) == src.nquery() > 0, lib.gnx_last_error()
    assert all(a.ptr(n) % 8 == 4 for n in ins + gs + dx if n is not None)
    assert lib.gnx_chain_block_backward_narrow_typed_applies(g._h, C.byref(_chain_params(gn, a, p, keep)), R, BF) == 1
    bits = []
    for fill in (0x00, 0xFF, 0xFF):
        a.refill(fill)
        torch.cuda.synchronize()
        assert call(a.nbytes(ws)) == 0, lib.gnx_last_error()
        a.check(f"native pullback, workspace {fill:#04x}")
        bits.append(a.output_bits())
    for k in bits[0]:
        assert torch.equal(bits[0][k], bits[1][k]), f"'{k}' depends on what the workspace held"
        assert torch.equal(bits[1][k], bits[2][k]), f"'{k}' differs between two calls"
    want, _ = src.brun(1)  # the kernels read every element by itself: the bits do not depend on the addresses either
    for n in dx:
        if n is not None:
            assert torch.equal(a.view(n).reshape(-1).view(torch.int16), want[n].view(torch.int16)), n
    a.refill(0x00)
    torch.cuda.synchronize()
    before, ws_before = a.output_bits(), a.raw(ws).clone()
    assert call(a.nbytes(ws) - 1) == L.ERR_WORKSPACE and qname in lib.gnx_last_error()
    a.check("refused", unwritten=False)
    after = a.output_bits()
    assert all(torch.equal(before[k], after[k]) for k in before) and torch.equal(ws_before, a.raw(ws)), "a refused call wrote an output or the workspace"


# ---- 7. capture ----
def test_a_captured_native_pullback_replays_the_eager_bits(gn):
    import torch
    c = _case(gn, 6)
    assert c.napplies() == 1
    nbytes = c.nquery()  # (builds the tables the call reads, the out-edge view included, outside the capture)
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device=c.g.device)
    eager, _ = c.nrun(ws=ws)
    graphed = c.grads(True)
    side = torch.cuda.Stream()
    cg = torch.cuda.CUDAGraph()
    gc.collect()  # nothing may free device memory while the capture is open
    gc.disable()
    try:
        with torch.cuda.stream(side):
            with torch.cuda.graph(cg, stream=side):
                c.nrun(outs=graphed, ws=ws, stream=side.cuda_stream, sync=False)
    finally:
        gc.enable()
    for t in graphed.values():
        t.zero_()
    cg.replay()
    torch.cuda.synchronize()
    assert sorted(eager) == sorted(graphed)
    for n in eager:
        assert TY._same(eager[n], graphed[n]), n


# ---- 8. Python ----
def test_python_switch(gn):
    import torch
    c = _case(gn, 2)
    blk = c.blk
    assert blk.native_chain_backward is False  # off by default
    blk.bf16_chain, blk.narrow_chain, blk.native_chain_backward = True, True, True
    leaves = []
    for ch in (blk.edgefn, blk.nodefn, blk.graphfn):
        for l in ch.layers:
            l.weight.requires_grad_(True); l.bias.requires_grad_(True)
            leaves.append((l.weight, l.bias))
    xt = [None if t is None else t.clone().requires_grad_(True) for t in c.xb]
    with pytest.raises(NotImplementedError, match="bf16_backward"):  # still required
        blk(TY._nt(gn, c, xt))
    blk.bf16_backward = True
    assert c.napplies() == 1
    want, _ = c.nrun()
    y = blk(TY._nt(gn, c, xt))
    assert all(o.dtype == torch.bfloat16 for o in (y.ef, y.nf, y.gf))
    loss = sum((o.permute(2, 1, 0).float() * ct.float()).sum() for o, ct in zip((y.ef, y.nf, y.gf), c.cb) if o is not None)
    prof = CN._profiled(gn, loss.backward)
    torch.cuda.synchronize()
    for n, t in zip(("d_ef", "d_nf", "d_gf"), xt):
        if t is not None:
            assert t.grad.dtype == torch.bfloat16 and torch.equal(TY._bits(t.grad).reshape(-1), TY._bits(want[n])), n
    k = 0
    for name in ("edge", "node", "graph"):
        for i in range(len(c.p[name])):
            w, b = leaves[k]; k += 1
            gw = w.grad if w.grad.dim() == 1 else w.grad.t()
            assert gw.dtype == torch.float32 and torch.equal(TY._bits(gw).reshape(-1), TY._bits(want[f"{name}{i}.dW"])), (name, i)
            assert torch.equal(TY._bits(b.grad).reshape(-1), TY._bits(want[f"{name}{i}.db"])), (name, i)
    _check_native_profile(c, prof)


# ---- 9. seeded sweep ----
@pytest.mark.parametrize("seed", range(12 + EXTRA))
def test_seeded_sweep(gn, seed):
    rng = np.random.default_rng(7000 + seed)
    case = CN._random_block(rng)
    R = 1
    adjs = CN._adjs(rng)
    if seed % 6 == 5:
        adjs, R = CN._adjs(rng, [int(rng.integers(3, 40))]), int(rng.integers(2, 4))
    c = NCall(gn, adjs, CN._params(rng, case), R, seed=seed)
    assert c.napplies() == c.rule(), case
    if c.outw[0] == 0:  # no pullback without an edge output: refused, as by every Chain pullback entry
        assert c.napplies() == 0
        return
    c.check_bits(f"sweep {seed} {case}")
    c.check_bits(f"sweep {seed} {case} optional", skip=SKIP, no_cot=(1,))
