"""gnx_block_backward_fused_typed on the GPU, GNX_ELEM_BF16.  Every comparison but one is torch.equal on raw bits.  With W(x) the fp32 widening
of a bf16 tensor and rb round-to-nearest-even to bf16, where the call applies:

  d_ef, d_nf, d_gf             == gnx_block_backward_typed's on the same nine bf16 tensors, and == rb(gnx_block_backward_fused(W(.)))
  dWn, dbn, dWg, dbg           == both of those calls' values
  dWe, dbe                     == gnx_block_backward_fused(W(.))'s (exact widenings, the same summation order)
  two runs on workspaces filled with different bytes give the same bits

and, one anchor per width set, dWe / dbe against torch float64 autograd at the bar of tests/test_gpu_backward.py, max|got - ref| <= 2e-4
max(1, max|ref|).  The float64 reference is the pullback this ABI defines — evaluated AT THE ROUNDED SAVED OUTPUTS (include/gnx.h): the restated
forward of tests/test_gpu_backward.py under autograd, each activation replaced by a function whose value is the saved bf16 output and whose
derivative is act' taken from it.  The forward inputs come from gnx_block_forward_typed.  Graphs and shapes are those of
tests/test_gpu_bw_fused.py (several chunks per tile, single-node tiles above the edge cap, nodes without in-edges, self-loops, graphs without
edges, more than 256 wave tiles, more than 256 partial rows).

Addresses.  The entry refuses a bf16 buffer that is not 4-byte aligned before any launch (check_bf16_aligned, as gnx_block_backward_typed), so
a tensor passed as a view one element into its buffer is refused — tested below, nothing written.  Whole tensors that start 2 bytes into a dword
do reach the kernel: with two replicas on a graph of 1501 edges and 261 nodes, replica 1 of every odd-width tensor (ef, ef_out, g_ef_out, d_ef at
width 3; nf, d_nf at width 5; gf at width 5) starts at an odd element, and inside every replica every second row of an odd-width tensor does.
The arena cases put every buffer 4, 8 and 12 bytes behind a 256-byte boundary."""
import ctypes as C

import numpy as np
import pytest

from tests import util as U
from tests.arena import Arena, WORKSPACE
from tests.test_gpu_backward import _torch_block
from tests.test_gpu_bw_fused import ACTS, GRAPHS, NAMES, README, SETS, Case, _graph, _profiled, _ptr, _seed, _stream

pytestmark = pytest.mark.gpu

S345 = ((3, 4, 5), (3, 4, 5))
NEW, TYPED, FUSED32 = "fused_typed", "typed", "fused_fp32"


@pytest.fixture(scope="module")
def gn():
    import torch
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b, what):
    import torch
    assert (a is None) == (b is None), what
    if a is None:
        return
    assert a.dtype == b.dtype and a.shape == b.shape, what
    x, y = _bits(a), _bits(b)
    if not torch.equal(x, y):
        bad = (x != y).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {x.numel()} values differ, first at {i}: {a[i].item()!r} vs {b[i].item()!r}")


def _rb(t):
    import torch
    return None if t is None else t.to(torch.bfloat16)


def _wide(ts):
    return [None if t is None else t.float() for t in ts]


def _at_saved(code):
    """an activation for _torch_block: value = the saved output, derivative = act' taken from the saved output (codes of include/gnx.h)"""
    import torch

    class AtSaved(torch.autograd.Function):
        @staticmethod
        def forward(ctx, z, y):
            ctx.save_for_backward(y)
            return y.clone()

        @staticmethod
        def backward(ctx, g):
            y, = ctx.saved_tensors
            d = {0: torch.ones_like(y), 1: (y > 0).to(y.dtype), 2: 1 - y * y, 3: y * (1 - y)}[code]
            return g * d, None

    return AtSaved.apply


def edge_grads_f64(p, csc, act, ins, outs, cots):
    """(dWe in the (in, out) layout of the ABI, dbe): torch float64 autograd of the restated forward at the saved outputs, summed over the replicas.
    ins / outs / cots: three packed [R][T][d] tensors each (None where the width is 0 or the cotangent absent)"""
    import torch
    W = {k: torch.tensor(p[k], dtype=torch.float64, requires_grad=True) for k in ("We", "be", "Wn", "bn", "Wg", "bg")}
    f64 = lambda t, r: None if t is None else t[r].double().cpu()
    loss = 0.0
    R = next(t.shape[0] for t in outs if t is not None)
    for r in range(R):
        saved = [f64(o, r) for o in outs]
        acts = [(lambda z, y=y, f=_at_saved(a): f(z, y)) for y, a in zip(saved, act)]
        res = _torch_block(p, csc, *[f64(t, r) for t in ins], W, None, acts)
        for o, c in zip(res, cots):
            if c is not None and o.shape[1] > 0:
                loss = loss + (o * f64(c, r)).sum()
    loss.backward()
    return W["We"].grad.numpy().T, W["be"].grad.numpy()


def _at_the_bar(got, ref, what):
    err = float(np.max(np.abs(got.double().cpu().numpy() - ref)))
    scale = max(1.0, float(np.abs(ref).max()))
    print(f"{what}: max err {err:.3e}, bar {2e-4 * scale:.3e}")
    assert err <= 2e-4 * scale, f"{what}: max err {err:.3e} (scale {scale:.3g})"


class Case16(Case):
    """Case of tests/test_gpu_bw_fused.py (the block, the kink-free draw), its inputs and cotangents rounded once to bf16 and the bf16 outputs of
    gnx_block_forward_typed on them: the nine bf16 tensors of a backward call"""

    def __init__(self, gn, g, R, in_dims, out_dims, act, seed):
        import torch
        super().__init__(gn, g, R, in_dims, out_dims, act, seed)
        lib, L = gn._lib.load(), gn._lib
        self.BF = L.ELEM_BF16
        self.ins16 = [_rb(t) for t in self.ins]
        self.outs16 = [torch.empty((R, T, d), dtype=torch.bfloat16, device="cuda") if d > 0 else None for T, d in zip(self.rows, out_dims)]
        nb = int(lib.gnx_block_typed_workspace_bytes(g._h, C.byref(self.cp), R, self.BF, 0))
        assert nb > 0, lib.gnx_last_error()
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        assert lib.gnx_block_forward_typed(g._h, C.byref(self.cp), self.BF, *map(_ptr, self.ins16), R, *map(_ptr, self.outs16), ws.data_ptr(), ws.numel(), 0,
                                           _stream()) == 0, lib.gnx_last_error()
        self.cots16 = [_rb(c) for c in self.cots]
        torch.cuda.synchronize()
        self.applies16 = int(lib.gnx_block_backward_fused_typed_applies(g._h, C.byref(self.cp), R, self.BF))

    def nine16(self, cots=(True, True, True)):
        return self.ins16 + self.outs16 + [c if keep else None for c, keep in zip(self.cots16, cots)]

    def query16(self, form):
        lib = self.gn._lib.load()
        a = (self.g._h, C.byref(self.cp), self.R)
        if form == FUSED32:
            return int(lib.gnx_block_backward_fused_workspace_bytes(*a))
        return int((lib.gnx_block_backward_fused_typed_workspace_bytes if form == NEW else lib.gnx_block_backward_typed_workspace_bytes)(*a, self.BF))

    def run(self, form, nine, want_d=(True, True, True), want_g=(True,) * 6, grads_null=False, ws_fill=0xA5):
        """one call: [d_ef, d_nf, d_gf, dWe, dbe, dWn, dbn, dWg, dbg], None where not wanted; every output starts as NaN"""
        import torch
        g, R = self.g, self.R
        lib, L = self.gn._lib.load(), self.gn._lib
        dt = torch.float32 if form == FUSED32 else torch.bfloat16
        nan = lambda shape, dtype: torch.full(shape, float("nan"), dtype=dtype, device="cuda")
        d = [nan((R, T, w), dt) if (w > 0 and keep) else None for T, w, keep in zip(self.rows, self.in_dims, want_d)]
        flat = [s for pair in self.grad_shapes() for s in pair]
        gs = [nan(tuple(s), torch.float32) if keep and int(np.prod(s)) > 0 else None for s, keep in zip(flat, want_g)]
        grads = L.BlockGrads(*[L.DenseGrad(_ptr(gs[2 * i]), _ptr(gs[2 * i + 1])) for i in range(3)])
        gp = None if grads_null else C.byref(grads)
        nb = self.query16(form)
        assert nb > 0, lib.gnx_last_error()
        ws = torch.full((nb,), ws_fill, dtype=torch.uint8, device="cuda")
        tail = (R, *map(_ptr, d), gp, ws.data_ptr(), ws.numel(), _stream())
        if form == FUSED32:
            rc = lib.gnx_block_backward_fused(g._h, C.byref(self.cp), *map(_ptr, nine), *tail)
        else:
            call = lib.gnx_block_backward_fused_typed if form == NEW else lib.gnx_block_backward_typed
            rc = call(g._h, C.byref(self.cp), self.BF, *map(_ptr, nine), *tail)
        assert rc == 0, lib.gnx_last_error()
        torch.cuda.synchronize()
        return d + (gs if not grads_null else [None] * 6)

    def check16(self, what, cots=(True, True, True), want_d=(True, True, True), want_g=(True,) * 6, grads_null=False, anchor=False):
        import torch
        nine = self.nine16(cots)
        kw = dict(want_d=want_d, want_g=want_g, grads_null=grads_null)
        got = self.run(NEW, nine, **kw)
        again = self.run(NEW, nine, ws_fill=0x3C, **kw)
        typed = self.run(TYPED, nine, **kw)
        for name, a, b in zip(NAMES, got, again):
            _same(a, b, f"{what} {name}: two runs, two workspace fills")
        for t in got[:3]:
            assert t is None or t.numel() == 0 or bool(torch.isfinite(t.float()).all()), what
        if not self.applies16:
            assert self.query16(NEW) == self.query16(TYPED), what
            for name, a, b in zip(NAMES, got, typed):
                _same(a, b, f"{what} {name}: not applicable, the typed call")
            return got
        wide = self.run(FUSED32, _wide(nine), **kw)
        for i, (name, a, t, w) in enumerate(zip(NAMES, got, typed, wide)):
            if i < 3:
                _same(a, t, f"{what} {name}: the typed call")
                _same(a, _rb(w), f"{what} {name}: rb(fused fp32 on the widened tensors)")
            elif i < 5:
                _same(a, w, f"{what} {name}: fused fp32 on the widened tensors")
            else:
                _same(a, t, f"{what} {name}: the typed call")
                _same(a, w, f"{what} {name}: fused fp32 on the widened tensors")
        if anchor:
            assert got[3] is not None and got[4] is not None
            dWe, dbe = edge_grads_f64(self.p, self.csc, self.act, self.ins16, self.outs16, nine[6:])
            _at_the_bar(got[3], dWe, f"{what} dWe")
            _at_the_bar(got[4], dbe, f"{what} dbe")
        return got


@pytest.mark.parametrize("dims", SETS)
@pytest.mark.parametrize("graph", GRAPHS)
def test_bits_of_the_typed_and_of_the_fused_backward(gn, graph, dims):
    g = _graph(gn, graph)
    for act in ACTS:
        c = Case16(gn, g, 1, *dims, act, _seed("bf16", dims, act, graph))
        assert c.applies16 == (0 if graph == "edgeless" else 1), (graph, dims)
        c.check16(f"{graph} {dims[0]}=>{dims[1]} act={act}")


@pytest.mark.parametrize("dims", SETS)
def test_edge_gradients_against_float64_at_the_bar(gn, dims):
    """the anchor of each width set: relu edges (the kink-free draw) and tanh edges on the degree graph (single-node tiles, several chunks)"""
    for act in ((1, 2, 3), (2, 3, 2)):
        c = Case16(gn, _graph(gn, "degrees"), 1, *dims, act, _seed("anchor", dims, act))
        assert c.applies16 == 1
        c.check16(f"anchor {dims} act={act}", anchor=True)


@pytest.mark.parametrize("graph,R", [("e20k", 2), ("e20k", 3), ("n20k", 4)], ids=["R2", "R3", "R4-more-than-256-partial-rows"])
def test_replicas(gn, graph, R):
    g = _graph(gn, graph)
    for dims in (README, S345):
        c = Case16(gn, g, R, *dims, (2, 3, 0), _seed("rep16", R, dims))
        assert c.applies16 == 1
        c.check16(f"{graph} R={R} {dims}")


@pytest.mark.parametrize("graph", ["degrees", "small40"])
def test_optional_arguments(gn, graph):
    """each upstream gradient NULL, each of d_ef / d_nf / d_gf not wanted, grads NULL, the edge weight gradient alone, the edge bias gradient alone"""
    g = _graph(gn, graph)
    for dims, seed in ((S345, 77), (README, 78)):
        c = Case16(gn, g, 1, *dims, (1, 2, 3), seed)
        assert c.applies16 == 1
        for k in range(3):
            c.check16(f"{graph} {dims} without cotangent {k}", cots=tuple(i != k for i in range(3)))
        c.check16(f"{graph} {dims} without any cotangent", cots=(False, False, False))
        for k in range(3):
            c.check16(f"{graph} {dims} without d[{k}]", want_d=tuple(i != k for i in range(3)))
        c.check16(f"{graph} {dims} no input gradient", want_d=(False, False, False))
        c.check16(f"{graph} {dims} grads NULL", grads_null=True)
        c.check16(f"{graph} {dims} dWe alone", want_g=(True, False, False, False, False, False))
        c.check16(f"{graph} {dims} dbe alone", want_g=(False, True, False, False, False, False))
        c.check16(f"{graph} {dims} no edge gradient", want_g=(False, False, True, True, True, True))
        c.check16(f"{graph} {dims} dWe alone, no input gradient", want_d=(False, False, False), want_g=(True, False, False, False, False, False))


_odd = {}


def _odd_graph(gn):
    """one graph of 261 nodes and 1501 edges: odd row counts, so that replica 1 of an odd-width tensor starts at an odd bf16 element"""
    if "g" not in _odd:
        colptr, rowval = U.er_csc(np.random.default_rng(6), 261, 1501)
        _odd["g"] = gn.GNGraphBatch.from_csc([colptr], [rowval], [261])
        assert _odd["g"].n_edges == 1501 and _odd["g"].n_nodes == 261
    return _odd["g"]


@pytest.mark.parametrize("dims", [pytest.param(S345, id="345"), pytest.param(README, id="1050-dn5")])
def test_tensors_that_start_two_bytes_into_a_dword(gn, dims):
    """R = 2 on odd row counts: replica 1 of ef / ef_out / g_ef_out / d_ef (width 3), of nf / d_nf (width 5) and of gf (width 5) lies 2 bytes behind a
    4-byte boundary — every row of it at the other parity than in replica 0"""
    g = _odd_graph(gn)
    c = Case16(gn, g, 2, *dims, (1, 2, 3), _seed("odd", dims))
    assert c.applies16 == 1
    skewed = [t for t in c.nine16() if t is not None and t[1].data_ptr() % 4 == 2]
    assert len(skewed) >= (6 if dims == S345 else 3), [None if t is None else t[1].data_ptr() % 4 for t in c.nine16()]
    c.check16(f"odd graph R=2 {dims}")
    c.check16(f"odd graph R=2 {dims}, d_ef alone", want_d=(True, False, False), want_g=(False,) * 6)


def test_a_view_one_element_into_its_buffer_is_refused_before_any_launch(gn):
    """the typed call's status for a bf16 buffer that is not 4-byte aligned; outputs and workspace untouched"""
    import torch
    lib, L = gn._lib.load(), gn._lib
    c = Case16(gn, _graph(gn, "degrees"), 1, *S345, (1, 2, 3), 3)
    nine = c.nine16()
    outs = [torch.full_like(t, float("nan")) for t in c.ins16] + [torch.full(tuple(s), float("nan"), device="cuda") for pair in c.grad_shapes() for s in pair]
    grads = L.BlockGrads(*[L.DenseGrad(_ptr(outs[3 + 2 * i]), _ptr(outs[4 + 2 * i])) for i in range(3)])
    nb = c.query16(NEW)
    ws = torch.full((nb,), 0x5A, dtype=torch.uint8, device="cuda")

    def view1(t):
        buf = torch.empty(t.numel() + 1, dtype=torch.bfloat16, device="cuda")
        buf[1:] = t.reshape(-1)
        return buf[1:]

    for k in range(9):
        args = list(nine)
        args[k] = view1(nine[k])
        assert args[k].data_ptr() % 4 == 2
        rc = lib.gnx_block_backward_fused_typed(c.g._h, C.byref(c.cp), c.BF, *map(_ptr, args), 1, *map(_ptr, outs[:3]), C.byref(grads), ws.data_ptr(), nb, _stream())
        assert rc == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error(), k
    for k in range(3):
        d = list(outs[:3])
        d[k] = view1(outs[k])
        rc = lib.gnx_block_backward_fused_typed(c.g._h, C.byref(c.cp), c.BF, *map(_ptr, nine), 1, *map(_ptr, d), C.byref(grads), ws.data_ptr(), nb, _stream())
        assert rc == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error(), k
    # a workspace one byte short, a missing workspace
    assert lib.gnx_block_backward_fused_typed(c.g._h, C.byref(c.cp), c.BF, *map(_ptr, nine), 1, *map(_ptr, outs[:3]), C.byref(grads), ws.data_ptr(), nb - 1,
                                              _stream()) == L.ERR_WORKSPACE
    assert b"gnx_block_backward_fused_typed_workspace_bytes" in lib.gnx_last_error()
    assert lib.gnx_block_backward_fused_typed(c.g._h, C.byref(c.cp), c.BF, *map(_ptr, nine), 1, *map(_ptr, outs[:3]), C.byref(grads), None, nb,
                                              _stream()) == L.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all()) and all(bool(torch.isnan(t.float()).all()) for t in outs)


def test_where_it_does_not_apply_it_is_the_typed_backward(gn):
    """a gelu edge function; (10,5,0) => (3,16,5) on 260 nodes, where the node level is on the matrix cores (the fp32 fused call applies there, the
    bf16 one does not: the typed call stages); a batch without edges.  applies == 0, the typed query's size, the typed call's bits in every
    output; elem = GNX_ELEM_F32 is gnx_block_backward_fused: its answer, its size, its bits"""
    import torch
    lib, L = gn._lib.load(), gn._lib
    for graph, dims, act, fp32_applies in (("degrees", README, (4, 0, 0), 0), ("degrees", ((10, 5, 0), (3, 16, 5)), (2, 2, 2), 1),
                                          ("e20k", ((10, 5, 0), (3, 16, 5)), (1, 2, 3), 1), ("edgeless", README, (2, 2, 2), 0)):
        c = Case16(gn, _graph(gn, graph), 1, *dims, act, 5)
        assert c.g.n_nodes >= 64 or graph == "edgeless"
        assert c.applies16 == 0 and c.applies == fp32_applies, (graph, dims, act)
        assert c.query16(NEW) == c.query16(TYPED)
        c.check16(f"not applicable: {graph} {dims} {act}")
        c.check16(f"not applicable: {graph} {dims} {act}, d_nf alone", want_d=(False, True, False), want_g=(False,) * 6)
        # elem = F32
        a3 = (c.g._h, C.byref(c.cp), 1)
        assert lib.gnx_block_backward_fused_typed_applies(*a3, L.ELEM_F32) == fp32_applies
        nb = int(lib.gnx_block_backward_fused_typed_workspace_bytes(*a3, L.ELEM_F32))
        assert nb == c.query(True)
        nine = c.nine()
        ref = c.backward(True, nine)
        outs = [None if t is None else torch.full_like(t, float("nan")) for t in ref]
        grads = L.BlockGrads(*[L.DenseGrad(_ptr(outs[3 + 2 * i]), _ptr(outs[4 + 2 * i])) for i in range(3)])
        ws = torch.full((nb,), 0x11, dtype=torch.uint8, device="cuda")
        assert lib.gnx_block_backward_fused_typed(c.g._h, C.byref(c.cp), L.ELEM_F32, *map(_ptr, nine), 1, *map(_ptr, outs[:3]), C.byref(grads), ws.data_ptr(), nb,
                                                  _stream()) == 0, lib.gnx_last_error()
        torch.cuda.synchronize()
        for name, x, y in zip(NAMES, outs, ref):
            _same(x, y, f"elem F32 {graph} {dims}: {name}")


def test_launch_structure(gn):
    """against the typed call: no edge function-input launch, no edge k_bw_dx, one launch under bw_delta_edge (the fused kernel), the final reduction
    alone for the edge weight gradient, no new profiler name; the workspace on the C2-like graph is below the typed query's"""
    if U.default_flags(gn) != 0:
        return  # (forms switched on for the whole process change which kernels run, not the bits)
    for graph, R in (("e20k", 1), ("e20k", 2), ("small40", 1)):
        c = Case16(gn, _graph(gn, graph), R, *README, (1, 2, 3), 9)
        nine = c.nine16()
        typ = _profiled(gn, lambda: c.run(TYPED, nine))
        new = _profiled(gn, lambda: c.run(NEW, nine))
        assert set(new) <= set(typ), (sorted(new), sorted(typ))
        assert new["bw_fn_inputs"]["kernels"] == typ["bw_fn_inputs"]["kernels"] - 1, (new["bw_fn_inputs"], typ["bw_fn_inputs"])
        assert new["bw_dx_generic"]["launches"] == typ["bw_dx_generic"]["launches"] - 1, (new["bw_dx_generic"], typ["bw_dx_generic"])
        assert new["bw_delta_edge"]["kernels"] == typ["bw_delta_edge"]["kernels"] == 1
        assert new["bw_dw_generic"]["kernels"] == typ["bw_dw_generic"]["kernels"] - 1
        for name in ("bw_dnf", "bw_dgf", "k_bf16_round"):
            assert (name in new) == (name in typ) and (name not in typ or new[name]["kernels"] == typ[name]["kernels"]), name
        if graph == "e20k":
            ke = 20
            print(f"{graph} R={R}: fused typed {c.query16(NEW)} B, typed {c.query16(TYPED)} B, fused fp32 {c.query16(FUSED32)} B")
            assert c.query16(NEW) <= c.query16(TYPED) - 4 * R * c.g.n_edges * ke
            assert c.query16(NEW) >= c.query16(FUSED32)


@pytest.mark.parametrize("dims", SETS)
def test_arena_memory_contract_and_skewed_addresses(gn, dims):
    """Every buffer of the call at its exact byte size inside one sentinel arena, aligned and 4 / 8 / 12 bytes behind a 256-byte boundary (the
    workspace on it): nothing outside the outputs and the workspace is written, the inputs are untouched, every requested output element is
    written, the bits are those of the plain-tensor run and do not depend on the address or on what the workspace held."""
    import torch
    lib, L = gn._lib.load(), gn._lib
    g, R = _graph(gn, "degrees"), 1
    c = Case16(gn, g, R, *dims, (1, 2, 3), 13)
    a = Arena("cuda")
    names = ("ef", "nf", "gf", "ef_out", "nf_out", "gf_out", "g_ef_out", "g_nf_out", "g_gf_out")
    nine = [a.input(n, t) if t is not None else None for n, t in zip(names, c.nine16())]
    dx = [a.output(n, t.shape, torch.bfloat16) if t is not None else None for n, t in zip(("d_ef", "d_nf", "d_gf"), c.ins16)]
    gnames = []
    for fn, (sw, sb) in zip(("edgefn", "nodefn", "graphfn"), c.grad_shapes()):
        gnames += [a.output(f"grad.{fn}.dW", sw), a.output(f"grad.{fn}.db", sb)]
    ws = a.workspace("ws", c.query16(NEW))
    a.build(ws_fill=0x00)

    def run():
        keep = []
        cp = c.blk._c(keep)
        grads = L.BlockGrads(*[L.DenseGrad(a.ptr(gnames[2 * k]), a.ptr(gnames[2 * k + 1])) for k in range(3)])
        rc = lib.gnx_block_backward_fused_typed(g._h, C.byref(cp), c.BF, *map(a.ptr, nine), R, *map(a.ptr, dx), C.byref(grads), a.ptr(ws), a.nbytes(ws), _stream())
        torch.cuda.synchronize()
        return rc

    assert run() == 0, lib.gnx_last_error()
    a.check(f"{dims} aligned")
    base = a.output_bits()
    ref = c.check16("arena reference")
    for n, t in zip(dx + gnames, ref):
        if n is not None:
            assert torch.equal(a.raw(n), t.contiguous().view(-1).view(torch.uint8)), n
    for k in (4, 8, 12):  # every buffer k bytes behind a 256-B boundary, the workspace on it
        a.relayout(lambda cv: 0 if cv.kind == WORKSPACE else k, ws_fill=0xFF)
        assert run() == 0, (k, lib.gnx_last_error())
        a.check(f"{dims} skew +{k}")
        got = a.output_bits()
        assert all(torch.equal(got[n], base[n]) for n in base), f"{dims}: other bits at +{k}"


def test_graph_capture_replays_same_bits(gn):
    import torch
    lib, L = gn._lib.load(), gn._lib
    c = Case16(gn, _graph(gn, "e20k"), 1, *README, (1, 2, 3), 14)
    nine = c.nine16()
    eager = c.run(NEW, nine)  # (the query ran here: outside the capture)
    outs = [None if t is None else torch.zeros_like(t) for t in eager]
    grads = L.BlockGrads(*[L.DenseGrad(_ptr(outs[3 + 2 * i]), _ptr(outs[4 + 2 * i])) for i in range(3)])
    ws = torch.empty(c.query16(NEW), dtype=torch.uint8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            assert lib.gnx_block_backward_fused_typed(c.g._h, C.byref(c.cp), c.BF, *map(_ptr, nine), 1, *map(_ptr, outs[:3]), C.byref(grads), ws.data_ptr(),
                                                      ws.numel(), s.cuda_stream) == 0, lib.gnx_last_error()
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES, outs, eager):
        _same(x, y, f"captured {name}")


# ---- Python ----
def _py_case(gn, fused, seed=21):
    import torch
    from oracle import gn_oracle as O
    rng = np.random.default_rng(seed)
    colptr, rowval = U.er_csc(rng, 300, 2500)
    g = gn.GNGraphBatch.from_csc([colptr], [rowval], [300])
    p = O.make_block_params(rng, *README, act=(2, 2, 0))
    blk = U.block_from_params(gn, p)
    blk.bf16_backward = True
    blk.fused_backward = fused
    params = [blk.edgefn.weight, blk.edgefn.bias, blk.nodefn.weight, blk.nodefn.bias, blk.graphfn.weight, blk.graphfn.bias]
    for t in params:
        t.requires_grad_(True)
    ef, nf, _ = U.packed_inputs(rng, 1, 2500, 300, 1, README[0])
    x = U.to_nt(gn, g, ef, nf, None)
    x = gn.NT(x.graphs, x.ef.to(torch.bfloat16), x.nf.to(torch.bfloat16), None)
    cot = [torch.from_numpy(rng.standard_normal((d, T, 1)).astype(np.float32)).to(g.device).to(torch.bfloat16) for d, T in zip(README[1], (2500, 300, 1))]
    return blk, params, x, cot, p, g


def test_python_autograd_with_both_switches(gn):
    """GNBlock(..., bf16_backward=True, fused_backward=True) on bf16 features under torch.autograd: the input gradients and the node / graph
    parameter gradients are the bits of the same block with fused_backward off, dWe / dbe within the bar of float64; AdamW steps reduce a loss"""
    import torch
    res = []
    for fused in (False, True):
        blk, params, x, cot, p, g = _py_case(gn, fused)
        assert blk.fused_backward is fused and blk.bf16_backward is True
        ef, nf = x.ef.detach().requires_grad_(True), x.nf.detach().requires_grad_(True)
        y = blk(gn.NT(x.graphs, ef, nf, None))
        assert all(t.dtype == torch.bfloat16 for t in (y.ef, y.nf, y.gf))
        sum((t.float() * c.float()).sum() for t, c in zip((y.ef, y.nf, y.gf), cot)).backward()  # d/dy = the bf16 cotangent exactly
        assert ef.grad.dtype == torch.bfloat16 and nf.grad.dtype == torch.bfloat16
        res.append([ef.grad, nf.grad] + [t.grad for t in params])
    pk = lambda t: None if t is None else t.detach().permute(2, 1, 0).contiguous()
    dWe, dbe = edge_grads_f64(p, (*g.csc(), g.node_off, g.edge_off), (2, 2, 0), [pk(x.ef), pk(x.nf), None], [pk(y.ef), pk(y.nf), pk(y.gf)], [pk(c) for c in cot])
    for i, (name, a, b) in enumerate(zip(("x.ef", "x.nf", "We", "be", "Wn", "bn", "Wg", "bg"), *res)):
        if i == 2:
            _at_the_bar(b.t(), dWe, "python dWe")
        elif i == 3:
            _at_the_bar(b, dbe, "python dbe")
        else:
            _same(a.contiguous(), b.contiguous(), f"grad {name}")
    blk, params, x, cot, p, g = _py_case(gn, True)
    target = [torch.from_numpy(np.random.default_rng(5).standard_normal((d, T, 1)).astype(np.float32)).to(g.device) for d, T in zip(README[1], (2500, 300, 1))]

    def loss_fn():
        y = blk(x)
        return sum(((o.float() - t) ** 2).mean() for o, t in zip((y.ef, y.nf, y.gf), target))

    first = float(loss_fn().detach())
    opt = torch.optim.AdamW(params, lr=1e-2)
    for _ in range(40):
        opt.zero_grad()
        loss_fn().backward()
        opt.step()
    last = float(loss_fn().detach())
    assert np.isfinite(last) and last < first, (first, last)
