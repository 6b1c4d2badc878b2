"""gnx_block_backward_typed on the GPU.  The reference of every case is built here from the public fp32 entry: gnx_block_backward on .float()
of the same nine bf16 tensors, its three input gradients rounded with .to(torch.bfloat16).  Every comparison is torch.equal on raw bits — no
tolerance: the input gradients are bit for bit the rounded reference, every parameter gradient bit for bit the reference's.  Shapes are the
smallest at which the typed kernels can go wrong: odd widths on 3001 edges / 300 nodes give odd element counts (a lone last 16-bit element
and rows that start in the middle of a dword), more than one workgroup per kernel, replicas, graphs without edges, and both paths (the native
one and, from 64 rows on at matrix-core widths, the staging one)."""
import ctypes as C
import zlib

import numpy as np
import pytest

from oracle import gn_oracle as O
from tests import util as U
from tests.arena import Arena

pytestmark = pytest.mark.gpu

README = ((10, 5, 0), (3, 4, 5))
SAME = ((3, 4, 5), (3, 4, 5))
WIDE = ((10, 5, 3), (10, 5, 3))  # edge J.K = 10 * 23, node J.K = 5 * 18: the matrix cores from 64 rows on
DIMS = [pytest.param(README, id="readme"), pytest.param(SAME, id="345"), pytest.param(((3, 2, 4), (3, 4, 5)), id="324"),
        pytest.param(((0, 2, 0), (2, 2, 2)), id="020"), pytest.param(((4, 0, 3), (2, 3, 2)), id="403"), pytest.param(((6, 5, 0), (4, 3, 0)), id="650"),
        pytest.param(WIDE, id="1053")]
ACTS = ((0, 0, 0), (1, 2, 3), (4, 4, 4))
BATCHES = ["one", "one-R3", "small40", "edgeless", "tiny"]


@pytest.fixture(scope="module")
def gn():
    import torch
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


_graphs = {}


def _batch(gn, name):
    """(graphs, R), built once per module"""
    if name not in _graphs:
        if name in ("one", "one-R3"):  # the same handle, one replica or three
            colptr, rowval = U.er_csc(np.random.default_rng(1), 300, 3001)
            g = gn.GNGraphBatch.from_csc([colptr], [rowval], [300])
            assert g.n_edges == 3001 and g.n_nodes == 300
            _graphs["one"], _graphs["one-R3"] = (g, 1), (g, 3)
        elif name == "small40":
            rng = np.random.default_rng(2)
            sizes = [1, 1, 12, 2] + list(rng.integers(1, 13, 36))
            adjs = U.random_graphs(rng, sizes, 0.3)
            adjs[2][:] = 0  # a 12-node graph without edges
            adjs[5][:] = 0
            _graphs[name] = (gn.GNGraphBatch(adjs), 1)
        elif name == "edgeless":
            _graphs[name] = (gn.GNGraphBatch([np.zeros((n, n), dtype=np.int64) for n in (3, 5, 2)]), 1)
        else:
            colptr, rowval = U.er_csc(np.random.default_rng(3), 5, 9)
            _graphs[name] = (gn.GNGraphBatch.from_csc([colptr], [rowval], [5]), 1)
    return _graphs[name]


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


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


class Case:
    """A block, its bf16 inputs, the bf16 outputs of gnx_block_forward_typed and random bf16 cotangents: the nine tensors of a backward call."""

    def __init__(self, gn, g, R, in_dims, out_dims, act, seed):
        import torch
        self.gn, self.g, self.R, self.in_dims, self.out_dims = gn, g, R, in_dims, out_dims
        lib, L = gn._lib.load(), gn._lib
        rng = np.random.default_rng(seed)
        self.p = O.make_block_params(rng, in_dims, out_dims, act=act)
        self.blk = U.block_from_params(gn, self.p)
        self.keep = []
        self.cp = self.blk._c(self.keep)
        self.rows = (g.n_edges, g.n_nodes, g.n_graphs)
        # values of both signs over a few binades, rounded once to bf16 (the inputs ARE bf16)
        mk = lambda a: None if a is None else torch.from_numpy((a * 4 - 2).astype(np.float32)).cuda().to(torch.bfloat16).contiguous()
        self.ins = [mk(a) for a in U.packed_inputs(rng, R, *self.rows, in_dims)]
        self.outs = [torch.empty((R, T, d), dtype=torch.bfloat16, device="cuda") if d > 0 else None for T, d in zip(self.rows, out_dims)]
        nb = int(lib.gnx_block_typed_workspace_bytes(g._h, C.byref(self.cp), R, L.ELEM_BF16, 0))
        assert nb > 0, lib.gnx_last_error()
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        assert lib.gnx_block_forward_typed(g._h, C.byref(self.cp), L.ELEM_BF16, *map(_ptr, self.ins), R, *map(_ptr, self.outs), ws.data_ptr(), ws.numel(), 0,
                                           _stream()) == 0, lib.gnx_last_error()
        self.cots = [None if o is None else torch.from_numpy(rng.standard_normal(tuple(o.shape)).astype(np.float32)).cuda().to(torch.bfloat16)
                     for o in self.outs]
        torch.cuda.synchronize()
        for o in self.outs:
            assert o is None or bool(torch.isfinite(o.float()).all())

    def nine(self, cots=(True, True, True)):
        return self.ins + self.outs + [c if keep else None for c, keep in zip(self.cots, cots)]

    def grad_shapes(self):
        """[(dW shape, db shape)] per function: the weight gradient in the (out x in) column-major layout = an (in, out) array"""
        return [(tuple(reversed(self.p[w].shape)), self.p[b].shape) for w, b in (("We", "be"), ("Wn", "bn"), ("Wg", "bg"))]

    def backward(self, elem, nine, want_d=(True, True, True), want_g=(True,) * 6, grads_null=False, ws_fill=0xA5):
        """one backward call in element type `elem` on `nine` (tensors of that type): (d_ef, d_nf, d_gf), [dWe, dbe, dWn, dbn, dWg, dbg] — None
        where not wanted; every output starts as NaN bytes"""
        import torch
        gn, g, R = self.gn, self.g, self.R
        lib, L = gn._lib.load(), gn._lib
        dt = torch.bfloat16 if elem == L.ELEM_BF16 else torch.float32
        nan = lambda shape, dtype: torch.full(shape, float("nan"), dtype=dtype, device="cuda")
        d = [nan((R, T, w), dt) if (w > 0 and keep) else None for T, w, keep in zip(self.rows, self.in_dims, want_d)]
        flat = [s for pair in self.grad_shapes() for s in pair]
        gs = [nan(tuple(s), torch.float32) if keep and int(np.prod(s)) > 0 else None for s, keep in zip(flat, want_g)]
        grads = L.BlockGrads(*[L.DenseGrad(_ptr(gs[2 * i]), _ptr(gs[2 * i + 1])) for i in range(3)])
        if elem == L.ELEM_BF16:
            nb = int(lib.gnx_block_backward_typed_workspace_bytes(g._h, C.byref(self.cp), R, elem))
        else:
            nb = int(lib.gnx_block_backward_workspace_bytes(g._h, C.byref(self.cp), R))
        assert nb > 0, lib.gnx_last_error()
        ws = torch.full((nb,), ws_fill, dtype=torch.uint8, device="cuda")
        gp = None if grads_null else C.byref(grads)
        if elem == L.ELEM_BF16:
            rc = lib.gnx_block_backward_typed(g._h, C.byref(self.cp), elem, *map(_ptr, nine), R, *map(_ptr, d), gp, ws.data_ptr(), ws.numel(), _stream())
        else:
            rc = lib.gnx_block_backward(g._h, C.byref(self.cp), *map(_ptr, nine), R, *map(_ptr, d), gp, ws.data_ptr(), ws.numel(), _stream())
        assert rc == 0, lib.gnx_last_error()
        torch.cuda.synchronize()
        return d, (gs if not grads_null else [None] * 6)

    def check(self, what, cots=(True, True, True), want_d=(True, True, True), want_g=(True,) * 6, grads_null=False):
        """typed bf16 call == the fp32 entry on the widened nine, input gradients rounded"""
        import torch
        L = self.gn._lib
        nine = self.nine(cots)
        d_ref, g_ref = self.backward(L.ELEM_F32, [None if t is None else t.float() for t in nine], want_d, want_g, grads_null)
        d, gs = self.backward(L.ELEM_BF16, nine, want_d, want_g, grads_null)
        for name, a, b in zip(("d_ef", "d_nf", "d_gf"), d, d_ref):
            _same(a, None if b is None else b.to(torch.bfloat16), f"{what} {name}")
            assert a is None or a.numel() == 0 or bool(torch.isfinite(a.float()).all()), f"{what} {name}: not finite"
        for name, a, b in zip(("dWe", "dbe", "dWn", "dbn", "dWg", "dbg"), gs, g_ref):
            _same(a, b, f"{what} {name}")
        return d, gs


def _seed(*key):
    return zlib.crc32(repr(key).encode())  # (the same in every process, unlike hash())


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("batch", BATCHES)
def test_bits_equal_the_fp32_backward_of_the_widened_tensors(gn, batch, dims):
    g, R = _batch(gn, batch)
    for act in ACTS:
        Case(gn, g, R, *dims, act, _seed(dims, act, BATCHES.index(batch))).check(f"{batch} {dims[0]}=>{dims[1]} act={act}")


@pytest.mark.parametrize("dims", [pytest.param(SAME, id="345"), pytest.param(WIDE, id="1053")])
@pytest.mark.parametrize("batch", ["one", "small40"])
def test_optional_arguments(gn, batch, dims):
    """every upstream gradient NULL but one, every output NULL but one, grads NULL — NULL for both the reference and the typed call"""
    g, R = _batch(gn, batch)
    c = Case(gn, g, R, *dims, (1, 2, 3), 77)
    for k in range(3):
        c.check(f"{batch} only cotangent {k}", cots=tuple(i == k for i in range(3)))
    for k in range(9):
        c.check(f"{batch} only output {k}", want_d=tuple(i == k for i in range(3)), want_g=tuple(i + 3 == k for i in range(6)))
    c.check(f"{batch} grads NULL", grads_null=True)
    c4 = Case(gn, g, R, *dims, (4, 4, 4), 78)  # gelu: the pre-activation buffers stand in for the outputs
    c4.check(f"{batch} gelu only g_gf_out", cots=(False, False, True))
    c4.check(f"{batch} gelu only d_nf", want_d=(False, True, False), want_g=(False,) * 6)


def test_f32_elem_is_gnx_block_backward(gn):
    """elem = GNX_ELEM_F32 is exactly gnx_block_backward: same workspace size, same bits"""
    import torch
    lib, L = gn._lib.load(), gn._lib
    for batch, dims in (("one", README), ("small40", WIDE)):
        g, R = _batch(gn, batch)
        c = Case(gn, g, R, *dims, (1, 2, 3), 5)
        nine = [None if t is None else t.float() * 1.001 for t in c.nine()]  # (fp32 values that are no bf16 values)
        assert lib.gnx_block_backward_typed_workspace_bytes(g._h, C.byref(c.cp), R, L.ELEM_F32) == lib.gnx_block_backward_workspace_bytes(g._h, C.byref(c.cp), R)
        d_ref, g_ref = c.backward(L.ELEM_F32, nine)
        d = [None if t is None else torch.full_like(t, float("nan")) for t in d_ref]
        gs = [None if t is None else torch.full_like(t, float("nan")) for t in g_ref]
        grads = L.BlockGrads(*[L.DenseGrad(_ptr(gs[2 * i]), _ptr(gs[2 * i + 1])) for i in range(3)])
        ws = torch.empty(int(lib.gnx_block_backward_workspace_bytes(g._h, C.byref(c.cp), R)), dtype=torch.uint8, device="cuda")
        assert lib.gnx_block_backward_typed(g._h, C.byref(c.cp), L.ELEM_F32, *map(_ptr, nine), R, *map(_ptr, d), C.byref(grads), ws.data_ptr(), ws.numel(),
                                            _stream()) == 0, lib.gnx_last_error()
        torch.cuda.synchronize()
        for a, b in zip(d + gs, d_ref + g_ref):
            _same(a, b, f"{batch} f32")


def test_bad_arguments_on_a_real_handle(gn):
    """what gnx_block_backward refuses, the typed entry refuses with the same code; bf16 buffers must be 4-byte aligned"""
    import torch
    lib, L = gn._lib.load(), gn._lib
    g, R = _batch(gn, "one")
    c = Case(gn, g, R, *README, (0, 0, 0), 6)
    nine = c.nine()
    d = [torch.empty_like(t) if t is not None else None for t in c.ins]
    ws = torch.empty(int(lib.gnx_block_backward_typed_workspace_bytes(g._h, C.byref(c.cp), R, L.ELEM_BF16)), dtype=torch.uint8, device="cuda")
    call = lambda nine, R=R, d=d, nbytes=ws.numel(), wsp=ws.data_ptr(): lib.gnx_block_backward_typed(
        g._h, C.byref(c.cp), L.ELEM_BF16, *map(_ptr, nine), R, *map(_ptr, d), None, wsp, nbytes, _stream())
    assert call(nine) == 0, lib.gnx_last_error()
    assert call(nine, R=0) == L.ERR_INVALID_ARG and call(nine, R=65536) == L.ERR_INVALID_ARG
    assert call([None] + nine[1:]) == L.ERR_INVALID_ARG          # ef NULL with de > 0
    assert call(nine[:4] + [None] + nine[5:]) == L.ERR_INVALID_ARG  # nf_out NULL with on > 0
    assert call(nine, nbytes=ws.numel() - 1) == L.ERR_WORKSPACE
    assert call(nine, wsp=None) == L.ERR_WORKSPACE
    odd = torch.empty(c.ins[1].numel() + 1, dtype=torch.bfloat16, device="cuda")[1:]
    assert odd.data_ptr() % 4 == 2
    assert call([nine[0], odd] + nine[2:]) == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error()
    assert call(nine, d=[d[0], odd, None]) == L.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error()
    torch.cuda.synchronize()


def _profiled_names(gn, f):
    gn.profile_reset(); gn.profile_enable(True)
    try:
        f()
    finally:
        gn.profile_enable(False)
    names = set(gn.profile_read()); gn.profile_reset()
    return names


def test_which_path_ran(gn):
    """README widths never widen (the kernels read bf16 themselves) and need only the d_gf staging on top of the fp32 workspace; matrix-core
    widths at >= 64 rows convert around the fp32 backward; the same widths on 9 edges are native again"""
    lib, L = gn._lib.load(), gn._lib
    align256 = lambda n: (n + 255) // 256 * 256
    for batch in ("one", "one-R3"):
        g, R = _batch(gn, batch)
        for dims in (README, SAME):
            c = Case(gn, g, R, *dims, (1, 2, 3), 9)
            names = _profiled_names(gn, lambda: c.check(f"profiled {batch} {dims}"))
            assert "k_bf16_widen" not in names, names
            assert {"bw_fn_inputs", "bw_delta_edge", "bw_dx_generic", "bw_dw_generic", "bw_dnf"} <= names, names
            if dims[0][2] > 0:
                assert {"bw_dgf", "k_bf16_round"} <= names, names  # (d_gf: summed in fp32, rounded once)
            typed = lib.gnx_block_backward_typed_workspace_bytes(g._h, C.byref(c.cp), R, L.ELEM_BF16)
            plain = lib.gnx_block_backward_workspace_bytes(g._h, C.byref(c.cp), R)
            assert plain <= typed <= plain + align256(4 * R * g.n_graphs * dims[0][2]) + 256, (typed, plain)
    g, R = _batch(gn, "one")
    c = Case(gn, g, R, *WIDE, (1, 2, 3), 10)
    names = _profiled_names(gn, lambda: c.check("profiled staging"))
    assert "k_bf16_widen" in names and "k_bf16_round" in names, names
    g, R = _batch(gn, "tiny")
    c = Case(gn, g, R, *WIDE, (1, 2, 3), 11)
    names = _profiled_names(gn, lambda: c.check("profiled tiny"))
    assert "k_bf16_widen" not in names, names
    typed = lib.gnx_block_backward_typed_workspace_bytes(g._h, C.byref(c.cp), R, L.ELEM_BF16)
    plain = lib.gnx_block_backward_workspace_bytes(g._h, C.byref(c.cp), R)
    assert plain <= typed <= plain + align256(4 * R * g.n_graphs * 3) + 256, (typed, plain)


@pytest.mark.parametrize("dims", [pytest.param(README, id="readme"), pytest.param(SAME, id="345"), pytest.param(WIDE, id="1053-staging")])
def test_memory_contract(gn, dims):
    """Twelve tensors, six parameter gradients and the workspace at their exact byte sizes inside one sentinel arena: nothing outside an
    output or the workspace is written, inputs are unchanged, every output element is written, and the outputs do not depend on what the
    workspace held."""
    import torch
    lib, L = gn._lib.load(), gn._lib
    g, R = _batch(gn, "one")
    c = Case(gn, g, R, *dims, (1, 2, 3), 12)
    a = Arena("cuda")
    names = ("ef", "nf", "gf", "ef_out", "nf_out", "gf_out", "g_ef_out", "g_nf_out", "g_gf_out")
    nine = [a.input(n, t) if t is not None else None for n, t in zip(names, c.nine())]
    dx = [a.output(n, t.shape, torch.bfloat16) if t is not None else None for n, t in zip(("d_ef", "d_nf", "d_gf"), c.ins)]
    gnames = []
    for fn, (sw, sb) in zip(("edgefn", "nodefn", "graphfn"), c.grad_shapes()):
        gnames += [a.output(f"grad.{fn}.dW", sw), a.output(f"grad.{fn}.db", sb)]
    ws = a.workspace("ws", int(lib.gnx_block_backward_typed_workspace_bytes(g._h, C.byref(c.cp), R, L.ELEM_BF16)))
    bits = []
    for i, fill in enumerate((0x00, 0xFF)):
        if i == 0:
            a.build(ws_fill=fill)
        else:
            a.refill(fill)
        P = a.ptr
        grads = L.BlockGrads(*[L.DenseGrad(P(gnames[2 * k]), P(gnames[2 * k + 1])) for k in range(3)])
        assert lib.gnx_block_backward_typed(g._h, C.byref(c.cp), L.ELEM_BF16, *map(P, nine), R, *map(P, dx), C.byref(grads), P(ws), a.nbytes(ws),
                                            _stream()) == 0, lib.gnx_last_error()
        torch.cuda.synchronize()
        a.check(f"{dims} ws_fill={fill:#x}")
        bits.append(a.output_bits())
    for n in bits[0]:
        assert torch.equal(bits[0][n], bits[1][n]), f"{n} depends on what the workspace held"
    # and they are the bits of the plain case
    d, gs = c.check("arena reference")
    for n, t in zip(dx + gnames, d + gs):
        if n is not None:
            assert torch.equal(a.raw(n), t.contiguous().view(-1).view(torch.uint8)), n


# ---- Python ----
def _py_batch(gn, seed, sizes, dtype):
    rng = np.random.default_rng(seed)
    adjs = U.random_graphs(rng, sizes, 0.4)
    efs = [(rng.random((10, int((adj == 1).sum())), dtype=np.float32) * 2 - 1) for adj in adjs]
    nfs = [(rng.random((5, adj.shape[0]), dtype=np.float32) * 2 - 1) for adj in adjs]
    return gn.batch(dict(graphs=adjs, ef=efs, nf=nfs, gf=None), dtype=dtype), rng


def test_python_autograd_matches_the_abi(gn):
    import torch
    lib, L = gn._lib.load(), gn._lib
    x, rng = _py_batch(gn, 21, (6, 9, 4, 1), torch.bfloat16)
    blk = U.block_from_params(gn, O.make_block_params(rng, *README, act=(1, 2, 0)))
    params = [blk.edgefn.weight, blk.edgefn.bias, blk.nodefn.weight, blk.nodefn.bias, blk.graphfn.weight, blk.graphfn.bias]
    for t in params:
        t.requires_grad_(True)
    ef, nf = x.ef.detach().requires_grad_(True), x.nf.detach().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="bf16_backward"):  # the switch is off
        blk(gn.NT(x.graphs, ef, nf, None))
    blk.bf16_backward = True
    y = blk(gn.NT(x.graphs, ef, nf, None))
    assert all(t.dtype == torch.bfloat16 and t.requires_grad for t in (y.ef, y.nf, y.gf))
    # cotangents that are bf16 values: d(sum(y.float() * c)) / dy = c exactly
    cot = [torch.from_numpy(rng.standard_normal(tuple(t.shape)).astype(np.float32)).cuda().to(torch.bfloat16) for t in (y.ef, y.nf, y.gf)]
    sum((t.float() * c.float()).sum() for t, c in zip((y.ef, y.nf, y.gf), cot)).backward()
    assert ef.grad.dtype == torch.bfloat16 and nf.grad.dtype == torch.bfloat16 and ef.grad.shape == ef.shape
    assert all(t.grad is not None and t.grad.dtype == torch.float32 and t.grad.shape == t.shape for t in params)
    # the direct ABI call on the same (packed) tensors
    pk = lambda t: None if t is None else t.detach().permute(2, 1, 0).contiguous()
    g = x.graphs
    keep = []
    cp = blk._c(keep)
    nine = [pk(ef), pk(nf), None, pk(y.ef), pk(y.nf), pk(y.gf)] + [pk(c) for c in cot]
    d = [torch.empty_like(nine[0]), torch.empty_like(nine[1]), None]
    gs = []
    for l in (blk.edgefn, blk.nodefn, blk.graphfn):
        gs += [torch.empty((l.weight.shape[1], l.weight.shape[0]), dtype=torch.float32, device="cuda"), torch.empty_like(l.bias)]
    grads = L.BlockGrads(*[L.DenseGrad(_ptr(gs[2 * i]), _ptr(gs[2 * i + 1])) for i in range(3)])
    ws = torch.empty(int(lib.gnx_block_backward_typed_workspace_bytes(g._h, C.byref(cp), 1, L.ELEM_BF16)), dtype=torch.uint8, device="cuda")
    assert lib.gnx_block_backward_typed(g._h, C.byref(cp), L.ELEM_BF16, *map(_ptr, nine), 1, *map(_ptr, d), C.byref(grads), ws.data_ptr(), ws.numel(),
                                        _stream()) == 0, lib.gnx_last_error()
    torch.cuda.synchronize()
    _same(pk(ef.grad), d[0], "x.ef.grad")
    _same(pk(nf.grad), d[1], "x.nf.grad")
    for name, t, w in zip(("We", "be", "Wn", "bn", "Wg", "bg"), params, gs):
        _same(t.grad.t().contiguous() if t.dim() == 2 else t.grad, w, f"grad {name}")
    # only the features need a gradient: no parameter gradient is computed, the input gradients are the same bits
    for t in params:
        t.requires_grad_(False)
    ef2 = x.ef.detach().requires_grad_(True)
    y2 = blk(gn.NT(x.graphs, ef2, x.nf, None))
    sum((t.float() * c.float()).sum() for t, c in zip((y2.ef, y2.nf, y2.gf), cot)).backward()
    _same(pk(ef2.grad), d[0], "features only: x.ef.grad")


def _train(gn, steps=50):
    import torch
    x, rng = _py_batch(gn, 31, (5, 40, 17, 8, 33, 12), torch.bfloat16)
    blk = U.block_from_params(gn, O.make_block_params(rng, *README, act=(2, 2, 0)))
    blk.bf16_backward = True
    params = [blk.edgefn.weight, blk.edgefn.bias, blk.nodefn.weight, blk.nodefn.bias, blk.graphfn.weight, blk.graphfn.bias]
    for t in params:
        t.requires_grad_(True)
    g = x.graphs
    target = [torch.from_numpy(rng.standard_normal((d, T, 1)).astype(np.float32)).cuda() for d, T in zip((3, 4, 5), (g.n_edges, g.n_nodes, g.n_graphs))]
    opt = torch.optim.AdamW(params, lr=1e-2)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        y = blk(x)
        loss = sum(((o.float() - t) ** 2).mean() for o, t in zip((y.ef, y.nf, y.gf), target))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def test_fifty_adamw_steps_reduce_the_loss_and_repeat_exactly(gn):
    a, b = _train(gn), _train(gn)
    assert all(np.isfinite(a))
    assert a[-1] < a[0], (a[0], a[-1])
    assert a == b  # the kernels are deterministic
