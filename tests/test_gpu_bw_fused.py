"""gnx_block_backward_fused on the GPU.  Reference of the bits: gnx_block_backward on the same nine fp32 tensors — d_ef, d_nf, d_gf and the
node / graph parameter gradients must be its bits; the edge function's weight / bias gradient, summed in another fixed order, is compared with
torch float64 autograd at the bar of tests/test_gpu_backward.py (max|got - ref| <= 2e-4 max(1, max|ref|)); two fused runs give the same bits.
Shapes are the smallest at which k_bw_edge_wave can go wrong: several chunks per tile, a single-node tile above the edge cap, nodes without
in-edges, self-loops, graphs without edges, more than 256 wave tiles, and (the partial rows are per workgroup of four tiles) more than 256
partial rows with four replicas."""
import ctypes as C
import zlib

import numpy as np
import pytest

from oracle import gn_oracle as O
from tests import util as U
from tests.arena import Arena, WORKSPACE
from tests.test_gpu_backward import _kink_free, _torch_block

pytestmark = pytest.mark.gpu

README = ((10, 5, 0), (3, 4, 5))
SETS = [pytest.param(README, id="1050"), pytest.param(((3, 4, 5), (3, 4, 5)), id="345"), pytest.param(((0, 2, 0), (2, 2, 2)), id="020"),
        pytest.param(((2, 2, 2), (2, 2, 2)), id="222"), pytest.param(((4, 3, 2), (3, 4, 5)), id="432")]
ACTS = ((0, 0, 0), (2, 3, 2), (3, 2, 3), (1, 2, 3))  # identity / tanh / sigmoid / relu on the edges (relu: kink-free draws)
GRAPHS = ["e20k", "n20k", "degrees", "small40", "edgeless"]
NAMES = ("d_ef", "d_nf", "d_gf", "dWe", "dbe", "dWn", "dbn", "dWg", "dbg")


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


def _degrees_csc():
    """260 nodes: in-degree 128, 129 and 200 at nodes 3, 7 and 11 (exactly two chunks, two chunks and one edge, four chunks — the last two above
    a wave tile's edge cap of 128: single-node tiles), self-loops at every fifth node, one or two in-edges elsewhere, none at nodes 20..59"""
    N = 260
    rng = np.random.default_rng(5)
    srcs = [[] for _ in range(N)]
    for n, deg in ((3, 128), (7, 129), (11, 200)):
        srcs[n] = sorted(rng.choice(N, deg, replace=False).tolist())
    for n in range(N):
        if srcs[n] or 20 <= n < 60:
            continue
        s = set(rng.choice(N, 1 + n % 2, replace=False).tolist())
        if n % 5 == 0:
            s.add(n)
        srcs[n] = sorted(s)
    colptr = np.zeros(N + 1, dtype=np.int64)
    colptr[1:] = np.cumsum([len(s) for s in srcs])
    return colptr, np.array([v for s in srcs for v in s], dtype=np.int64), N


def _graph(gn, name):
    if name not in _graphs:
        if name == "e20k":
            colptr, rowval = U.er_csc(np.random.default_rng(1), 2000, 20000)
            g = gn.GNGraphBatch.from_csc([colptr], [rowval], [2000])
        elif name == "n20k":
            colptr, rowval = U.er_csc(np.random.default_rng(2), 20000, 30000)
            g = gn.GNGraphBatch.from_csc([colptr], [rowval], [20000])
        elif name == "degrees":
            colptr, rowval, N = _degrees_csc()
            g = gn.GNGraphBatch.from_csc([colptr], [rowval], [N])
            deg = np.diff(colptr)
            assert {128, 129, 200, 0} <= set(deg.tolist()) and any(rowval[colptr[n]:colptr[n + 1]].tolist().count(n) for n in range(N))
        elif name == "small40":
            rng = np.random.default_rng(3)
            adjs = U.random_graphs(rng, list(range(1, 41)), 0.3)
            adjs[0][:] = 0   # a single node without an edge
            adjs[11][:] = 0  # a 12-node graph without edges
            g = gn.GNGraphBatch(adjs)
        elif name == "tiny":
            colptr, rowval = U.er_csc(np.random.default_rng(4), 5, 9)
            g = gn.GNGraphBatch.from_csc([colptr], [rowval], [5])
        else:
            g = gn.GNGraphBatch([np.zeros((n, n), dtype=np.int64) for n in (3, 5, 2)])
        _graphs[name] = g
    return _graphs[name]


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _same(a, b, what):
    import torch
    assert (a is None) == (b is None), what
    if a is None:
        return
    assert a.dtype == b.dtype and a.shape == b.shape, what
    x, y = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    if not torch.equal(x, y):
        bad = (x != y).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {x.numel()} values differ, first at {i}: {a[i].item()!r} vs {b[i].item()!r}")


def _seed(*key):
    return zlib.crc32(repr(key).encode())


class Case:
    """A block, fp32 inputs, the outputs of gnx_block_forward and random cotangents: the nine tensors of a backward call"""

    def __init__(self, gn, g, R, in_dims, out_dims, act, seed):
        import torch
        self.gn, self.g, self.R, self.in_dims, self.out_dims, self.act = gn, g, R, in_dims, out_dims, act
        lib = gn._lib.load()
        self.rows = (g.n_edges, g.n_nodes, g.n_graphs)
        self.csc = (*g.csc(), g.node_off, g.edge_off)
        for attempt in range(40):  # a relu edge function: a draw whose float64 pre-activations stay clear of the kink (tests/test_gpu_backward.py)
            rng = np.random.default_rng(seed + 7919 * attempt)
            self.p = O.make_block_params(rng, in_dims, out_dims, act=act)
            self.np_ins = U.packed_inputs(rng, R, *self.rows, in_dims)
            if 1 not in act:
                break
            ok = True
            for r in range(R):
                pre = []
                _torch_block(self.p, self.csc, *[None if a is None else torch.tensor(a[r], dtype=torch.float64) for a in self.np_ins], self._leaves(False), pre)
                ok = ok and _kink_free([z for z, a in zip(pre, act) if a == 1])
            if ok:
                break
        else:
            pytest.fail("no kink-free draw in 40 attempts")
        self.blk = U.block_from_params(gn, self.p)
        self.keep = []
        self.cp = self.blk._c(self.keep)
        self.ins = [None if a is None else torch.from_numpy(a).cuda() for a in self.np_ins]
        self.outs = [torch.empty((R, T, d), dtype=torch.float32, device="cuda") if d > 0 else None for T, d in zip(self.rows, out_dims)]
        nb = int(lib.gnx_block_workspace_bytes(g._h, C.byref(self.cp), R))
        ws = torch.empty(max(nb, 256), dtype=torch.uint8, device="cuda")
        assert lib.gnx_block_forward(g._h, C.byref(self.cp), *map(_ptr, self.ins), R, *map(_ptr, self.outs), ws.data_ptr(), ws.numel(), 0, _stream()) == 0, lib.gnx_last_error()
        self.np_cots = [None if o is None else rng.standard_normal(tuple(o.shape)).astype(np.float32) for o in self.outs]
        self.cots = [None if c is None else torch.from_numpy(c).cuda() for c in self.np_cots]
        torch.cuda.synchronize()
        self.applies = int(lib.gnx_block_backward_fused_applies(g._h, C.byref(self.cp), R))

    def _leaves(self, grad=True):
        import torch
        return {k: torch.tensor(self.p[k], dtype=torch.float64, requires_grad=grad) for k in ("We", "be", "Wn", "bn", "Wg", "bg")}

    def nine(self, cots=(True, True, True)):
        return self.ins + self.outs + [c if keep else None for c, keep in zip(self.cots, cots)]

    def grad_shapes(self):
        return [(tuple(reversed(self.p[w].shape)), self.p[b].shape) for w, b in (("We", "be"), ("Wn", "bn"), ("Wg", "bg"))]

    def query(self, fused):
        lib = self.gn._lib.load()
        f = lib.gnx_block_backward_fused_workspace_bytes if fused else lib.gnx_block_backward_workspace_bytes
        return int(f(self.g._h, C.byref(self.cp), self.R))

    def backward(self, fused, nine, want_d=(True, True, True), want_g=(True,) * 6, grads_null=False, ws_fill=0xA5):
        """one call: [d_ef, d_nf, d_gf, dWe, dbe, dWn, dbn, dWg, dbg], None where not wanted; every output starts as NaN"""
        import torch
        g, R = self.g, self.R
        lib, L = self.gn._lib.load(), self.gn._lib
        nan = lambda shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
        d = [nan((R, T, w)) if (w > 0 and keep) else None for T, w, keep in zip(self.rows, self.in_dims, want_d)]
        flat = [s for pair in self.grad_shapes() for s in pair]
        gs = [nan(tuple(s)) if keep and int(np.prod(s)) > 0 else None for s, keep in zip(flat, want_g)]
        grads = L.BlockGrads(*[L.DenseGrad(_ptr(gs[2 * i]), _ptr(gs[2 * i + 1])) for i in range(3)])
        nb = self.query(fused)
        assert nb > 0, lib.gnx_last_error()
        ws = torch.full((nb,), ws_fill, dtype=torch.uint8, device="cuda")
        call = lib.gnx_block_backward_fused if fused else lib.gnx_block_backward
        rc = call(g._h, C.byref(self.cp), *map(_ptr, nine), R, *map(_ptr, d), None if grads_null else C.byref(grads), ws.data_ptr(), ws.numel(), _stream())
        assert rc == 0, lib.gnx_last_error()
        torch.cuda.synchronize()
        return d + (gs if not grads_null else [None] * 6)

    def edge_grads_f64(self, cots=(True, True, True)):
        """(dWe in the (in, out) layout of the ABI, dbe) by torch float64 autograd of the restated forward, summed over the replicas"""
        import torch
        W = self._leaves()
        loss = 0.0
        for r in range(self.R):
            outs = _torch_block(self.p, self.csc, *[None if a is None else torch.tensor(a[r], dtype=torch.float64) for a in self.np_ins], W)
            for o, c, keep, w in zip(outs, self.np_cots, cots, self.out_dims):
                if w > 0 and keep:
                    loss = loss + (o * torch.from_numpy(c[r]).double()).sum()
        if not isinstance(loss, torch.Tensor):
            return np.zeros(tuple(reversed(self.p["We"].shape))), np.zeros(self.p["be"].shape)
        loss.backward()
        zero = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
        return zero(W["We"]).T, zero(W["be"])

    def check(self, what, cots=(True, True, True), want_d=(True, True, True), want_g=(True,) * 6, grads_null=False):
        nine = self.nine(cots)
        ref = self.backward(False, nine, want_d, want_g, grads_null)
        got = self.backward(True, nine, want_d, want_g, grads_null)
        again = self.backward(True, nine, want_d, want_g, grads_null, ws_fill=0x3C)
        for name, a, b in zip(NAMES, got, again):
            _same(a, b, f"{what} {name}: two fused runs")
        f64 = None
        for i, (name, a, b) in enumerate(zip(NAMES, got, ref)):
            if i in (3, 4) and self.applies and a is not None:  # dWe, dbe: another summation order
                assert b is not None
                f64 = f64 or self.edge_grads_f64(cots)
                r = f64[i - 3]
                err = float(np.max(np.abs(a.double().cpu().numpy() - r)))
                scale = max(1.0, float(np.abs(r).max()))
                print(f"{what} {name}: max err {err:.3e}, bar {2e-4 * scale:.3e}")
                assert err <= 2e-4 * scale, f"{what} {name}: max err {err:.3e} (scale {scale:.3g})"
            else:
                _same(a, b, f"{what} {name}")
        return got


@pytest.mark.parametrize("dims", SETS)
@pytest.mark.parametrize("graph", GRAPHS)
def test_bits_of_the_generic_backward_and_edge_gradients_at_the_bar(gn, graph, dims):
    g = _graph(gn, graph)
    for act in ACTS:
        c = Case(gn, g, 1, *dims, act, _seed(dims, act, graph))
        assert c.applies == (0 if graph == "edgeless" else 1), (graph, dims)
        c.check(f"{graph} {dims[0]}=>{dims[1]} act={act}")


@pytest.mark.parametrize("graph,R", [("e20k", 2), ("e20k", 3), ("n20k", 4)], ids=["R2", "R3", "R4-more-than-256-partial-rows"])
def test_replicas(gn, graph, R):
    g = _graph(gn, graph)
    for dims in (README, ((3, 4, 5), (3, 4, 5))):
        c = Case(gn, g, R, *dims, (2, 3, 0), _seed("rep", R, dims))
        assert c.applies == 1
        c.check(f"{graph} R={R} {dims}")


@pytest.mark.parametrize("graph", ["degrees", "small40"])
def test_optional_arguments(gn, graph):
    """each upstream gradient absent in turn, each output absent in turn (the edge weight gradient alone, the edge bias gradient alone), grads
    NULL; a block without node outputs and one without graph outputs"""
    g = _graph(gn, graph)
    c = Case(gn, g, 1, (3, 4, 5), (3, 4, 5), (1, 2, 3), 77)
    for k in range(3):
        c.check(f"{graph} without cotangent {k}", cots=tuple(i != k for i in range(3)))
    c.check(f"{graph} without any cotangent", cots=(False, False, False))
    for k in range(3):
        c.check(f"{graph} without d[{k}]", want_d=tuple(i != k for i in range(3)))
    c.check(f"{graph} no input gradient", want_d=(False, False, False))
    c.check(f"{graph} grads NULL", grads_null=True)
    c.check(f"{graph} dWe alone", want_g=(True, False, False, False, False, False))
    c.check(f"{graph} dbe alone", want_g=(False, True, False, False, False, False))
    c.check(f"{graph} no edge gradient", want_g=(False, False, True, True, True, True))
    c.check(f"{graph} dWe alone, no input gradient", want_d=(False, False, False), want_g=(True, False, False, False, False, False))
    for out in ((3, 0, 5), (3, 4, 0), (3, 0, 0)):  # on = 0, og = 0, both
        c2 = Case(gn, g, 1, (10, 5, 0), out, (2, 2, 2), 78)
        assert c2.applies == 1
        c2.check(f"{graph} => {out}")
        c3 = Case(gn, g, 1, (4, 3, 2), out, (3, 3, 3), 79)
        c3.check(f"{graph} (4,3,2) => {out}")


def test_where_it_does_not_apply_it_is_the_generic_backward(gn):
    """a gelu edge function, a width set outside the list, matrix-core widths above 64 rows, a batch without edges: applies == 0, the bits of
    gnx_block_backward in every output, the generic workspace size"""
    for graph, dims, act in (("degrees", README, (4, 0, 0)), ("degrees", ((3, 2, 4), (3, 4, 5)), (1, 2, 3)), ("degrees", ((10, 5, 0), (4, 4, 5)), (0, 0, 0)),
                             ("degrees", ((10, 5, 3), (3, 4, 5)), (2, 2, 2)), ("small40", ((10, 5, 3), (3, 4, 5)), (0, 0, 0)), ("edgeless", README, (2, 2, 2))):
        c = Case(gn, _graph(gn, graph), 1, *dims, act, 5)
        assert c.applies == 0, (graph, dims, act)
        assert c.query(True) == c.query(False)
        c.check(f"not applicable: {graph} {dims} {act}")
        c.check(f"not applicable: {graph} {dims} {act}, d_nf alone", want_d=(False, True, False), want_g=(False,) * 6)
    # the same handle, the same widths, but a gelu NODE function: the edge level is still fused
    assert Case(gn, _graph(gn, "degrees"), 1, *README, (2, 4, 4), 6).applies == 1


def _profiled(gn, f):
    gn.profile_reset(); gn.profile_enable(True)
    try:
        f()
    finally:
        gn.profile_enable(False)
    out = gn.profile_read(); gn.profile_reset()
    return out


def test_launch_structure(gn):
    """against the generic call: no Xe launch (one kernel fewer under bw_fn_inputs), no edge dX launch, the fused kernel under bw_delta_edge"""
    if U.default_flags(gn) != 0:
        return  # (forms switched on for the whole process change which kernels run, not the bits)
    for graph, R in (("e20k", 1), ("e20k", 2), ("small40", 1)):
        c = Case(gn, _graph(gn, graph), R, *README, (1, 2, 3), 9)
        nine = c.nine()
        gen = _profiled(gn, lambda: c.backward(False, nine))
        fus = _profiled(gn, lambda: c.backward(True, nine))
        assert set(fus) <= set(gen), (sorted(fus), sorted(gen))  # no new profiler name
        assert fus["bw_fn_inputs"]["kernels"] == gen["bw_fn_inputs"]["kernels"] - 1, (fus["bw_fn_inputs"], gen["bw_fn_inputs"])
        assert fus["bw_dx_generic"]["launches"] == gen["bw_dx_generic"]["launches"] - 1, (fus["bw_dx_generic"], gen["bw_dx_generic"])
        assert fus["bw_delta_edge"]["kernels"] == gen["bw_delta_edge"]["kernels"] == 1
        assert fus["bw_dw_generic"]["kernels"] == gen["bw_dw_generic"]["kernels"] - 1  # the edge level: the final reduction only
        for name in ("bw_dnf", "bw_dgf"):
            assert (name in fus) == (name in gen) and (name not in gen or fus[name]["kernels"] == gen[name]["kernels"]), name


@pytest.mark.parametrize("dims", SETS)
def test_workspace(gn, dims):
    """smaller than the generic workspace by at least the Xe region on the two larger graphs; one byte less than the query is refused with
    nothing written; (Case.check runs the fused call on workspaces filled with 0xA5 and 0x3C, here 0x00 and 0xFF: the bits do not depend on it)"""
    import torch
    lib, L = gn._lib.load(), gn._lib
    for graph, R in (("e20k", 1), ("e20k", 3), ("n20k", 1)):
        c = Case(gn, _graph(gn, graph), R, *dims, (2, 2, 2), 12)
        ke = dims[0][0] + 2 * dims[0][1] + dims[0][2]
        fused, generic = c.query(True), c.query(False)
        print(f"{graph} R={R} {dims}: fused {fused} B, generic {generic} B, Xe {4 * R * c.g.n_edges * ke} B")
        assert fused <= generic - 4 * R * c.g.n_edges * ke, (fused, generic)
        nine = c.nine()
        a, b = c.backward(True, nine, ws_fill=0x00), c.backward(True, nine, ws_fill=0xFF)
        for name, x, y in zip(NAMES, a, b):
            _same(x, y, f"{name} depends on what the workspace held")
        outs = [None if t is None else torch.full_like(t, float("nan")) for t in a]
        d, gs = outs[:3], outs[3:]
        grads = L.BlockGrads(*[L.DenseGrad(_ptr(gs[2 * i]), _ptr(gs[2 * i + 1])) for i in range(3)])
        ws = torch.full((fused,), 0x5A, dtype=torch.uint8, device="cuda")
        rc = lib.gnx_block_backward_fused(c.g._h, C.byref(c.cp), *map(_ptr, nine), R, *map(_ptr, d), C.byref(grads), ws.data_ptr(), fused - 1, _stream())
        assert rc == L.ERR_WORKSPACE and b"gnx_block_backward_fused_workspace_bytes" in lib.gnx_last_error()
        assert lib.gnx_block_backward_fused(c.g._h, C.byref(c.cp), *map(_ptr, nine), R, *map(_ptr, d), C.byref(grads), None, fused, _stream()) == L.ERR_WORKSPACE
        torch.cuda.synchronize()
        assert bool((ws == 0x5A).all()) and all(bool(torch.isnan(t).all()) for t in outs if t is not None)


@pytest.mark.parametrize("dims", SETS)
def test_arena_memory_contract_and_skewed_addresses(gn, dims):
    """Every buffer of the call at its exact byte size inside one sentinel arena, aligned and 4 / 8 / 12 bytes behind a 256-byte boundary:
    nothing outside the outputs and the workspace is written, the inputs are untouched, every requested output element is written, and the skewed
    runs give the bits of the aligned run — the kernel has one form."""
    import torch
    lib, L = gn._lib.load(), gn._lib
    g, R = _graph(gn, "degrees"), 1
    c = Case(gn, g, R, *dims, (1, 2, 3), 13)
    a = Arena("cuda")
    names = ("ef", "nf", "gf", "ef_out", "nf_out", "gf_out", "g_ef_out", "g_nf_out", "g_gf_out")
    nine = [a.input(n, t) if t is not None else None for n, t in zip(names, c.nine())]
    dx = [a.output(n, t.shape) if t is not None else None for n, t in zip(("d_ef", "d_nf", "d_gf"), c.ins)]
    gnames = []
    for fn, (sw, sb) in zip(("edgefn", "nodefn", "graphfn"), c.grad_shapes()):
        gnames += [a.output(f"grad.{fn}.dW", sw), a.output(f"grad.{fn}.db", sb)]
    ws = a.workspace("ws", c.query(True))
    a.build(ws_fill=0x00)

    def run():
        keep = []
        cp = c.blk._c(keep)
        grads = L.BlockGrads(*[L.DenseGrad(a.ptr(gnames[2 * k]), a.ptr(gnames[2 * k + 1])) for k in range(3)])
        rc = lib.gnx_block_backward_fused(g._h, C.byref(cp), *map(a.ptr, nine), R, *map(a.ptr, dx), C.byref(grads), a.ptr(ws), a.nbytes(ws), _stream())
        torch.cuda.synchronize()
        return rc

    assert run() == 0, lib.gnx_last_error()
    a.check(f"{dims} aligned")
    base = a.output_bits()
    ref = c.check("arena reference")
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
    c = Case(gn, _graph(gn, "e20k"), 1, *README, (1, 2, 3), 14)
    nine = c.nine()
    eager = c.backward(True, nine)  # (the query ran here: outside the capture)
    outs = [None if t is None else torch.zeros_like(t) for t in eager]
    grads = L.BlockGrads(*[L.DenseGrad(_ptr(outs[3 + 2 * i]), _ptr(outs[4 + 2 * i])) for i in range(3)])
    ws = torch.empty(c.query(True), dtype=torch.uint8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            assert lib.gnx_block_backward_fused(c.g._h, C.byref(c.cp), *map(_ptr, nine), 1, *map(_ptr, outs[:3]), C.byref(grads), ws.data_ptr(), ws.numel(),
                                                s.cuda_stream) == 0, lib.gnx_last_error()
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES, outs, eager):
        _same(x, y, f"captured {name}")


# ---- Python ----
def _py_case(gn, fused, seed=21):
    import torch
    rng = np.random.default_rng(seed)
    colptr, rowval = U.er_csc(rng, 300, 2500)
    g = gn.GNGraphBatch.from_csc([colptr], [rowval], [300])
    blk = U.block_from_params(gn, O.make_block_params(rng, *README, act=(2, 2, 0)))
    blk.fused_backward = fused
    params = [blk.edgefn.weight, blk.edgefn.bias, blk.nodefn.weight, blk.nodefn.bias, blk.graphfn.weight, blk.graphfn.bias]
    for t in params:
        t.requires_grad_(True)
    ef, nf, _ = U.packed_inputs(rng, 1, 2500, 300, 1, README[0])
    x = U.to_nt(gn, g, ef, nf, None)
    target = torch.from_numpy(rng.random((4, 300), dtype=np.float32)).to(g.device)
    return blk, params, x, target


def test_python_autograd_with_the_switch(gn):
    """GNBlock(..., fused_backward=True) under torch.autograd: the input gradients are the bits of the same block with the switch off, the node
    and graph parameter gradients too, the edge function's within the bar; a few Adam steps reduce a loss"""
    import torch
    res = []
    for fused in (False, True):
        blk, params, x, target = _py_case(gn, fused)
        assert blk.fused_backward is fused
        ef, nf = x.ef.detach().requires_grad_(True), x.nf.detach().requires_grad_(True)
        y = blk(gn.NT(x.graphs, ef, nf, None))
        (((y.nf[:, :, 0] - target) ** 2).mean() + 1e-3 * (y.gf ** 2).mean() + 1e-2 * (y.ef ** 2).mean()).backward()
        res.append([ef.grad, nf.grad] + [t.grad for t in params])
    for i, (name, a, b) in enumerate(zip(("x.ef", "x.nf", "We", "be", "Wn", "bn", "Wg", "bg"), *res)):
        if i in (2, 3):
            err, scale = float((a.double() - b.double()).abs().max()), max(1.0, float(a.double().abs().max()))
            assert err <= 2e-4 * scale, (name, err, scale)
        else:
            _same(a.contiguous(), b.contiguous(), f"grad {name}")
    blk, params, x, target = _py_case(gn, True)

    def loss_fn():
        y = blk(x)
        return ((y.nf[:, :, 0] - target) ** 2).mean() + 1e-6 * (y.gf ** 2).mean() + 1e-3 * (y.ef ** 2).mean()

    first = float(loss_fn().detach())
    opt = torch.optim.Adam(params, lr=1e-2)
    for _ in range(60):
        opt.zero_grad()
        loss_fn().backward()
        opt.step()
    last = float(loss_fn().detach())
    assert np.isfinite(last) and last < 0.7 * first, (first, last)
