"""bfloat16 features through gnx_block_forward_typed on the GPU.  Every case is bit for bit bf16(gnx_block_forward(widened inputs)) under the
same flags — the native fused kernels (ahead of time and run-time specialised), and the paths that convert around the fp32 forward — and
every output is written without touching a byte outside it (64 B of sentinel on both sides)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle import gn_oracle as O
from tests import util as U

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0xA5
FORCE_GENERIC, NO_JIT = 0x1, 0x8000


@pytest.fixture(scope="module")
def gn():
    import torch
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


def _guarded(R, T, d):
    """a bf16 (R, T, d) tensor inside a byte buffer with GUARD sentinel bytes on both sides (start 64-B aligned)"""
    import torch
    n = R * T * d * 2
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(torch.bfloat16).view(R, T, d)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bf16_inputs(rng, R, g, dims):
    import torch
    ef, nf, gf = U.packed_inputs(rng, R, g.n_edges, g.n_nodes, g.n_graphs, dims)
    # values of both signs over a few binades, then rounded once to bf16 (the inputs ARE bf16)
    mk = lambda a: None if a is None else torch.from_numpy((a * 4 - 2).astype(np.float32)).cuda().to(torch.bfloat16).contiguous()
    return mk(ef), mk(nf), mk(gf)


def _forward_pair(gn, blk, g, R, flags, ef, nf, gf):
    """(bf16 outputs of the typed call, bf16(fp32 outputs of gnx_block_forward on the widened inputs)); checks the guards"""
    import torch
    lib = gn._lib.load()
    L = gn._lib
    keep = []
    p = blk._c(keep)
    oe, on, og = blk.out_dims
    rows = (g.n_edges, g.n_nodes, g.n_graphs)
    stream = torch.cuda.current_stream().cuda_stream
    w = [None if a is None else a.float() for a in (ef, nf, gf)]
    outs32 = [torch.empty((R, T, d), dtype=torch.float32, device="cuda") if d > 0 else None for T, d in zip(rows, (oe, on, og))]
    ws32 = torch.empty(max(int(lib.gnx_block_workspace_bytes(g._h, C.byref(p), R)), 256), dtype=torch.uint8, device="cuda")
    assert lib.gnx_block_forward(g._h, C.byref(p), *map(_ptr, w), R, *map(_ptr, outs32), ws32.data_ptr(), ws32.numel(), flags, stream) == 0, \
        lib.gnx_last_error()
    guarded = [_guarded(R, T, d) if d > 0 else (None, None) for T, d in zip(rows, (oe, on, og))]
    outs = [o for _, o in guarded]
    nb = int(lib.gnx_block_typed_workspace_bytes(g._h, C.byref(p), R, L.ELEM_BF16, flags))
    assert nb > 0, lib.gnx_last_error()
    ws = torch.full((nb,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert lib.gnx_block_forward_typed(g._h, C.byref(p), L.ELEM_BF16, _ptr(ef), _ptr(nf), _ptr(gf), R, *map(_ptr, outs), ws.data_ptr(), ws.numel(),
                                       flags, stream) == 0, lib.gnx_last_error()
    torch.cuda.synchronize()
    for buf, o in guarded:
        if buf is not None:
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + o.numel() * 2:] == SENTINEL).all()), "a store left its output"
    refs = [None if o is None else o.to(torch.bfloat16) for o in outs32]
    return outs, refs, outs32


def _assert_bits(outs, refs, what=""):
    import torch
    for name, o, r in zip(("ef'", "nf'", "gf'"), outs, refs):
        assert (o is None) == (r is None), name
        if o is None:
            continue
        a, b = o.view(torch.int16), r.view(torch.int16)
        if not torch.equal(a, b):
            bad = (a != b).nonzero()
            raise AssertionError(f"{what} {name}: {bad.shape[0]} of {a.numel()} values differ, first at {tuple(bad[0].tolist())}: "
                                 f"{o[tuple(bad[0])].item()} vs {r[tuple(bad[0])].item()}")


def _case(gn, g, in_dims, out_dims, R=1, flags=0, seed=0, act=(1, 0, 2)):
    rng = np.random.default_rng(seed)
    p = O.make_block_params(rng, in_dims, out_dims, act=act)
    blk = U.block_from_params(gn, p)
    ef, nf, gf = _bf16_inputs(rng, R, g, in_dims)
    outs, refs, _ = _forward_pair(gn, blk, g, R, flags, ef, nf, gf)
    _assert_bits(outs, refs, f"{in_dims}=>{out_dims} R={R} flags={flags:#x}")
    return p, (ef, nf, gf), outs


def _one_graph(gn, N=2000, E=20000, seed=1):
    colptr, rowval = U.er_csc(np.random.default_rng(seed), N, E)
    return gn.GNGraphBatch.from_csc([colptr], [rowval], [N])


def _small_graphs(gn, seed=2, n=40):
    rng = np.random.default_rng(seed)
    return gn.GNGraphBatch(U.random_graphs(rng, list(rng.integers(3, 40, n)), 0.3))


DIMS = [pytest.param(((10, 5, 0), (3, 4, 5)), id="readme"),       # ahead of time: odd ef' (6-B rows) and odd nf row gathers
        pytest.param(((7, 3, 3), (5, 1, 3)), id="jit-odd"),       # run-time specialised, every width odd
        pytest.param(((6, 4, 2), (4, 2, 2)), id="jit-even")]      # run-time specialised, dword-aligned rows


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("flags", [pytest.param(0, id="default"), pytest.param(FORCE_GENERIC, id="generic"), pytest.param(NO_JIT, id="nojit")])
def test_one_big_graph(gn, dims, R, flags):
    """one graph of 20k edges: the two-launch form (k_block_wave + k_graph_t), replicas"""
    _case(gn, _one_graph(gn), *dims, R=R, flags=flags, seed=R)


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("flags", [pytest.param(0, id="default"), pytest.param(FORCE_GENERIC, id="generic")])
def test_batch_of_small_graphs(gn, dims, flags):
    """40 graphs of 3..39 nodes: README dims take the one-launch pack form (graph update inside k_block_wave)"""
    _case(gn, _small_graphs(gn), *dims, flags=flags, seed=7)


@pytest.mark.parametrize("flags", [pytest.param(0, id="default"), pytest.param(FORCE_GENERIC, id="generic")])
def test_batch_without_edges(gn, flags):
    adjs = [np.zeros((n, n), dtype=np.int64) for n in (3, 5, 2)]
    g = gn.GNGraphBatch(adjs)
    assert g.n_edges == 0
    _case(gn, g, (10, 5, 3), (3, 4, 5), flags=flags, seed=3)


@pytest.mark.parametrize("in_dims", [d for d in itertools.product((0, 3), (0, 2), (0, 4)) if any(d)])
@pytest.mark.parametrize("out_dims", [(3, 4, 5), (2, 0, 3), (0, 2, 2), (2, 3, 0)])
def test_nothing_combinations(gn, in_dims, out_dims):
    """the `nothing` combinations of test_gpu_block.py on a heterogeneous batch with an edgeless and a one-node graph"""
    rng = np.random.default_rng(abs(hash((in_dims, out_dims))) % 2**31)
    adjs = U.random_graphs(rng, (5, 1, 9, 3, 14), 0.4)
    adjs[3][:] = 0
    _case(gn, gn.GNGraphBatch(adjs), in_dims, out_dims, seed=11)


def test_core_widths_fall_back(gn):
    """(128,64,32) => (128,64,32): no fused kernel; widened, the matrix-core forward, rounded"""
    _case(gn, _one_graph(gn, 500, 4000, seed=4), (128, 64, 32), (128, 64, 32), seed=5, act=(1, 1, 0))


def test_c2_full_size(gn):
    """BASELINE configs[1]: 100k nodes, 1M edges, README dims"""
    _case(gn, _one_graph(gn, 100_000, 1_000_000, seed=0), (10, 5, 0), (3, 4, 5), seed=6)


def test_oracle_readme_dims(gn):
    """float64 oracle on the widened inputs: within half a bf16 ulp of the output plus the fp32 tolerance 1e-5 * S"""
    import torch
    g = _one_graph(gn)
    p, (ef, nf, gf), outs = _case(gn, g, (10, 5, 0), (3, 4, 5), seed=8)
    wide = [None if a is None else a.float().cpu().numpy() for a in (ef, nf, gf)]
    ref, scale = O.block_forward_sparse(p, (*g.csc(), g.node_off, g.edge_off), *wide, return_scale=True)
    for o, r, s in zip(outs, ref, scale):
        got = o.float().cpu().numpy().astype(np.float64)
        ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(r), 1e-30))) - 7)  # bf16: 8 significant bits
        assert np.all(np.abs(got - r) <= 0.5 * ulp + U.RTOL * s + 1e-30), float(np.max(np.abs(got - r) - 0.5 * ulp - U.RTOL * s))


def test_graph_capture_replays_same_bits(gn):
    import torch
    lib = gn._lib.load()
    L = gn._lib
    for dims, g in (((10, 5, 0), (3, 4, 5)), _one_graph(gn)), (((7, 3, 3), (5, 1, 3)), _small_graphs(gn)):
        rng = np.random.default_rng(9)
        p = O.make_block_params(rng, *dims)
        blk = U.block_from_params(gn, p)
        keep = []
        cp = blk._c(keep)
        ef, nf, gf = _bf16_inputs(rng, 1, g, dims[0])
        rows = (g.n_edges, g.n_nodes, g.n_graphs)
        outs = [torch.empty((1, T, d), dtype=torch.bfloat16, device="cuda") if d > 0 else None for T, d in zip(rows, dims[1])]
        ws = torch.empty(int(lib.gnx_block_typed_workspace_bytes(g._h, C.byref(cp), 1, L.ELEM_BF16, 0)), dtype=torch.uint8, device="cuda")
        call = lambda: lib.gnx_block_forward_typed(g._h, C.byref(cp), L.ELEM_BF16, _ptr(ef), _ptr(nf), _ptr(gf), 1, *map(_ptr, outs), ws.data_ptr(),
                                                   ws.numel(), 0, torch.cuda.current_stream().cuda_stream)
        assert call() == 0, lib.gnx_last_error()
        torch.cuda.synchronize()
        eager = [None if o is None else o.clone() for o in outs]
        for o in outs:
            if o is not None:
                o.fill_(0)
        graph = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                assert call() == 0, lib.gnx_last_error()
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(2):
            graph.replay()
        torch.cuda.synchronize()
        _assert_bits(outs, eager, f"captured {dims}")


def test_python_api_round_trip(gn):
    """batch(..., dtype=torch.bfloat16) -> GNBlock -> unbatch returns bf16 that matches the ABI result; views work on bf16 batches;
    GNCore refuses bf16 features"""
    import torch
    rng = np.random.default_rng(12)
    adjs = U.random_graphs(rng, (6, 9, 4), 0.5)
    efs = [rng.random((10, int((a == 1).sum())), dtype=np.float32) for a in adjs]
    nfs = [rng.random((5, a.shape[0]), dtype=np.float32) for a in adjs]
    x = gn.batch(dict(graphs=adjs, ef=efs, nf=nfs, gf=None), dtype=torch.bfloat16)
    assert x.ef.dtype == torch.bfloat16 and x.nf.dtype == torch.bfloat16
    x32 = gn.batch(dict(graphs=adjs, ef=efs, nf=nfs, gf=None))
    assert x32.ef.dtype == torch.float32
    assert torch.equal(x.ef, x32.ef.to(torch.bfloat16)) and torch.equal(x.nf, x32.nf.to(torch.bfloat16))
    p = O.make_block_params(rng, (10, 5, 0), (3, 4, 5))
    blk = U.block_from_params(gn, p)
    with torch.no_grad():
        y = blk(x)
    assert all(t.dtype == torch.bfloat16 for t in (y.ef, y.nf, y.gf))
    outs, refs, _ = _forward_pair(gn, blk, x.graphs, 1, 0, *(None if a is None else a.permute(2, 1, 0).contiguous() for a in (x.ef, x.nf, x.gf)))
    _assert_bits([t.permute(2, 1, 0).contiguous() for t in (y.ef, y.nf, y.gf)], refs, "api")
    _assert_bits(outs, refs, "abi")
    u = gn.unbatch(y)
    assert len(u.ef) == 3 and all(t.dtype == torch.bfloat16 for t in u.ef + u.nf + u.gf)
    assert torch.equal(torch.cat([t for t in u.ef], dim=1), y.ef[:, :, 0])
    assert gn.flatunpaddedef(y).dtype == torch.bfloat16 and gn.flatunpaddednf(y).dtype == torch.bfloat16
    # a shared adjacency with replicas, through the views
    adj = adjs[0]
    ef = rng.random((10, int((adj == 1).sum()), 3), dtype=np.float32)
    nf = rng.random((5, adj.shape[0], 3), dtype=np.float32)
    xs = gn.batch(dict(graphs=adj, ef=ef, nf=nf, gf=None), dtype=torch.bfloat16)
    with torch.no_grad():
        ys = blk(xs)
    us = gn.unbatch(ys)
    assert us.ef.dtype == torch.bfloat16 and us.ef.shape == (3, ef.shape[1], 3)
    # mixed dtypes and the fp32-only layers
    with pytest.raises(TypeError):
        blk(gn.NT(x.graphs, x.ef, x32.nf, None))
    core = gn.GNCore((10, 5, 3))
    gf = torch.zeros((3, 3, 1), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(TypeError):
        core(gn.NT(x.graphs, x.ef, x.nf, gf))
    # a differentiable call is not supported in bf16
    blk.edgefn.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        blk(x)


def test_f32_elem_is_gnx_block_forward(gn):
    """elem = GNX_ELEM_F32 is exactly gnx_block_forward"""
    import torch
    lib = gn._lib.load()
    L = gn._lib
    g = _one_graph(gn)
    rng = np.random.default_rng(13)
    p = O.make_block_params(rng, (10, 5, 0), (3, 4, 5))
    blk = U.block_from_params(gn, p)
    keep = []
    cp = blk._c(keep)
    ef, nf, _ = U.packed_inputs(rng, 1, g.n_edges, g.n_nodes, 1, (10, 5, 0))
    ef, nf = torch.from_numpy(ef).cuda(), torch.from_numpy(nf).cuda()
    res = []
    for typed in (False, True):
        outs = [torch.full((1, T, d), float("nan"), device="cuda") for T, d in zip((g.n_edges, g.n_nodes, 1), (3, 4, 5))]
        nb = lib.gnx_block_typed_workspace_bytes(g._h, C.byref(cp), 1, L.ELEM_F32, 0) if typed else lib.gnx_block_workspace_bytes(g._h, C.byref(cp), 1)
        ws = torch.empty(int(nb), dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        if typed:
            rc = lib.gnx_block_forward_typed(g._h, C.byref(cp), L.ELEM_F32, ef.data_ptr(), nf.data_ptr(), None, 1, *(o.data_ptr() for o in outs),
                                             ws.data_ptr(), ws.numel(), 0, s)
        else:
            rc = lib.gnx_block_forward(g._h, C.byref(cp), ef.data_ptr(), nf.data_ptr(), None, 1, *(o.data_ptr() for o in outs), ws.data_ptr(), ws.numel(), 0, s)
        assert rc == 0, lib.gnx_last_error()
        res.append(outs)
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
