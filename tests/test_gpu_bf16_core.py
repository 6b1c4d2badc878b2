"""bfloat16 features through gnx_core_forward_typed on the GPU.  Every case is bit for bit bf16(gnx_core_forward(widened inputs)) under the same
flags: the native path at README ex.3's widths — the one-launch form with and without the edge FeedForward in the block kernel, the
three-launch form — with the launch structure read from the per-kernel profiler, and the path that converts around the fp32 core.  Every
output sits between sentinel bytes; three cases run inside one sentinel arena (tests/arena.py) at exact sizes and at skewed addresses."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import gn_oracle as O
from tests import arena as AR
from tests import test_gpu_memory_contract as MC  # the arena descriptors of a core (_decl_core, _core_params)
from tests import util as U

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0xA5
FORCE_GENERIC, NO_FFE = 0x1, 0x4000
DIMS = (10, 5, 3)


@pytest.fixture(scope="module")
def gn():
    import torch
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


# ---------------------------------------------------------------------------------------------------------------------------------------
# graphs (made once per name)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pairs(N, src, dst):
    return MC._pairs_csc(N, np.asarray(src), np.asarray(dst))


def _csc_parts(name):
    if name == "big":  # >= 65536 edge and node rows, odd counts: partial last workgroups, a lone last bf16 element
        return [U.er_csc(np.random.default_rng(1), 65539, 70001)]
    if name == "hub":  # the same size with one node of in-degree 200 (> 128: a wave tile of several chunks, no FeedForward in the edge lanes)
        rng = np.random.default_rng(2)
        N = 65539
        src = np.concatenate([rng.integers(0, N, 70001), rng.choice(N, 200, replace=False)])
        dst = np.concatenate([rng.integers(0, N, 70001), np.full(200, 31337)])
        return [_pairs(N, src, dst)]
    if name == "three":  # several graphs whose totals just exceed 65536 rows
        rng = np.random.default_rng(3)
        return [U.er_csc(rng, n, e) for n, e in ((22001, 23501), (21999, 23503), (22003, 23497))]
    if name == "medium":
        return [U.er_csc(np.random.default_rng(4), 2000, 20000)]
    if name == "wide":
        return [U.er_csc(np.random.default_rng(5), 300, 5000)]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _graph(name):
    import graphnets_jl_amd as gn
    if name == "small":
        rng = np.random.default_rng(6)
        return gn.GNGraphBatch(U.random_graphs(rng, list(rng.integers(3, 40, 40)), 0.3))
    if name == "no-edges":
        return gn.GNGraphBatch([np.zeros((n, n), dtype=np.int64) for n in (3, 5, 1, 2)])
    parts = _csc_parts(name)
    return gn.GNGraphBatch.from_csc([p[0] for p in parts], [p[1] for p in parts], [len(p[0]) - 1 for p in parts])


def test_graph_shapes(gn):
    """the shapes the cases below rely on"""
    for name in ("big", "hub", "three"):
        g = _graph(name)
        assert g.n_edges >= 65536 and g.n_nodes >= 65536, name
    assert _graph("big").n_graphs == 1 and _graph("three").n_graphs == 3
    colptr = _csc_parts("hub")[0][0]
    assert int(np.diff(colptr).max()) >= 200 > 128
    assert int(np.diff(_csc_parts("big")[0][0]).max()) <= 128
    assert _graph("medium").n_edges < 65536 and _graph("small").n_graphs == 40 and _graph("no-edges").n_edges == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# one case: parameters, bf16 inputs and the fp32 reference, computed once
# ---------------------------------------------------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _guarded(R, T, d):
    """a bf16 (R, T, d) tensor inside a byte buffer with GUARD sentinel bytes on both sides (start 64-B aligned)"""
    import torch
    n = R * T * d * 2
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(torch.bfloat16).view(R, T, d)


def _bf16_inputs(rng, R, g, dims):
    import torch
    xs = U.packed_inputs(rng, R, g.n_edges, g.n_nodes, g.n_graphs, dims)
    # values of both signs over a few binades, rounded once to bf16 (the inputs ARE bf16)
    return [torch.from_numpy((a * 4 - 2).astype(np.float32)).cuda().to(torch.bfloat16).contiguous() for a in xs]


class Case:
    def __init__(self, gn, graph, dims, R, flags, seed):
        import torch
        self.gn, self.g, self.dims, self.R, self.flags = gn, _graph(graph), dims, R, flags
        self.what = f"{graph} {dims} R={R} flags={flags:#x}"
        rng = np.random.default_rng(seed)
        self.p = O.make_core_params(rng, dims)  # LayerNorm gammas in [0.5, 1.5], betas in [-0.1, 0.1]
        self.core = U.core_from_params(gn, self.p)
        self.keep = []
        self.cp = self.core._c(self.keep)
        self.x = _bf16_inputs(rng, R, self.g, dims)
        self.rows = (self.g.n_edges, self.g.n_nodes, self.g.n_graphs)
        lib = self.lib = gn._lib.load()
        g = self.g
        # the reference: gnx_core_forward on the exactly widened inputs, rounded once
        wide = [a.float() for a in self.x]
        o32 = [torch.empty((R, T, d), dtype=torch.float32, device="cuda") for T, d in zip(self.rows, dims)]
        self.nb32 = int(lib.gnx_core_workspace_bytes(g._h, C.byref(self.cp), R))
        ws32 = torch.empty(max(self.nb32, 256), dtype=torch.uint8, device="cuda")
        rc = lib.gnx_core_forward(g._h, C.byref(self.cp), *map(_ptr, wide), R, *map(_ptr, o32), ws32.data_ptr(), ws32.numel(), flags,
                                  torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.gnx_last_error()
        torch.cuda.synchronize()
        self.refs = [o.to(torch.bfloat16) for o in o32]
        self.nb = int(lib.gnx_core_typed_workspace_bytes(g._h, C.byref(self.cp), R, gn._lib.ELEM_BF16, flags))
        assert self.nb > 0, lib.gnx_last_error()

    def typed(self, outs, ws, nbytes=None):
        import torch
        return self.lib.gnx_core_forward_typed(self.g._h, C.byref(self.cp), self.gn._lib.ELEM_BF16, *map(_ptr, self.x), self.R, *map(_ptr, outs), ws.data_ptr(),
                                               ws.numel() if nbytes is None else nbytes, self.flags, torch.cuda.current_stream().cuda_stream)

    def run(self, ws_fill=SENTINEL, profile=False):
        """the typed call into guarded outputs and a workspace of exactly the queried size; returns (outs, kernels seen by the profiler)"""
        import torch
        L = self.gn._lib
        guarded = [_guarded(self.R, T, d) for T, d in zip(self.rows, self.dims)]
        outs = [o for _, o in guarded]
        ws = torch.full((max(self.nb, 16),), ws_fill, dtype=torch.uint8, device="cuda")
        if profile:
            L.profile_reset()
            L.profile_enable(True)
        try:
            rc = self.typed(outs, ws, self.nb)
            torch.cuda.synchronize()
            seen = L.profile_read() if profile else None
        finally:
            if profile:
                L.profile_enable(False)
                L.profile_reset()
        assert rc == 0, f"{self.what}: {self.lib.gnx_last_error()}"
        for buf, o in guarded:
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + o.numel() * 2:] == SENTINEL).all()), f"{self.what}: a store left its output"
        return outs, seen


@functools.lru_cache(maxsize=None)
def _case_cached(graph, dims, R, flags, seed):
    import graphnets_jl_amd as gn
    return Case(gn, graph, dims, R, flags, seed)


def case(gn, graph, dims=DIMS, R=1, flags=0, seed=0):
    return _case_cached(graph, tuple(dims), R, flags, seed)


def _assert_bits(outs, refs, what=""):
    import torch
    for name, o, r in zip(("ef'", "nf'", "gf'"), outs, refs):
        assert o.shape == r.shape, name
        a, b = o.contiguous().view(torch.int16), r.contiguous().view(torch.int16)
        if not torch.equal(a, b):
            bad = (a != b).nonzero()
            raise AssertionError(f"{what} {name}: {bad.shape[0]} of {a.numel()} values differ, first at {tuple(bad[0].tolist())}: "
                                 f"{o[tuple(bad[0])].item()} vs {r[tuple(bad[0])].item()}")


def _check(gn, c, must=(), must_not=(), one_post=False):
    outs, _ = c.run()
    _assert_bits(outs, c.refs, c.what)
    outs2, seen = c.run(profile=True)  # (a second, profiled run: the launch structure)
    _assert_bits(outs2, c.refs, c.what + " (profiled)")
    if U.default_flags(gn) == 0:  # (forms switched on for the whole process change which kernels run, not the bits)
        for k in must:
            assert k in seen, f"{c.what}: {k} did not run: {sorted(seen)}"
        for k in must_not:
            assert k not in seen, f"{c.what}: {k} ran: {sorted(seen)}"
        if one_post:
            assert seen["k_core_post"]["launches"] == 1 and seen["k_block_wave"]["launches"] == 1, seen
    return outs


NO_CONVERSION = ("k_ln1_rows", "k_bf16_widen", "k_bf16_round")
ONE_LAUNCH = dict(must=("k_block_wave", "k_core_post"), must_not=("k_graph_t",) + NO_CONVERSION, one_post=True)
THREE_LAUNCH = dict(must=("k_block_wave", "k_graph_t", "k_core_post"), must_not=NO_CONVERSION)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the native path
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,R", [("big", 1), ("big", 2), ("three", 1)])
def test_one_launch_form_with_ffe(gn, graph, R):
    """k_block_wave with the edge FeedForward in its edge lanes, then k_core_post3 with the graph update inside: one graph, replicas,
    several graphs"""
    c = case(gn, graph, R=R, seed=10 + R)
    _check(gn, c, **ONE_LAUNCH)
    # no edge-sized staging exists in this form
    assert c.nb < c.nb32 + 4 * R * c.g.n_edges * DIMS[0]


def test_one_launch_form_without_ffe(gn):
    """GNX_FLAG_NO_FFE, and a node of in-degree 200: the edge job of k_core_post3 runs the FeedForward from fp32 ef' in the workspace"""
    import torch
    plain = case(gn, "big", seed=11)
    noffe = case(gn, "big", flags=NO_FFE, seed=11)
    a = _check(gn, noffe, **ONE_LAUNCH)
    b, _ = plain.run()
    _assert_bits(a, b, "NO_FFE against the default form")
    assert all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(plain.refs, noffe.refs))
    _check(gn, case(gn, "hub", seed=12), **ONE_LAUNCH)
    _check(gn, case(gn, "three", flags=NO_FFE, seed=13), **ONE_LAUNCH)


@pytest.mark.parametrize("graph,R", [("medium", 1), ("medium", 3), ("small", 1)])
def test_three_launch_form(gn, graph, R):
    """below 65536 rows: the block with its own k_graph_t (bf16 gf in, fp32 gf' out), then k_core_post per entity"""
    _check(gn, case(gn, graph, R=R, seed=20 + R), **THREE_LAUNCH)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the fallback
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_fallback_other_narrow_triple(gn):
    c = case(gn, "medium", dims=(6, 5, 3), seed=30)
    _check(gn, c, must=("k_bf16_widen", "k_bf16_round"))
    n = [c.R * T * d for T, d in zip(c.rows, c.dims)]
    assert c.nb >= c.nb32 + 2 * 4 * sum(n)  # the six fp32 copies


def test_fallback_force_generic(gn):
    _check(gn, case(gn, "medium", flags=FORCE_GENERIC, seed=31), must=("k_bf16_widen", "k_bf16_round"))


def test_fallback_wide_core(gn):
    _check(gn, case(gn, "wide", dims=(128, 64, 32), seed=32), must=("k_bf16_widen", "k_bf16_round"))


def test_fallback_batch_without_edges(gn):
    _check(gn, case(gn, "no-edges", seed=33))


# ---------------------------------------------------------------------------------------------------------------------------------------
# workspace
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,dims,flags", [("big", DIMS, 0), ("big", DIMS, NO_FFE), ("medium", DIMS, 0), ("medium", (6, 5, 3), 0)])
def test_workspace_size_is_exact_and_its_contents_do_not_matter(gn, graph, dims, flags):
    import torch
    c = case(gn, graph, dims=dims, flags=flags, seed=11 if graph == "big" else 40)
    a, _ = c.run(ws_fill=0x00)
    b, _ = c.run(ws_fill=0xFF)
    _assert_bits(a, c.refs, c.what + " ws=0x00")
    _assert_bits(b, c.refs, c.what + " ws=0xFF")
    # one byte less than the query: refused, nothing written
    guarded = [_guarded(c.R, T, d) for T, d in zip(c.rows, c.dims)]
    ws = torch.full((c.nb,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert c.typed([o for _, o in guarded], ws, c.nb - 1) == gn._lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert all(bool((buf == SENTINEL).all()) for buf, _ in guarded) and bool((ws == SENTINEL).all())


def test_f32_elem_is_gnx_core_forward(gn):
    import torch
    c = case(gn, "medium", seed=41)
    L = gn._lib
    assert c.lib.gnx_core_typed_workspace_bytes(c.g._h, C.byref(c.cp), 1, L.ELEM_F32, 0) == c.nb32
    wide = [a.float() for a in c.x]
    res = []
    for typed in (False, True):
        outs = [torch.full((1, T, d), float("nan"), device="cuda") for T, d in zip(c.rows, c.dims)]
        ws = torch.empty(c.nb32, dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        if typed:
            rc = c.lib.gnx_core_forward_typed(c.g._h, C.byref(c.cp), L.ELEM_F32, *map(_ptr, wide), 1, *map(_ptr, outs), ws.data_ptr(), ws.numel(), 0, s)
        else:
            rc = c.lib.gnx_core_forward(c.g._h, C.byref(c.cp), *map(_ptr, wide), 1, *map(_ptr, outs), ws.data_ptr(), ws.numel(), 0, s)
        assert rc == 0, c.lib.gnx_last_error()
        res.append(outs)
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# memory contract and alignment: every buffer of the call inside one sentinel arena
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,dims", [pytest.param("big", DIMS, id="native-one-launch"), pytest.param("medium", DIMS, id="native-three-launch"),
                                        pytest.param("medium", (6, 5, 3), id="fallback")])
def test_arena_memory_contract_and_skewed_addresses(gn, graph, dims):
    import torch
    L = gn._lib
    lib = L.load()
    ref = case(gn, graph, dims=dims, seed=11 if graph == "big" else (40 if dims != DIMS else 21))
    g, p, R = ref.g, ref.p, 1
    a = AR.Arena("cuda")
    MC._decl_core(a, p)
    ins = [a.input(n, t) for n, t in zip(("ef", "nf", "gf"), ref.x)]
    outs = [a.output(n, (R, T, d), torch.bfloat16) for n, T, d in zip(("ef_out", "nf_out", "gf_out"), ref.rows, dims)]
    w = a.workspace("ws", lambda: lib.gnx_core_typed_workspace_bytes(g._h, C.byref(MC._core_params(gn, a, p)), R, L.ELEM_BF16, 0))
    a.build(ws_fill=0x00)

    def run():
        cp = MC._core_params(gn, a, p)
        rc = lib.gnx_core_forward_typed(g._h, C.byref(cp), L.ELEM_BF16, *map(a.ptr, ins), R, *map(a.ptr, outs), a.ptr(w), a.nbytes(w), 0,
                                        torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    assert run() == 0, lib.gnx_last_error()
    a.check(ref.what)  # nothing outside outputs and workspace written; inputs, weights, gammas and betas untouched; every output element written
    assert a.nbytes(w) == ref.nb
    _assert_bits([a.view(n) for n in outs], ref.refs, ref.what + " (arena)")
    base = a.output_bits()
    for k in (4, 8, 12):  # every buffer k bytes behind a 256-B boundary, the workspace on it
        a.relayout(lambda c: 0 if c.kind == AR.WORKSPACE else k, ws_fill=0xFF)
        assert run() == 0, (k, lib.gnx_last_error())
        a.check(f"{ref.what} skew +{k}")
        got = a.output_bits()
        assert all(torch.equal(got[n], base[n]) for n in base), f"{ref.what}: other bits at +{k}"
    # a bf16 buffer at +2 and a workspace at +8 are refused before any GPU work
    for name in ("nf", "ef_out"):
        a.relayout(lambda c: 2 if c.name == name else 0)
        assert run() == L.ERR_INVALID_ARG and b"4-byte aligned" in lib.gnx_last_error(), name
        a.check(f"{ref.what}: {name} at +2", unwritten=False)
        assert all(bool((a.raw(n) == AR.UNWRITTEN).all()) for n in outs)
    a.relayout(lambda c: 8 if c.kind == AR.WORKSPACE else 0)
    assert run() == L.ERR_WORKSPACE and b"16-byte aligned" in lib.gnx_last_error()
    a.check(f"{ref.what}: workspace at +8", unwritten=False)
    assert all(bool((a.raw(n) == AR.UNWRITTEN).all()) for n in outs)


# ---------------------------------------------------------------------------------------------------------------------------------------
# capture, Python
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_same_bits(gn):
    import torch
    c = case(gn, "big", seed=11)  # (the query ran when the case was made: outside the capture)
    outs = [torch.zeros((c.R, T, d), dtype=torch.bfloat16, device="cuda") for T, d in zip(c.rows, c.dims)]
    ws = torch.empty(c.nb, dtype=torch.uint8, device="cuda")
    assert c.typed(outs, ws) == 0, c.lib.gnx_last_error()
    torch.cuda.synchronize()
    _assert_bits(outs, c.refs, "eager")
    for o in outs:
        o.fill_(0)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            assert c.typed(outs, ws) == 0, c.lib.gnx_last_error()
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    _assert_bits(outs, c.refs, "captured")


def test_python_model_in_bf16(gn):
    """batch(..., dtype=torch.bfloat16) -> GNBlock -> two GNCore(bf16=True) -> GNBlock under no_grad: bf16 at every stage, the bits of the same
    chain driven through the ABI"""
    import torch
    L = gn._lib
    lib = L.load()
    rng = np.random.default_rng(50)
    adjs = U.random_graphs(rng, (6, 9, 4, 31), 0.5)
    efs = [rng.random((10, int((a == 1).sum())), dtype=np.float32) * 4 - 2 for a in adjs]
    nfs = [rng.random((5, a.shape[0]), dtype=np.float32) * 4 - 2 for a in adjs]
    gfs = [rng.random((3,), dtype=np.float32) * 4 - 2 for a in adjs]
    x = gn.batch(dict(graphs=adjs, ef=efs, nf=nfs, gf=gfs), dtype=torch.bfloat16)
    assert all(t.dtype == torch.bfloat16 for t in (x.ef, x.nf, x.gf))
    blocks = [U.block_from_params(gn, O.make_block_params(rng, DIMS, DIMS, act=(1, 0, 2))) for _ in range(2)]
    cores = [U.core_from_params(gn, O.make_core_params(rng, DIMS)) for _ in range(2)]
    default = gn.GNCore(DIMS)
    assert default.bf16 is False
    with pytest.raises(TypeError, match="bfloat16"):
        default(x)
    for c in cores:
        assert c.bf16 is False
        c.bf16 = True
    assert gn.GNCore(DIMS, bf16=True).bf16 is True
    layers = [blocks[0], cores[0], cores[1], blocks[1]]
    g = x.graphs
    stream = torch.cuda.current_stream().cuda_stream
    pk = lambda t: t.permute(2, 1, 0).contiguous()
    y, z = x, [pk(t) for t in (x.ef, x.nf, x.gf)]
    with torch.no_grad():
        for layer in layers:
            y = layer(y)
            assert all(t.dtype == torch.bfloat16 for t in (y.ef, y.nf, y.gf)), type(layer).__name__
            keep = []
            p = layer._c(keep)
            outs = [torch.empty_like(t) for t in z]
            if isinstance(layer, gn.GNCore):
                ws = torch.empty(max(int(lib.gnx_core_typed_workspace_bytes(g._h, C.byref(p), 1, L.ELEM_BF16, 0)), 256), dtype=torch.uint8, device="cuda")
                rc = lib.gnx_core_forward_typed(g._h, C.byref(p), L.ELEM_BF16, *map(_ptr, z), 1, *map(_ptr, outs), ws.data_ptr(), ws.numel(), 0, stream)
            else:
                ws = torch.empty(max(int(lib.gnx_block_typed_workspace_bytes(g._h, C.byref(p), 1, L.ELEM_BF16, 0)), 256), dtype=torch.uint8, device="cuda")
                rc = lib.gnx_block_forward_typed(g._h, C.byref(p), L.ELEM_BF16, *map(_ptr, z), 1, *map(_ptr, outs), ws.data_ptr(), ws.numel(), 0, stream)
            assert rc == 0, lib.gnx_last_error()
            torch.cuda.synchronize()
            z = outs
            _assert_bits([pk(t) for t in (y.ef, y.nf, y.gf)], z, type(layer).__name__)
    # float32 features do not notice the switch; the list form carries each core's own
    x32 = gn.NT(g, x.ef.float(), x.nf.float(), x.gf.float())
    with torch.no_grad():
        on = cores[0](x32)
        cores[0].bf16 = False
        off = cores[0](x32)
        cores[0].bf16 = True
        assert on.ef.dtype == torch.float32 and all(torch.equal(u, v) for u, v in zip((on.ef, on.nf, on.gf), (off.ef, off.nf, off.gf)))
        yl = gn.GNCoreList(cores)(blocks[0](x))
    assert yl.ef.dtype == torch.bfloat16
    # an odd-offset view is copied to a 4-byte aligned buffer
    flat = torch.zeros(x.nf.numel() + 1, dtype=torch.bfloat16, device="cuda")
    flat[1:] = pk(x.nf).reshape(-1)
    nf_odd = flat[1:].view(pk(x.nf).shape).permute(2, 1, 0)
    assert nf_odd.permute(2, 1, 0).data_ptr() % 4 == 2
    with torch.no_grad():
        y1, y2 = cores[0](gn.NT(g, x.ef, nf_odd, x.gf)), cores[0](x)
    _assert_bits([y1.ef, y1.nf, y1.gf], [y2.ef, y2.nf, y2.gf], "odd-offset view")
