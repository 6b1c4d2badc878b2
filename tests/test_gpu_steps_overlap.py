"""gnx_block_forward_steps on two streams: even steps on the caller's stream, odd steps on a side stream of the handle, the chained graph
update of step i at the front of step i + 2's launch, two flushes and a join before the call returns.  Every case compares the call's default
schedule (and GNX_FLAG_NO_FORK, one stream) against K separate gnx_block_forward calls in order: outputs bit-identical, eagerly and from a
captured graph replayed three times; steps whose buffers overlap are ordered, an argument error leaves the caller's stream joined."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import gn_oracle as O
from tests import util as U

pytestmark = pytest.mark.gpu

NO_FORK = 0x1000  # GNX_FLAG_NO_FORK (include/gnx.h)


@pytest.fixture(scope="module")
def gn():
    import graphnets_jl_amd as gn
    return gn


def _batch(gn, rng, case):
    if case in ("c2", "r2"):
        n, e = (250_000, 1_000_000) if case == "c2" else (30_000, 200_000)
        cp, rv = U.er_csc(rng, n, e)
        return gn.GNGraphBatch.from_csc([cp], [rv], [n])
    if case == "small":
        cp, rv = U.er_csc(rng, 3_000, 20_000)
        return gn.GNGraphBatch.from_csc([cp], [rv], [3_000])
    if case == "multigraph":  # graphs of > 8 wave tiles: the chained two-launch form, one wavefront per graph in the graph update
        sizes = rng.integers(1_500, 3_000, 12)
    else:  # "pack": 4096 small graphs, the graph update inside the block kernel
        sizes = rng.integers(10, 40, 4096)
    cs = [U.er_csc(rng, int(n), 4 * int(n)) for n in sizes]
    return gn.GNGraphBatch.from_csc([c[0] for c in cs], [c[1] for c in cs], [int(n) for n in sizes])


def _sets(plan, g, dims, R, n, seed):
    gen = torch.Generator(device=g.device).manual_seed(seed)
    mk = lambda T, d: torch.rand((R, T, d), device=g.device, generator=gen) if d > 0 else None
    de, dn, dg = dims
    return [dict(ef=mk(g.n_edges, de), nf=mk(g.n_nodes, dn), gf=mk(g.n_graphs, dg), out=plan.outputs(), ws=plan.new_workspace()) for _ in range(n)]


def _serial(plan, seq):
    """K separate gnx_block_forward calls in order; returns what each step's outputs held right after it ran"""
    got = []
    for b in seq:
        plan(b["ef"], b["nf"], b["gf"], *b["out"], ws=b["ws"])
        got.append([None if t is None else t.clone() for t in b["out"]])
    torch.cuda.synchronize()
    return got


def _poison(seq):
    for b in seq:
        for t in b["out"]:
            if t is not None:
                t.fill_(float("nan"))


def _final(seq):
    """the outputs each buffer set holds after the loop (the last step that wrote it)"""
    last = {}
    for i, b in enumerate(seq):
        last[id(b["out"][0]) if b["out"][0] is not None else id(b["out"][1])] = i
    return sorted(last.values())


def _assert_equal(seq, ref, what):
    for i in _final(seq):
        for name, a, r in zip(("ef", "nf", "gf"), seq[i]["out"], ref[i]):
            if a is not None:
                assert torch.equal(a, r), f"{what}: step {i} {name} differs from the serial forwards"


def _run_all_forms(gn, plan, plan1, seq, ref, what):
    for p, form in ((plan, "two streams"), (plan1, "GNX_FLAG_NO_FORK")):
        _poison(seq)
        p.steps(seq)
        torch.cuda.synchronize()
        _assert_equal(seq, ref, f"{what}, {form}, eager")
    _poison(seq)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, capture_error_mode="thread_local"):
        plan.steps(seq)
    for rep in range(3):
        _poison(seq)
        cg.replay()
        torch.cuda.synchronize()
        _assert_equal(seq, ref, f"{what}, captured, replay {rep}")
    del cg


def _setup(gn, case, dims=((10, 5, 3), (3, 4, 5)), seed=0):
    rng = np.random.default_rng(4200 + seed + len(case))
    g = _batch(gn, rng, case)
    R = 2 if case == "r2" else 1
    blk = U.block_from_params(gn, O.make_block_params(rng, *dims))
    plan = gn.BlockPlan(blk, g, R=R)
    plan1 = gn.BlockPlan(blk, g, R=R, flags=plan.flags | NO_FORK)
    return g, R, plan, plan1


@pytest.mark.parametrize("K", [1, 2, 3, 20])
@pytest.mark.parametrize("case", ["c2", "small", "multigraph", "pack", "r2"])
def test_steps_two_streams_match_serial_forwards(gn, case, K):
    dims = ((10, 5, 3), (3, 4, 5))
    g, R, plan, plan1 = _setup(gn, case, dims)
    sets = _sets(plan, g, dims[0], R, min(K, 4), seed=K)
    seq = [sets[i % len(sets)] for i in range(K)]
    ref = _serial(plan, seq)
    _run_all_forms(gn, plan, plan1, seq, ref, f"{case}, K={K}")


@pytest.mark.parametrize("nsets", [1, 2, 3, 4, 5, 7])
def test_steps_rotating_buffer_sets(gn, nsets):
    """one set: every pair of steps aliases and the call must order them; two: every step shares with the step two before it (the
    pending update of its own stream); three: with the one three before it (the other stream); five and seven: with a step on the other
    stream further back, which only the wait of every step for the step three before it keeps apart"""
    dims = ((10, 5, 3), (3, 4, 5))
    g, R, plan, plan1 = _setup(gn, "small", dims, seed=nsets)
    sets = _sets(plan, g, dims[0], R, nsets, seed=10 + nsets)
    seq = [sets[i % nsets] for i in range(17)]
    ref = _serial(plan, seq)
    _run_all_forms(gn, plan, plan1, seq, ref, f"{nsets} sets")


def test_steps_shared_workspace(gn):
    dims = ((10, 5, 3), (3, 4, 5))
    g, R, plan, plan1 = _setup(gn, "c2", dims, seed=7)
    sets = _sets(plan, g, dims[0], R, 6, seed=77)
    seq = [dict(b, ws=sets[0]["ws"]) for b in sets]
    ref = _serial(plan, seq)
    _run_all_forms(gn, plan, plan1, seq, ref, "one workspace")


@pytest.mark.parametrize("case", ["small", "multigraph"])
def test_steps_dims_to_dims_chain_reads_previous_outputs(gn, case):
    """step i + 1 reads step i's ef_out / nf_out / gf_out: the steps cannot overlap, the call must serialise them"""
    dims = ((10, 5, 3), (10, 5, 3))
    g, R, plan, plan1 = _setup(gn, case, dims, seed=11)
    K = 6
    bufs = _sets(plan, g, dims[0], R, 1, seed=5)[0]
    seq = []
    src = (bufs["ef"], bufs["nf"], bufs["gf"])
    for i in range(K):
        out = plan.outputs()
        seq.append(dict(ef=src[0], nf=src[1], gf=src[2], out=out, ws=plan.new_workspace()))
        src = out
    ref = _serial(plan, seq)
    for p, form in ((plan, "two streams"), (plan1, "GNX_FLAG_NO_FORK")):
        _poison(seq)
        p.steps(seq)
        torch.cuda.synchronize()
        for i in range(K):
            for name, a, r in zip(("ef", "nf", "gf"), seq[i]["out"], ref[i]):
                assert torch.equal(a, r), f"{case} {form}: step {i} {name}"
    _poison(seq)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, capture_error_mode="thread_local"):
        plan.steps(seq)
    for rep in range(3):
        _poison(seq)
        cg.replay()
        torch.cuda.synchronize()
        for i in range(K):
            for name, a, r in zip(("ef", "nf", "gf"), seq[i]["out"], ref[i]):
                assert torch.equal(a, r), f"{case} captured replay {rep}: step {i} {name}"


@pytest.mark.parametrize("bad", [1, 3, 4])
def test_steps_argument_error_leaves_stream_joined(gn, bad):
    """an invalid step (workspace too small): the error comes back, every step before it is complete once the caller's stream is, and
    the next call on that stream gives the right results"""
    dims = ((10, 5, 3), (3, 4, 5))
    g, R, plan, plan1 = _setup(gn, "small", dims, seed=20 + bad)
    sets = _sets(plan, g, dims[0], R, 6, seed=bad)
    ref = _serial(plan, sets)
    _poison(sets)
    lib = gn._lib.load()
    s = torch.cuda.current_stream(g.device).cuda_stream
    arr = (gn._lib.BlockStep * len(sets))()
    P = lambda t: None if t is None else t.data_ptr()
    for i, b in enumerate(sets):
        arr[i] = gn._lib.BlockStep(P(b["ef"]), P(b["nf"]), P(b["gf"]), P(b["out"][0]), P(b["out"][1]), P(b["out"][2]), b["ws"].data_ptr(),
                                   b["ws"].numel() if i != bad else 16)
    assert lib.gnx_block_forward_steps(g._h, C.byref(plan.p), arr, len(sets), R, plan.flags, s) == gn._lib.ERR_WORKSPACE
    # only the caller's stream is waited for: the side stream's steps must have been joined into it
    torch.cuda.current_stream(g.device).synchronize()
    for i in range(bad):
        for name, a, r in zip(("ef", "nf", "gf"), sets[i]["out"], ref[i]):
            assert torch.equal(a, r), f"step {i} {name} before the invalid step {bad}"
    _poison(sets)
    plan.steps(sets)
    torch.cuda.current_stream(g.device).synchronize()
    for i in range(len(sets)):
        for name, a, r in zip(("ef", "nf", "gf"), sets[i]["out"], ref[i]):
            assert torch.equal(a, r), f"step {i} {name} of the call after the error"


def _hip():
    """the HIP runtime torch has loaded"""
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln)
    hip = C.CDLL(path)
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphGetRootNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    return hip


@pytest.mark.parametrize("case", ["c2", "pack"])
def test_steps_schedule_engages_two_streams(gn, case):
    """The default schedule really forks: captured on its own, the call's graph has TWO root launches (step 0 on the caller's stream, step 1
    on the side stream, neither behind the other); with GNX_FLAG_NO_FORK it is one chain with one root.  (The other tests cannot tell the
    two schedules apart: their outputs are the same bits.)"""
    dims = ((10, 5, 3), (3, 4, 5))
    g, R, plan, plan1 = _setup(gn, case, dims, seed=30)
    sets = _sets(plan, g, dims[0], R, 4, seed=31)
    seq = [sets[i % 4] for i in range(8)]
    hip = _hip()
    torch.cuda.synchronize()
    roots = {}
    for p, form in ((plan, "default"), (plan1, "no_fork")):
        st = torch.cuda.Stream(g.device)
        assert hip.hipStreamBeginCapture(st.cuda_stream, 1) == 0  # hipStreamCaptureModeThreadLocal
        p.steps(seq, stream=st.cuda_stream)
        graph = C.c_void_p()
        assert hip.hipStreamEndCapture(st.cuda_stream, C.byref(graph)) == 0
        n_roots, n_nodes = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipGraphGetRootNodes(graph, None, C.byref(n_roots)) == 0
        assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0
        assert hip.hipGraphDestroy(graph) == 0
        roots[form] = (n_roots.value, n_nodes.value)
    assert roots["default"][0] == 2 and roots["no_fork"][0] == 1, roots
