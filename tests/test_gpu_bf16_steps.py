"""gnx_block_forward_steps_typed on bfloat16 features (BlockPlan(..., dtype=torch.bfloat16).steps): every output of every step is bit for bit
what K separate gnx_block_forward_typed calls in order give, in every schedule — two streams, one stream (GNX_FLAG_NO_FORK), chained, the
fallback that converts around the fp32 forward — eagerly and from a captured graph replayed three times."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import gn_oracle as O
from tests import util as U

pytestmark = pytest.mark.gpu

FORCE_GENERIC, NO_FORK, NO_JIT = 0x1, 0x1000, 0x8000
BF = torch.bfloat16


@pytest.fixture(scope="module")
def gn():
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


def _batch(gn, rng, case):
    if case == "c2":  # BASELINE configs[1]: one graph, 100k nodes, 1M edges
        cp, rv = U.er_csc(rng, 100_000, 1_000_000)
        return gn.GNGraphBatch.from_csc([cp], [rv], [100_000])
    if case == "one":
        cp, rv = U.er_csc(rng, 3_000, 20_000)
        return gn.GNGraphBatch.from_csc([cp], [rv], [3_000])
    if case == "multigraph":  # graphs of > 8 wave tiles: the chained two-launch form, one wavefront per graph in the graph update
        sizes = rng.integers(1_500, 3_000, 12)
    else:  # "pack": 4096 small graphs, the graph update inside the block kernel
        sizes = rng.integers(10, 40, 4096)
    cs = [U.er_csc(rng, int(n), 4 * int(n)) for n in sizes]
    return gn.GNGraphBatch.from_csc([c[0] for c in cs], [c[1] for c in cs], [int(n) for n in sizes])


def _setup(gn, case, dims, flags=0, seed=0, act=(1, 0, 2)):
    rng = np.random.default_rng(5100 + seed + len(case))
    g = _batch(gn, rng, case)
    blk = U.block_from_params(gn, O.make_block_params(rng, *dims, act=act))
    plan = gn.BlockPlan(blk, g, flags=blk.flags | flags, dtype=BF)
    return g, blk, plan


def _sets(plan, g, dims, n, seed):
    gen = torch.Generator(device=g.device).manual_seed(seed)
    # values of both signs over a few binades, rounded once to bf16 (the inputs ARE bf16)
    mk = lambda T, d: (torch.rand((1, T, d), device=g.device, generator=gen) * 4 - 2).to(BF) if d > 0 else None
    de, dn, dg = dims
    return [dict(ef=mk(g.n_edges, de), nf=mk(g.n_nodes, dn), gf=mk(g.n_graphs, dg), out=plan.outputs(), ws=plan.new_workspace()) for _ in range(n)]


def _serial(plan, seq):
    """K separate gnx_block_forward_typed calls in order; what each step's outputs held right after it ran"""
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
                t.view(torch.int16).fill_(0x7FC1)  # a NaN no forward writes


def _final(seq):
    """the steps whose outputs are still in their buffers after the loop (the last step that wrote each set)"""
    last = {}
    for i, b in enumerate(seq):
        last[next(id(t) for t in b["out"] if t is not None)] = i
    return sorted(last.values())


def _assert_bits(seq, ref, what, steps=None):
    for i in (_final(seq) if steps is None else steps):
        for name, a, r in zip(("ef", "nf", "gf"), seq[i]["out"], ref[i]):
            if a is None:
                continue
            x, y = a.view(torch.int16), r.view(torch.int16)
            if not torch.equal(x, y):
                n = int((x != y).sum())
                raise AssertionError(f"{what}: step {i} {name}: {n} of {x.numel()} values differ from the serial typed forwards")


def _eager_and_captured(plan, seq, ref, what, steps=None):
    _poison(seq)
    plan.steps(seq)
    torch.cuda.synchronize()
    _assert_bits(seq, ref, f"{what}, eager", steps)
    _poison(seq)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, capture_error_mode="thread_local"):
        plan.steps(seq)
    for rep in range(3):
        _poison(seq)
        cg.replay()
        torch.cuda.synchronize()
        _assert_bits(seq, ref, f"{what}, captured, replay {rep}", steps)
    del cg


README = ((10, 5, 0), (3, 4, 5))
EX1OUT = ((3, 4, 5), (3, 4, 5))
CASES = [
    pytest.param("c2", README, 0, id="c2"),
    pytest.param("multigraph", EX1OUT, 0, id="multigraph"),
    pytest.param("pack", README, 0, id="pack"),
    pytest.param("one", ((7, 3, 3), (5, 1, 3)), 0, id="jit-dg"),
    pytest.param("one", ((128, 64, 32), (128, 64, 32)), 0, id="fallback-wide"),
    pytest.param("one", EX1OUT, FORCE_GENERIC, id="force-generic"),
    pytest.param("one", ((7, 3, 3), (5, 1, 3)), NO_JIT, id="no-jit"),
    pytest.param("one", EX1OUT, NO_FORK, id="no-fork"),
]


@pytest.mark.parametrize("case,dims,flags", CASES)
def test_bf16_steps_match_serial_typed_forwards(gn, case, dims, flags):
    act = (1, 1, 0) if dims[0][0] == 128 else (1, 0, 2)
    g, _, plan = _setup(gn, case, dims, flags, act=act)
    sets = _sets(plan, g, dims[0], 4, seed=3)
    seq = [sets[i % 4] for i in range(7)]
    ref = _serial(plan, seq)
    _eager_and_captured(plan, seq, ref, f"{case} {dims} flags={flags:#x}")


def test_bf16_steps_match_rounded_fp32_steps(gn):
    """spot check: bf16(gnx_block_forward_steps(widened inputs)) — the fp32 loop on the same values, rounded once"""
    g, blk, plan = _setup(gn, "multigraph", EX1OUT, seed=1)
    plan32 = gn.BlockPlan(blk, g)
    sets = _sets(plan, g, EX1OUT[0], 3, seed=4)
    seq = [sets[i % 3] for i in range(5)]
    wide = [dict(ef=b["ef"].float(), nf=b["nf"].float(), gf=b["gf"].float(), out=plan32.outputs(), ws=plan32.new_workspace()) for b in sets]
    seq32 = [wide[i % 3] for i in range(5)]
    _poison(seq)
    plan.steps(seq)
    plan32.steps(seq32)
    torch.cuda.synchronize()
    ref = [[t.to(BF) for t in b["out"]] for b in seq32]
    _assert_bits(seq, ref, "bf16 steps vs bf16(fp32 steps)")


def _recurrent(plan, x0, K):
    """step i + 1 reads step i's outputs"""
    seq, src = [], x0
    for _ in range(K):
        out = plan.outputs()
        seq.append(dict(ef=src[0], nf=src[1], gf=src[2], out=out, ws=plan.new_workspace()))
        src = out
    return seq


@pytest.mark.parametrize("case,dims", [pytest.param("one", EX1OUT, id="chained-one"), pytest.param("multigraph", EX1OUT, id="chained-multigraph"),
                                       pytest.param("one", ((4, 4, 4), (4, 4, 4)), id="jit")])
def test_bf16_recurrent_loop(gn, case, dims):
    """x_{i+1} = block(x_i): the steps cannot overlap, the call must order them; every step's outputs are kept"""
    g, blk, plan = _setup(gn, case, dims, seed=2)
    plan1 = gn.BlockPlan(blk, g, flags=plan.flags | NO_FORK, dtype=BF)
    b0 = _sets(plan, g, dims[0], 1, seed=5)[0]
    K = 6
    seq = _recurrent(plan, (b0["ef"], b0["nf"], b0["gf"]), K)
    ref = _serial(plan, seq)
    _eager_and_captured(plan, seq, ref, f"recurrent {case} {dims}", steps=range(K))
    _poison(seq)
    plan1.steps(seq)
    torch.cuda.synchronize()
    _assert_bits(seq, ref, f"recurrent {case} {dims}, one stream", steps=range(K))


def test_bf16_shared_workspace_and_overwritten_input(gn):
    """steps i and i + 2 share a workspace (the pending update of the same stream); step i + 1 writes over step i's input"""
    g, blk, plan = _setup(gn, "one", EX1OUT, seed=3)
    sets = _sets(plan, g, EX1OUT[0], 6, seed=6)
    seq = [dict(b, ws=sets[i % 2]["ws"]) for i, b in enumerate(sets)]
    # step 2 writes its outputs over step 1's inputs (same widths: dims => dims)
    seq[2] = dict(seq[2], out=(seq[1]["ef"], seq[1]["nf"], seq[1]["gf"]))
    # ... and step 4 over step 3's, which is also step 5's input
    seq[4] = dict(seq[4], out=(seq[3]["ef"], seq[3]["nf"], seq[3]["gf"]))
    seq[5] = dict(seq[5], ef=seq[3]["ef"], nf=seq[3]["nf"], gf=seq[3]["gf"])
    keep = [(b["ef"].clone(), b["nf"].clone(), b["gf"].clone()) for b in seq]  # the inputs before any step ran
    ref = _serial(plan, seq)
    plan1 = gn.BlockPlan(blk, g, flags=plan.flags | NO_FORK, dtype=BF)
    for p, form in ((plan, "two streams"), (plan1, "one stream")):
        for b, k in zip(seq, keep):
            for t, v in zip((b["ef"], b["nf"], b["gf"]), k):
                t.copy_(v)
        _poison([b for i, b in enumerate(seq) if i not in (2, 4)])
        p.steps(seq)
        torch.cuda.synchronize()
        _assert_bits(seq, ref, f"shared workspace / overwritten input, {form}", steps=range(len(seq)))


def test_bf16_steps_chain_the_graph_update(gn):
    """profiler on (one stream): K bf16 steps at ahead-of-time widths issue K k_block_wave launches and ONE k_graph_t (the last step's flush)"""
    g, _, plan = _setup(gn, "one", EX1OUT, seed=4)
    sets = _sets(plan, g, EX1OUT[0], 2, seed=7)
    K = 8
    seq = [sets[i % 2] for i in range(K)]
    torch.cuda.synchronize()
    gn.profile_reset()
    gn.profile_enable(True)
    try:
        plan.steps(seq)
        torch.cuda.synchronize()
    finally:
        gn.profile_enable(False)
    prof = gn.profile_read()
    gn.profile_reset()
    assert prof["k_block_wave"]["launches"] == K and prof["k_graph_t"]["launches"] == 1, prof


def _hip():
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln)
    hip = C.CDLL(path)
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphGetRootNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    return hip


@pytest.mark.parametrize("case,dims", [pytest.param("c2", README, id="c2"), pytest.param("one", ((7, 3, 3), (5, 1, 3)), id="jit")])
def test_bf16_steps_engage_two_streams(gn, case, dims):
    """captured on its own, the default bf16 schedule's graph has two root launches; GNX_FLAG_NO_FORK one"""
    g, blk, plan = _setup(gn, case, dims, seed=5)
    plan1 = gn.BlockPlan(blk, g, flags=plan.flags | NO_FORK, dtype=BF)
    sets = _sets(plan, g, dims[0], 4, seed=8)
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
        n = C.c_size_t(0)
        assert hip.hipGraphGetRootNodes(graph, None, C.byref(n)) == 0
        assert hip.hipGraphDestroy(graph) == 0
        roots[form] = n.value
    assert roots == {"default": 2, "no_fork": 1}, roots


def _step_array(gn, seq, ws_bytes=None):
    P = lambda t: None if t is None else t.data_ptr()
    arr = (gn._lib.BlockStep * len(seq))()
    for i, b in enumerate(seq):
        arr[i] = gn._lib.BlockStep(P(b["ef"]), P(b["nf"]), P(b["gf"]), *(P(t) for t in b["out"]), b["ws"].data_ptr(),
                                   b["ws"].numel() if ws_bytes is None or i not in ws_bytes else ws_bytes[i])
    return arr


def test_bf16_misaligned_last_step_is_refused_before_any_launch(gn):
    g, _, plan = _setup(gn, "one", EX1OUT, seed=6)
    sets = _sets(plan, g, EX1OUT[0], 5, seed=9)
    _poison(sets)
    # the last step's nf_out 2 bytes into its buffer: not 4-byte aligned
    last = sets[-1]
    nf_buf = torch.empty(last["out"][1].numel() + 2, dtype=BF, device=g.device)
    nf_buf.view(torch.int16).fill_(0x7FC1)
    n = last["out"][1].numel()
    last["out"] = (last["out"][0], nf_buf[1:1 + n].view(last["out"][1].shape), last["out"][2])
    assert last["out"][1].data_ptr() % 4 == 2
    lib = gn._lib.load()
    rc = lib.gnx_block_forward_steps_typed(g._h, C.byref(plan.p), gn._lib.ELEM_BF16, _step_array(gn, sets), len(sets), 1, plan.flags,
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == gn._lib.ERR_INVALID_ARG and b"aligned" in lib.gnx_last_error()
    torch.cuda.synchronize()
    for i, b in enumerate(sets):
        for t in b["out"]:
            assert bool((t.view(torch.int16) == 0x7FC1).all()), f"step {i} wrote an output before the check of the last step"


@pytest.mark.parametrize("bad", [1, 4])
def test_bf16_error_inside_the_loop_leaves_stream_joined(gn, bad):
    """a workspace too small at step `bad` (found inside the loop): the error comes back, every step before it is complete once the CALLER's
    stream is, and the next call on that stream gives the right results"""
    g, _, plan = _setup(gn, "one", EX1OUT, seed=7 + bad)
    sets = _sets(plan, g, EX1OUT[0], 6, seed=bad)
    ref = _serial(plan, sets)
    _poison(sets)
    lib = gn._lib.load()
    s = torch.cuda.current_stream(g.device)
    rc = lib.gnx_block_forward_steps_typed(g._h, C.byref(plan.p), gn._lib.ELEM_BF16, _step_array(gn, sets, {bad: 16}), len(sets), 1, plan.flags,
                                           s.cuda_stream)
    assert rc == gn._lib.ERR_WORKSPACE
    s.synchronize()
    _assert_bits(sets, ref, f"steps before the invalid step {bad}", steps=range(bad))
    _poison(sets)
    plan.steps(sets)
    s.synchronize()
    _assert_bits(sets, ref, "the call after the error", steps=range(len(sets)))


def test_typed_workspace_query_creates_side_streams(gn):
    """a bf16 caller that sizes its workspaces only through the typed query still gets the two-stream schedule (a fresh handle)"""
    rng = np.random.default_rng(77)
    cp, rv = U.er_csc(rng, 3_000, 20_000)
    g = gn.GNGraphBatch.from_csc([cp], [rv], [3_000])
    blk = U.block_from_params(gn, O.make_block_params(rng, *EX1OUT))
    plan = gn.BlockPlan(blk, g, dtype=BF)  # (only gnx_block_typed_workspace_bytes was called on this handle)
    sets = _sets(plan, g, EX1OUT[0], 2, seed=10)
    hip = _hip()
    torch.cuda.synchronize()
    st = torch.cuda.Stream(g.device)
    assert hip.hipStreamBeginCapture(st.cuda_stream, 1) == 0
    plan.steps(sets, stream=st.cuda_stream)
    graph = C.c_void_p()
    assert hip.hipStreamEndCapture(st.cuda_stream, C.byref(graph)) == 0
    n = C.c_size_t(0)
    assert hip.hipGraphGetRootNodes(graph, None, C.byref(n)) == 0
    assert hip.hipGraphDestroy(graph) == 0
    assert n.value == 2
