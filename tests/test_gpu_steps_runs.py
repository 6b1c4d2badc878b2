"""Runs of gnx_block_forward_steps: a full window of neighbouring steps whose buffers do not overlap (or the last four or more of the loop) shares one launch (k_block_wave_run, one slot
per step) and one launch for their graph updates.  Every output of every step is bit for bit what separate gnx_block_forward(_typed) calls give — eagerly
and from a captured graph replayed twice, at every run maximum (GNX_STEPS_RUN_MAX is read once per process: the other maxima run in a child
process each), for step counts around the run maximum and 1, 2, 3 and 9 rotating buffer sets; steps that conflict fall back to runs of one; an
invalid step inside a would-be run reports today's error with the earlier steps complete; and a run stays inside its slots' buffers."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import gn_oracle as O  # noqa: E402
from tests import util as U  # noqa: E402
from tests.arena import Arena  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
README = ((10, 5, 0), (3, 4, 5))
EX1OUT = ((3, 4, 5), (3, 4, 5))
NO_FORK = 0x1000
SET_COUNTS = (1, 2, 3, 9)


def _default_run_max():
    with open(os.path.join(ROOT, "graphnets.jl_amd", "csrc", "gnx_forward.hip")) as f:
        return int(re.search(r"kStepsRunDefault = (\d+);", f.read()).group(1))


def _run_max():
    v = os.environ.get("GNX_STEPS_RUN_MAX")
    return min(max(int(v), 1), 8) if v else _default_run_max()


def _step_counts(rm):
    return sorted({1, 2, rm, rm + 1, 2 * rm + 3})


def _gn():
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


@pytest.fixture(scope="module")
def gn():
    import __graft_entry__ as ge
    ge.build()
    return _gn()


def _table_bytes(gn, g, which):
    n = C.c_int64(0)
    gn._lib.check(gn._lib.load().gnx_graphs_get_table(g._h, which, None, 0, C.byref(n)))
    return n.value


def _pairs_csc(N, src, dst):
    k = np.unique(dst.astype(np.int64) * N + src.astype(np.int64))
    dst, src = k // N, k % N
    colptr = np.zeros(N + 1, dtype=np.int64)
    np.add.at(colptr, dst + 1, 1)
    return np.cumsum(colptr), src.astype(np.int64)


def _batch(gn, shape):
    rng = np.random.default_rng(4242)
    if shape == "one":  # ~300 nodes / ~3000 edges: several wave tiles, a last workgroup with inactive waves
        for n in range(300, 340):
            cp, rv = U.er_csc(rng, n, 10 * n)
            g = gn.GNGraphBatch.from_csc([cp], [rv], [n])
            n_wt = _table_bytes(gn, g, 7) // 32
            if n_wt > 8 and n_wt % 4 != 0:
                return g
        raise AssertionError("no candidate graph leaves the last workgroup partly empty")
    if shape == "three":  # three graphs, each of more than 8 wave tiles: the two-launch form, workgroups that straddle two graphs
        parts = [U.er_csc(rng, n, e) for n, e in ((333, 2221), (701, 5003), (458, 3001))]
        g = gn.GNGraphBatch.from_csc([p[0] for p in parts], [p[1] for p in parts], [len(p[0]) - 1 for p in parts])
        assert _table_bytes(gn, g, 8) == 0, "the batch has a pack table: the pack form would be chosen"
        ids = _wtile_graph_ids(gn, g)  # a workgroup is four consecutive wave tiles
        assert any(ids[w] != ids[min(w + 3, len(ids) - 1)] for w in range(0, len(ids), 4)), "no workgroup straddles two graphs"
        return g
    # "hub": one graph with a node of more than 128 in-edges (a single-node tile of several chunks)
    N, E, hub = 400, 2500, 300
    hs = rng.choice(N, hub, replace=False)
    cp, rv = _pairs_csc(N, np.concatenate([rng.integers(0, N, E), hs]), np.concatenate([rng.integers(0, N, E), np.full(hub, N // 2)]))
    g = gn.GNGraphBatch.from_csc([cp], [rv], [N])
    assert g.max_in_degree > 128
    return g


def _wtile_graph_ids(gn, g):
    n = _table_bytes(gn, g, 7)
    buf = np.zeros(n // 4, dtype=np.int32)
    got = C.c_int64(0)
    gn._lib.check(gn._lib.load().gnx_graphs_get_table(g._h, 7, buf.ctypes.data, buf.nbytes, C.byref(got)))
    return buf.reshape(-1, 8)[:, 4].tolist()


class Case:
    """a batch, a block, a plan; distinct inputs for every step, nine output / workspace sets, and the reference of every step (separate
    forwards, computed once and never written again)"""

    def __init__(self, gn, shape, dims, dtype, n_max, flags=0):
        self.gn, self.dims, self.dtype = gn, dims, dtype
        self.g = _batch(gn, shape)
        rng = np.random.default_rng(99)
        self.blk = U.block_from_params(gn, O.make_block_params(rng, *dims, act=(1, 0, 2)))
        self.plan = gn.BlockPlan(self.blk, self.g, flags=self.blk.flags | flags, dtype=dtype)
        g = self.g
        gen = torch.Generator(device=g.device).manual_seed(7)
        mk = lambda T, d: (torch.rand((1, T, d), device=g.device, generator=gen) * 4 - 2).to(dtype) if d > 0 else None
        de, dn, dg = dims[0]
        self.inputs = [(mk(g.n_edges, de), mk(g.n_nodes, dn), mk(g.n_graphs, dg)) for _ in range(n_max)]
        self.sets = [(self.plan.outputs(), self.plan.new_workspace()) for _ in range(max(SET_COUNTS))]
        self.ref = []
        for x in self.inputs:
            out = self.plan.outputs()
            self.plan(*x, *out)
            self.ref.append(out)
        torch.cuda.synchronize()

    def seq(self, n_steps, n_sets):
        return [dict(ef=x[0], nf=x[1], gf=x[2], out=self.sets[i % n_sets][0], ws=self.sets[i % n_sets][1]) for i, x in zip(range(n_steps), self.inputs)]

    def poison(self, seq):
        for b in seq:
            for t in b["out"]:
                if t is not None:
                    t.view(torch.int16).fill_(0x7FC1)  # NaNs no forward writes

    def assert_bits(self, seq, what, steps=None, ref=None):
        ref = self.ref if ref is None else ref
        if steps is None:  # the last step that wrote each output set
            last = {}
            for i, b in enumerate(seq):
                last[id(b["out"][0])] = i
            steps = sorted(last.values())
        for i in steps:
            for name, a, r in zip(("ef", "nf", "gf"), seq[i]["out"], ref[i]):
                if a is not None and not torch.equal(a.view(torch.int16), r.view(torch.int16)):
                    n = int((a.view(torch.int16) != r.view(torch.int16)).sum())
                    raise AssertionError(f"{what}: step {i} {name}: {n} of {a.numel()} values differ from the separate forward")

    def eager_and_captured(self, seq, what, steps=None, ref=None, plan=None):
        plan = self.plan if plan is None else plan
        self.poison(seq)
        plan.steps(seq)
        torch.cuda.synchronize()
        self.assert_bits(seq, f"{what}, eager", steps, ref)
        self.poison(seq)
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg, capture_error_mode="thread_local"):
            plan.steps(seq)
        for rep in range(2):
            self.poison(seq)
            cg.replay()
            torch.cuda.synchronize()
            self.assert_bits(seq, f"{what}, captured, replay {rep}", steps, ref)
        del cg


def _sweep(gn, shape, dims, dtype):
    rm = _run_max()
    counts = _step_counts(rm)
    case = Case(gn, shape, dims, dtype, max(counts))
    for n_steps in counts:
        for n_sets in SET_COUNTS:
            case.eager_and_captured(case.seq(n_steps, n_sets), f"{shape} {dims} {dtype} run max {rm}: {n_steps} steps on {n_sets} sets")
    return case


SHAPES = ("one", "three", "hub")
GRID = [pytest.param(s, d, t, id=f"{s}-{'readme' if d is README else 'ex1out'}-{'bf16' if t is BF else 'f32'}")
        for s in SHAPES for d in (README, EX1OUT) for t in (torch.float32, BF)]


@pytest.mark.parametrize("shape,dims,dtype", GRID)
def test_runs_match_separate_forwards(gn, shape, dims, dtype):
    _sweep(gn, shape, dims, dtype)


def child_main():
    """the sweep at the run maximum of this process's GNX_STEPS_RUN_MAX (the variable is read once per process)"""
    gn = _gn()
    for shape, dims, dtype in (("one", README, torch.float32), ("three", EX1OUT, BF), ("hub", EX1OUT, torch.float32), ("one", README, BF)):
        _sweep(gn, shape, dims, dtype)
    print(f"runs child ok {_run_max()}")


@pytest.mark.parametrize("rm", [m for m in (1, 2, 4, 8) if m != _run_max()])  # (this process's own: test_runs_match_separate_forwards)
def test_every_other_run_maximum_in_a_process_of_its_own(gn, rm):
    env = dict(os.environ, GNX_STEPS_RUN_MAX=str(rm))
    r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_steps_runs as t; t.child_main()"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"runs child ok {rm}" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _hip():
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln)
    hip = C.CDLL(path)
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    return hip


def _captured_nodes(case, seq, plan=None):
    """the kernel launches of the call, counted in a graph captured from it"""
    hip = _hip()
    torch.cuda.synchronize()
    st = torch.cuda.Stream(case.g.device)
    assert hip.hipStreamBeginCapture(st.cuda_stream, 1) == 0  # hipStreamCaptureModeThreadLocal
    (case.plan if plan is None else plan).steps(seq, stream=st.cuda_stream)
    graph = C.c_void_p()
    assert hip.hipStreamEndCapture(st.cuda_stream, C.byref(graph)) == 0
    n = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0
    nodes = (C.c_void_p * max(n.value, 1))()
    assert hip.hipGraphGetNodes(graph, nodes, C.byref(n)) == 0
    kernels = 0
    for i in range(n.value):
        t = C.c_int(-1)
        assert hip.hipGraphNodeGetType(nodes[i], C.byref(t)) == 0
        kernels += t.value == 0  # hipGraphNodeTypeKernel
    assert hip.hipGraphDestroy(graph) == 0
    return kernels


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_runs_are_formed_and_conflicts_fall_back_to_single_steps(gn, dtype):
    """the captured call's launches: two per full run of steps on disjoint sets; one per step (+ the flushes) when every step conflicts with
    its predecessor — the recurrent loop x_{i+1} = block(x_i) and steps on one workspace — whose results are bit-equal all the same"""
    rm = _run_max()
    K = 2 * rm + 1 if rm > 1 else 5
    case = Case(gn, "one", EX1OUT, dtype, K)
    free = [dict(b, out=case.plan.outputs(), ws=case.plan.new_workspace()) for b in case.seq(K, 1)]  # a set of its own for every step
    n_free = _captured_nodes(case, free)
    if rm > 1:
        # two full runs; the last step is a single chained step + its flush: two launches as well
        assert n_free == 2 * -(-K // rm), (n_free, K, rm)
    # the recurrent loop: step i + 1 reads step i's outputs
    x0 = case.inputs[0]
    rec, src, ref = [], x0, []
    for _ in range(K):
        out = case.plan.outputs()
        rec.append(dict(ef=src[0], nf=src[1], gf=src[2], out=out, ws=case.plan.new_workspace()))
        src = out
    for b in rec:  # separate forwards in order; what each step's outputs held
        case.plan(b["ef"], b["nf"], b["gf"], *b["out"], ws=b["ws"])
        ref.append([t.clone() for t in b["out"]])
    torch.cuda.synchronize()
    assert _captured_nodes(case, rec) >= K
    case.eager_and_captured(rec, "recurrent loop", steps=range(K), ref=ref)
    plan1 = gn.BlockPlan(case.blk, case.g, flags=case.plan.flags | NO_FORK, dtype=dtype)
    case.eager_and_captured(rec, "recurrent loop, one stream", steps=range(K), ref=ref, plan=plan1)
    # every step on ONE workspace (distinct outputs)
    outs = [case.plan.outputs() for _ in range(K)]
    shared = [dict(b, out=o, ws=case.sets[0][1]) for b, o in zip(case.seq(K, 1), outs)]
    assert _captured_nodes(case, shared) >= K
    case.eager_and_captured(shared, "one workspace", steps=range(K))
    case.eager_and_captured(shared, "one workspace, one stream", steps=range(K), plan=plan1)
    # runs on one stream (GNX_FLAG_NO_FORK): formed all the same, issued in order
    if rm > 1:
        assert _captured_nodes(case, free, plan1) == 2 * -(-K // rm)
    case.eager_and_captured(free, "disjoint sets, one stream", steps=range(K), plan=plan1)


def _step_array(gn, seq, null_ef_out=None):
    P = lambda t: None if t is None else t.data_ptr()
    arr = (gn._lib.BlockStep * len(seq))()
    for i, b in enumerate(seq):
        outs = [P(t) for t in b["out"]]
        if i == null_ef_out:
            outs[0] = None
        arr[i] = gn._lib.BlockStep(P(b["ef"]), P(b["nf"]), P(b["gf"]), *outs, b["ws"].data_ptr(), b["ws"].numel())
    return arr


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_invalid_step_inside_a_would_be_run(gn, dtype):
    """a NULL ef_out at a step that would have joined the first run: the error of a separate forward, the steps before it complete and correct
    once the caller's stream is, and the next call on that stream right"""
    rm = _run_max()
    bad = 2 if rm > 2 else 1
    K = rm + 3
    case = Case(gn, "one", EX1OUT, dtype, K)
    seq = [dict(b, out=case.plan.outputs(), ws=case.plan.new_workspace()) for b in case.seq(K, 1)]  # a set of its own for every step
    case.poison(seq)
    lib = gn._lib.load()
    s = torch.cuda.current_stream(case.g.device)
    b = seq[bad]
    if dtype is BF:
        want = lib.gnx_block_forward_typed(case.g._h, C.byref(case.plan.p), gn._lib.ELEM_BF16, b["ef"].data_ptr(), b["nf"].data_ptr(), b["gf"].data_ptr(), 1, None,
                                           b["out"][1].data_ptr(), b["out"][2].data_ptr(), b["ws"].data_ptr(), b["ws"].numel(), case.plan.flags, s.cuda_stream)
    else:
        want = lib.gnx_block_forward(case.g._h, C.byref(case.plan.p), b["ef"].data_ptr(), b["nf"].data_ptr(), b["gf"].data_ptr(), 1, None, b["out"][1].data_ptr(),
                                     b["out"][2].data_ptr(), b["ws"].data_ptr(), b["ws"].numel(), case.plan.flags, s.cuda_stream)
    assert want == gn._lib.ERR_INVALID_ARG
    arr = _step_array(gn, seq, null_ef_out=bad)
    if dtype is BF:
        rc = lib.gnx_block_forward_steps_typed(case.g._h, C.byref(case.plan.p), gn._lib.ELEM_BF16, arr, len(seq), 1, case.plan.flags, s.cuda_stream)
    else:
        rc = lib.gnx_block_forward_steps(case.g._h, C.byref(case.plan.p), arr, len(seq), 1, case.plan.flags, s.cuda_stream)
    assert rc == want, (rc, lib.gnx_last_error())
    s.synchronize()
    case.assert_bits(seq, f"steps before the invalid step {bad}", steps=range(bad))
    for t in seq[bad]["out"]:
        assert bool((t.view(torch.int16) == 0x7FC1).all()), "the invalid step wrote an output"
    case.poison(seq)
    case.plan.steps(seq)
    s.synchronize()
    case.assert_bits(seq, "the call after the error", steps=range(len(seq)))


@pytest.mark.parametrize("shape,dims,dtype", [pytest.param("hub", README, torch.float32, id="hub-readme-f32"), pytest.param("three", EX1OUT, BF, id="three-ex1out-bf16")])
def test_a_run_stays_inside_its_slots_buffers(gn, shape, dims, dtype):
    """every input, output and workspace of every step of a call of two runs carved out of ONE sentinel-filled arena (tests/arena.py): after the
    call the guard bytes around every carve and every input are untouched, every output element is written, and each slot's outputs are its own
    step's bits — no slot wrote into another slot's buffers"""
    rm = _run_max()
    K = rm + 2
    case = Case(gn, shape, dims, dtype, K)
    a = Arena("cuda")
    names = []
    rows = (case.g.n_edges, case.g.n_nodes, case.g.n_graphs)
    for i, x in enumerate(case.inputs):
        ins = [a.input(f"s{i}.{n}", v) if v is not None else None for n, v in zip(("ef", "nf", "gf"), x)]
        outs = [a.output(f"s{i}.{n}_out", (1, T, d), dtype) if d > 0 else None for n, T, d in zip(("ef", "nf", "gf"), rows, dims[1])]
        names.append((ins, outs, a.workspace(f"s{i}.ws", case.plan.ws.numel())))
    a.build(ws_fill=0x5A)
    V = lambda n: None if n is None else a.view(n)
    seq = [dict(ef=V(ins[0]), nf=V(ins[1]), gf=V(ins[2]), out=tuple(V(o) for o in outs), ws=a.raw(w)) for ins, outs, w in names]
    for form, plan in (("two streams", case.plan), ("one stream", gn.BlockPlan(case.blk, case.g, flags=case.plan.flags | NO_FORK, dtype=dtype))):
        a.refill(0x5A)
        plan.steps(seq)
        torch.cuda.synchronize()
        a.check(f"{shape} {dims} {dtype}, {K} steps at run maximum {rm}, {form}")
        case.assert_bits(seq, f"arena, {form}", steps=range(K))
