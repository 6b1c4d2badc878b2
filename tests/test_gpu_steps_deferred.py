"""Carrying runs of gnx_block_forward_steps: where a run of several steps conflicts with the run before it only in ways that stream order and
two partial-row areas resolve (gnx_step_hazard.h: run_defers), front workgroups of ITS block launch (k_block_wave_carry) finish the previous
run's graph updates and the run writes the partial-row area the previous one did not.  ef', nf' and gf' of EVERY step are bit for bit what K
separate gnx_block_forward calls give: one graph in each of the three summation classes of the graph update (under 256 partial rows, 256 to
1023, 1024 and more), a batch of several graphs in the two-launch form, 16, 20, 12 and 9 steps over 8 workspaces, a rotation of whole buffer
sets, a shared gf_out, gf' fed back into the next run, a dense batch whose second area does not fit, and a captured call replayed three times.
The launches of a captured call are counted as well: a carrying run is one launch, and only the last run of a call has a graph-update launch."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import gn_oracle as O  # noqa: E402
from tests import util as U  # noqa: E402
from tests.test_gpu_steps_runs import _captured_nodes, _table_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

README = ((10, 5, 0), (3, 4, 5))
EX1OUT = ((3, 4, 5), (3, 4, 5))
SETS = 8  # the run maximum: the rotation conflicts run by run
DEFER = os.environ.get("GNX_STEPS_DEFER", "1") != "0" and os.environ.get("GNX_STEPS_RUN_MAX", "8") == "8"


@pytest.fixture(scope="module")
def gn():
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


def _ring_csc(N):
    """one in-edge per node (from its left neighbour): 64 nodes per wave tile"""
    return np.arange(N + 1, dtype=np.int64), (np.arange(N, dtype=np.int64) - 1) % N


def _dense_csc(N, deg):
    """every node has `deg` in-edges (from the next `deg` nodes)"""
    src = (np.arange(N, dtype=np.int64)[:, None] + 1 + np.arange(deg, dtype=np.int64)[None, :]) % N
    return np.arange(N + 1, dtype=np.int64) * deg, np.sort(src, axis=1).reshape(-1)


def _graph(gn, kind):
    rng = np.random.default_rng(2718)
    if kind == "rows<256":
        cp, rv = U.er_csc(rng, 301, 3010)
        return gn.GNGraphBatch.from_csc([cp], [rv], [301])
    if kind == "rows256-1023":
        cp, rv = _ring_csc(70003)
        return gn.GNGraphBatch.from_csc([cp], [rv], [70003])
    if kind == "rows>=1024":
        cp, rv = _ring_csc(270001)
        return gn.GNGraphBatch.from_csc([cp], [rv], [270001])
    if kind == "three-graphs":  # more than 8 wave tiles each: the two-launch form, not the pack form
        parts = [U.er_csc(rng, n, e) for n, e in ((333, 2221), (701, 5003), (458, 3001))]
        return gn.GNGraphBatch.from_csc([p[0] for p in parts], [p[1] for p in parts], [len(p[0]) - 1 for p in parts])
    assert kind == "dense"  # three graphs of 80 nodes with 70 in-edges each: a wave tile (128 edges) holds ONE node
    parts = [_dense_csc(80, 70) for _ in range(3)]
    return gn.GNGraphBatch.from_csc([p[0] for p in parts], [p[1] for p in parts], [80] * 3)


def _partial_rows(gn, g):
    n_wt = _table_bytes(gn, g, 7) // 32
    return (n_wt + 3) // 4 if g.n_graphs == 1 else n_wt


def _area_b_fits(gn, g, dims):
    """the second partial-row area is the head of the workspace's agg area (N x oe floats, rounded up to 256 bytes)"""
    oe, on, _ = dims[1]
    agg = -(-4 * g.n_nodes * oe // 256) * 256
    return agg >= _partial_rows(gn, g) * ((oe + on + 3) // 4 * 4) * 4


class Case:
    """a batch, a block, a plan; K distinct inputs and output sets, 8 workspaces, and every step's reference from a separate forward
    (computed once, never written again)"""

    def __init__(self, gn, kind, dims, K):
        self.gn, self.dims, self.K = gn, dims, K
        self.g = _graph(gn, kind)
        rng = np.random.default_rng(99)
        self.blk = U.block_from_params(gn, O.make_block_params(rng, *dims, act=(1, 0, 2)))
        self.plan = gn.BlockPlan(self.blk, self.g, flags=self.blk.flags, dtype=torch.float32)
        g = self.g
        gen = torch.Generator(device=g.device).manual_seed(7)
        mk = lambda T, d: (torch.rand((1, T, d), device=g.device, generator=gen) * 4 - 2) if d > 0 else None
        de, dn, dg = dims[0]
        self.inputs = [(mk(g.n_edges, de), mk(g.n_nodes, dn), mk(g.n_graphs, dg)) for _ in range(K)]
        self.outs = [self.plan.outputs() for _ in range(K)]
        self.ws = [self.plan.new_workspace() for _ in range(SETS)]
        self.ref = []
        for x in self.inputs:
            out = self.plan.outputs()
            self.plan(*x, *out)
            self.ref.append(out)
        torch.cuda.synchronize()

    def seq(self, K, outs=None):
        """K steps on the 8 workspaces in rotation; outs(i): the output set of step i (default: one of its own)"""
        return [dict(ef=x[0], nf=x[1], gf=x[2], out=outs(i) if outs else self.outs[i], ws=self.ws[i % SETS]) for i, x in zip(range(K), self.inputs)]

    @staticmethod
    def poison(seq):
        for b in seq:
            for t in b["out"]:
                if t is not None:
                    t.view(torch.int32).fill_(0x7FC00001)  # NaNs no forward writes

    def assert_bits(self, seq, what, ref=None):
        """every output tensor against the LAST step that wrote it (with an output set per step: every step)"""
        ref = self.ref if ref is None else ref
        last = {}
        for i, b in enumerate(seq):
            for name, t in zip(("ef", "nf", "gf"), b["out"]):
                if t is not None:
                    last[(name, t.data_ptr())] = (i, t)
        for (name, _), (i, t) in last.items():
            r = ref[i][("ef", "nf", "gf").index(name)]
            if not torch.equal(t.view(torch.int32), r.view(torch.int32)):
                n = int((t.view(torch.int32) != r.view(torch.int32)).sum())
                raise AssertionError(f"{what}: step {i} {name}: {n} of {t.numel()} values differ from the separate forward")

    def run(self, seq, what, ref=None):
        self.poison(seq)
        self.plan.steps(seq)
        torch.cuda.synchronize()
        self.assert_bits(seq, what, ref)


def _launches(K, carried):
    """kernel launches of K steps on 8 workspaces: the runs of 8, a tail of 4 or more as a run, else single steps (each one launch, the last
    one's graph update a launch more)"""
    full, rest = divmod(K, SETS)
    tail = rest >= 4
    runs = full + tail
    singles = 0 if tail else rest
    if not carried:
        return 2 * runs + (singles + 1 if singles else 0)
    # every run but the first is carried ... and the last run's graph updates are flushed (before a single step or at the end of the call)
    return runs + 1 + (singles + 1 if singles else 0)


ONE_GRAPH = {"rows<256": (0, 256), "rows256-1023": (256, 1024), "rows>=1024": (1024, 1 << 30)}


@pytest.mark.parametrize("kind", list(ONE_GRAPH) + ["three-graphs"])
def test_every_step_matches_a_separate_forward(gn, kind):
    case = Case(gn, kind, README, 20)
    rows = _partial_rows(gn, case.g)
    if kind in ONE_GRAPH:
        lo, hi = ONE_GRAPH[kind]
        assert lo <= rows < hi and (kind != "rows<256" or rows > 1), rows
    else:
        assert _table_bytes(gn, case.g, 8) == 0, "the batch has a pack table: the pack form would be chosen"
    assert _area_b_fits(gn, case.g, README)
    for K in (16, 20, 12, 9):
        seq = case.seq(K)
        case.run(seq, f"{kind}: {K} steps on 8 workspaces")
        if DEFER:
            assert _captured_nodes(case, seq) == _launches(K, True), (kind, K)
    # the whole buffer set in rotation (the benchmark's loop): outputs are overwritten run by run
    seq = case.seq(20, outs=lambda i: case.outs[i % SETS])
    case.run(seq, f"{kind}: 20 steps on 8 buffer sets")
    if DEFER:
        assert _captured_nodes(case, seq) == _launches(20, True), kind
    # gf_out in rotation, ef_out / nf_out of its own for every step
    gfo = [case.plan.outputs()[2] for _ in range(SETS)]
    seq = case.seq(16, outs=lambda i: (case.outs[i][0], case.outs[i][1], gfo[i % SETS]))
    case.run(seq, f"{kind}: gf_out in rotation")
    # ONE gf_out for all steps: every step conflicts with its predecessor — single steps
    seq = case.seq(12, outs=lambda i: (case.outs[i][0], case.outs[i][1], gfo[0]))
    case.run(seq, f"{kind}: one gf_out")


def test_captured_and_replayed(gn):
    case = Case(gn, "rows>=1024", README, 20)
    seq = case.seq(20, outs=lambda i: case.outs[i % SETS])
    seq2 = case.seq(20)
    for s, what in ((seq, "8 buffer sets"), (seq2, "8 workspaces")):
        case.poison(s)
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg, capture_error_mode="thread_local"):
            case.plan.steps(s)
        for rep in range(3):
            case.poison(s)
            cg.replay()
            torch.cuda.synchronize()
            case.assert_bits(s, f"captured, {what}, replay {rep}")
        del cg


@pytest.mark.parametrize("kind", ["rows<256", "three-graphs"])
def test_feedback_is_never_carried(gn, kind):
    """(3,4,5) => (3,4,5): step i reads the outputs of step i - 8, so the runs of 8 form and every run reads the gf' of the run before it:
    its graph updates are a launch of their own, as before"""
    K = 20
    case = Case(gn, kind, EX1OUT, SETS)
    seq, ref = [], []
    for i in range(K):
        src = case.inputs[i] if i < SETS else seq[i - SETS]["out"]
        seq.append(dict(ef=src[0], nf=src[1], gf=src[2], out=case.plan.outputs(), ws=case.ws[i % SETS]))
    for b in seq:  # separate forwards, in order
        case.plan(b["ef"], b["nf"], b["gf"], *b["out"])
        ref.append([t.clone() for t in b["out"]])
    torch.cuda.synchronize()
    case.run(seq, f"{kind}: feedback over 8 steps", ref)
    if DEFER:
        assert _captured_nodes(case, seq) == _launches(K, False)


def test_dense_batch_without_room_for_the_second_area(gn):
    """three graphs of in-degree 70: a partial row per node, more than the agg area holds — nothing is carried"""
    case = Case(gn, "dense", README, 16)
    assert _table_bytes(gn, case.g, 8) == 0, "the batch has a pack table: the pack form would be chosen"
    assert not _area_b_fits(gn, case.g, README)
    for K in (16, 12, 9):
        seq = case.seq(K)
        case.run(seq, f"dense: {K} steps on 8 workspaces")
        if DEFER:
            assert _captured_nodes(case, seq) == _launches(K, False), K
