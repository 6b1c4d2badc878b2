"""The edge->node sum of the fused narrow kernels (k_block_wave: rows of a node's segment read from LDS in batches, added in edge order) and the
wait in front of it: ef', nf' and gf' are BIT for bit what the commit before the batched sum computed, and within the usual bound of the float64
oracle.  Through gnx_block_forward, gnx_block_forward_steps (20 steps on 9 buffer sets: runs of 8, 8 and 4, the later ones carrying the graph
updates of the run before) and the bf16 entries, on one graph and on a batch of three, at (10,5,0) => (3,4,5) and (3,4,5) => (3,4,5) (a gf
term).  The expected bits are tests/golden/segment_sum/parent.npz, recorded on an MI355X with that commit's library
(`python -m tests.test_gpu_segment_sum --record`); a directory of its own, because tests/test_golden.py takes every .npz directly under
tests/golden for an oracle vector.

The graph is built from a list of in-degrees (wave tiles are cut greedily: nodes join a tile while it has <= 64 nodes and <= 128 in-edges):
  tile 0  in-degrees 0 1 3 4 5 7 8 9 2 0: every remainder of a batch of four rows, a zero-degree node first and last in the tile
  tile 1  90 + 38: exactly 128 edges, both edge slots of every lane
  tile 2  one node with 300 in-edges: the single-node path, three chunks (the reload path)
  tile 3  64 nodes without an in-edge: a tile without edges
  ...     small degrees, 64 nodes per tile
  last    one node with 60 in-edges: a single-node tile whose second edge slot is empty"""
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

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "segment_sum", "parent.npz")
BF = torch.bfloat16
README = ((10, 5, 0), (3, 4, 5))
EX1OUT = ((3, 4, 5), (3, 4, 5))
DEGREES = [0, 1, 3, 4, 5, 7, 8, 9, 2, 0] + [90, 38] + [300] + [0] * 64 + [0, 1, 0, 2, 0, 1, 0, 3] * 28 + [0, 6] + [120, 60]
N_INPUTS, N_STEPS, N_SETS = 2, 20, 9


def _csc_from_degrees(rng, deg):
    n = len(deg)
    colptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    rowval = np.concatenate([np.sort(rng.choice(n, d, replace=False)) for d in deg]).astype(np.int64)
    return colptr, rowval


def _batch(gn, shape):
    rng = np.random.default_rng(20260)
    parts = [_csc_from_degrees(rng, DEGREES)]
    if shape == "three":  # two small graphs behind it: workgroups that straddle graphs, one partial row per wave tile
        parts += [_csc_from_degrees(rng, list(rng.integers(0, 10, n))) for n in (40, 70)]
    g = gn.GNGraphBatch.from_csc([p[0] for p in parts], [p[1] for p in parts], [len(p[0]) - 1 for p in parts])
    assert g.max_in_degree == 300
    return g


def _tiles(gn, g):
    import ctypes as C
    n = C.c_int64(0)
    gn._lib.check(gn._lib.load().gnx_graphs_get_table(g._h, 7, None, 0, C.byref(n)))
    buf = np.zeros(n.value // 4, dtype=np.int32)
    gn._lib.check(gn._lib.load().gnx_graphs_get_table(g._h, 7, buf.ctypes.data, buf.nbytes, C.byref(n)))
    return buf.reshape(-1, 8)  # n0, n1, e0, e1, g, ...


def _key(shape, dims, dtype):
    return f"{shape}-{'readme' if dims is README else 'ex1out'}-{'bf16' if dtype is BF else 'f32'}"


class Case:
    def __init__(self, gn, shape, dims, dtype):
        self.key = _key(shape, dims, dtype)
        self.g = g = _batch(gn, shape)
        rng = np.random.default_rng(77)
        self.p = O.make_block_params(rng, *dims, act=(1, 0, 2))
        self.plan = gn.BlockPlan(U.block_from_params(gn, self.p), g, dtype=dtype)
        self.np_inputs, self.inputs = [], []
        for _ in range(N_INPUTS):
            x = [None if a is None else (a * 4 - 2).astype(np.float32) for a in U.packed_inputs(rng, 1, g.n_edges, g.n_nodes, g.n_graphs, dims[0])]
            t = [None if a is None else torch.from_numpy(a).to(g.device).to(dtype).contiguous() for a in x]
            self.inputs.append(t)
            self.np_inputs.append([None if a is None else a.float().cpu().numpy() for a in t])  # (what the kernel reads: rounded once for bf16)
        self.dtype = dtype

    def separate(self):
        outs = []
        for x in self.inputs:
            o = self.plan.outputs()
            self.plan(*x, *o)
            outs.append(o)
        torch.cuda.synchronize()
        return outs

    def steps(self):
        sets = [(self.plan.outputs(), self.plan.new_workspace()) for _ in range(N_SETS)]
        seq = [dict(ef=x[0], nf=x[1], gf=x[2], out=sets[i % N_SETS][0], ws=sets[i % N_SETS][1]) for i, x in ((i, self.inputs[i % N_INPUTS]) for i in range(N_STEPS))]
        for o, _ in sets:
            for t in o:
                t.view(torch.int16).fill_(0x7FC1)
        self.plan.steps(seq)
        torch.cuda.synchronize()
        last = {}
        for i, b in enumerate(seq):
            last[id(b["out"][0])] = i
        return [(i % N_INPUTS, seq[i]["out"]) for i in sorted(last.values())]  # (input, outputs) of the last step on every set


def _bits(t):
    return t.view(torch.int16 if t.dtype is BF else torch.int32).cpu().numpy()


CASES = [(s, d, t) for s in ("one", "three") for d in (README, EX1OUT) for t in (torch.float32, BF)]


@pytest.fixture(scope="module")
def gn():
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_the_graph_has_the_tiles_the_cases_are_about(gn):
    t = _tiles(gn, _batch(gn, "one"))
    nn, ne = t[:, 1] - t[:, 0], t[:, 3] - t[:, 2]
    assert (nn[0], ne[0]) == (10, 39) and (nn[1], ne[1]) == (2, 128) and (nn[2], ne[2]) == (1, 300) and (nn[3], ne[3]) == (64, 0), t[:4]
    assert (nn[-1], ne[-1]) == (1, 60), t[-1]
    assert len(t) > 8 and _tiles(gn, _batch(gn, "three"))[-1][4] == 2


@pytest.mark.parametrize("shape,dims,dtype", [pytest.param(*c, id=_key(*c)) for c in CASES])
def test_bits_of_the_parent_commit_and_oracle_bound(gn, golden, shape, dims, dtype):
    case = Case(gn, shape, dims, dtype)
    want = [[golden[f"{case.key}-{i}-{n}"] for n in ("ef", "nf", "gf")] for i in range(N_INPUTS)]
    sep = case.separate()
    for i, outs in enumerate(sep):
        for n, o, w in zip(("ef'", "nf'", "gf'"), outs, want[i]):
            d = int((_bits(o) != w).sum())
            assert d == 0, f"{case.key}: separate forward, input {i}, {n}: {d} of {w.size} values differ from the parent commit's bits"
    for i, outs in case.steps():
        for n, o, w in zip(("ef'", "nf'", "gf'"), outs, want[i]):
            d = int((_bits(o) != w).sum())
            assert d == 0, f"{case.key}: steps, input {i}, {n}: {d} of {w.size} values differ from the parent commit's bits"
    g = case.g
    for i, outs in enumerate(sep):
        ref, scale = O.block_forward_sparse(case.p, (*g.csc(), g.node_off, g.edge_off), *case.np_inputs[i], return_scale=True)
        for n, o, r, s in zip(("ef'", "nf'", "gf'"), outs, ref, scale):
            got = o.float().cpu().numpy()
            if dtype is BF:  # half a bf16 ulp of the output on top of the fp32 bound (tests/test_gpu_bf16_block.py)
                ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(r), 1e-30))) - 7)
                assert np.all(np.abs(got.astype(np.float64) - r) <= 0.5 * ulp + U.RTOL * s + 1e-30), f"{case.key}: input {i}, {n}"
            else:
                U.assert_close(got, r, s, f"{case.key}: input {i}, {n}")


def record(path=GOLDEN):
    """the outputs of separate forwards with the library in use, as bit patterns (run with the build of the commit before the batched sum)"""
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    out = {}
    for c in CASES:
        case = Case(gn, *c)
        for i, outs in enumerate(case.separate()):
            for n, o in zip(("ef", "nf", "gf"), outs):
                out[f"{case.key}-{i}-{n}"] = _bits(o)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print("recorded", len(out), "arrays,", os.path.getsize(path), "bytes:", path)


if __name__ == "__main__":
    if "--record" in sys.argv:
        record(sys.argv[sys.argv.index("--record") + 1] if len(sys.argv) > sys.argv.index("--record") + 1 else GOLDEN)
