"""The MEMORY contract of every dispatch form of the C ABI (include/gnx.h), on the GPU.

The rest of the suite checks values; this module checks where a call writes.  Every case calls the ABI through `gn._lib.load()` directly with ALL
its buffers — features, weights, gradients, workspaces — carved out of one sentinel-filled arena (tests/arena.py: exact byte sizes, 256-byte
aligned starts — tests/test_gpu_alignment.py runs the same table at 4-byte aligned ones —, 64 KiB of sentinel on both sides of every carve) and asserts, in this order:

  1. the call returns 0;
  2. every byte of the arena outside an output or workspace carve is unchanged (guards intact, inputs bit-identical) and no output element still
     holds the 0xFF bytes it was given;
  3. the outputs meet the float64 oracle at the suite's bound (U.assert_close at U.RTOL; the backward cases at the bars of
     tests/test_gpu_backward.py and tests/test_gpu_chain.py) — so a case cannot pass by running nothing;
  4. the same call with the workspace pre-filled with 0x00 and with 0xFF bytes gives bit-identical outputs (for the chained / deferred / steps
     forms, which by contract read what the previous step left in a workspace, the poison goes in before the first step only);
  5. a third, profiled run (one stream) passes 1-3 too and records the kernel names it saw.

`test_every_profiled_kernel_name_is_covered` then requires every name the sources hand to the profiler to have been seen in some case, or to
stand in NOT_COVERED with its reason: a kernel added later without a contract case fails it.  tests/test_arena_cpu.py proves, without a GPU,
that the checker reports each situation it exists for."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import gn_oracle as O
from tests import arena as AR
from tests import util as U
from tests.test_gpu_backward import ACT, _torch_block, _torch_ln
from tests.test_gpu_chain import _torch_chain_block

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SEEN = {}   # case id -> kernel names of its profiled run
DONE = set()

# names the profiler can report that no contract case is required to show (at most 4, none of them a kernel that writes a caller's buffer)
NOT_COVERED = {
    "__empty_bracket__": "the profiler's own calibration launch (gnx_profile_calibrate): an empty kernel, no caller buffer",
}


@pytest.fixture(scope="module")
def gn():
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


# ---------------------------------------------------------------------------------------------------------------------------------------
# graphs: shapes chosen for where a tail goes wrong
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pairs_csc(N, src, dst):
    k = np.unique(dst.astype(np.int64) * N + src.astype(np.int64))
    dst, src = k // N, k % N
    colptr = np.zeros(N + 1, dtype=np.int64)
    np.add.at(colptr, dst + 1, 1)
    return np.cumsum(colptr), src.astype(np.int64)


def _from_csc(gn, parts):
    g = gn.GNGraphBatch.from_csc([p[0] for p in parts], [p[1] for p in parts], [int(len(p[0]) - 1) for p in parts])
    return g, (*g.csc(), g.node_off, g.edge_off)


def g_er(N, E, seed=1):
    """one Erdos-Renyi graph with exactly E edges"""
    return lambda gn: _from_csc(gn, [U.er_csc(np.random.default_rng(seed), N, E)])


def g_hub(N, E, hub_deg, isolated=17, seed=2):
    """one graph: ~E random edges among the first N - isolated nodes, one hub with hub_deg in-edges (several tiles), isolated nodes at the end"""
    def make(gn):
        rng = np.random.default_rng(seed)
        M = N - isolated
        hs = rng.choice(M, hub_deg, replace=False)
        return _from_csc(gn, [_pairs_csc(N, np.concatenate([rng.integers(0, M, E), hs]), np.concatenate([rng.integers(0, M, E), np.full(hub_deg, M // 2)]))])
    return make


def g_small(seed=3, n=41):
    """many small graphs (the pack form): a one-node graph with and without its self loop, a graph without edges, a hub, isolated nodes"""
    def make(gn):
        rng = np.random.default_rng(seed)
        adjs = U.random_graphs(rng, [int(v) for v in rng.integers(2, 40, n)], 0.3)
        adjs[0] = np.zeros((1, 1), dtype=np.int64)
        adjs[5] = np.ones((1, 1), dtype=np.int64)
        adjs[7][:] = 0                      # a graph without edges inside the batch
        adjs[9] = np.zeros((37, 37), dtype=np.int64)
        adjs[9][:, 11] = 1                  # every node -> node 11 ...
        adjs[9][30:, :] = 0                 # ... and nodes without out-edges
        adjs[9][:, 30:] = 0                 # ... or in-edges: isolated
        g = gn.GNGraphBatch(adjs)
        return g, O.csc_from_adj(adjs)
    return make


def g_medium(seed=4):
    """three graphs of different sizes, ragged against every tile size"""
    def make(gn):
        rng = np.random.default_rng(seed)
        return _from_csc(gn, [U.er_csc(rng, n, e) for n, e in ((333, 2221), (1, 1), (701, 5003))])
    return make


def g_no_edges(gn):
    adjs = [np.zeros((n, n), dtype=np.int64) for n in (3, 5, 1, 2)]
    return gn.GNGraphBatch(adjs), O.csc_from_adj(adjs)


def g_big3(seed=5):
    """three graphs with >= 4096 nodes and edges in all: the matrix-core pullbacks of the backward"""
    def make(gn):
        rng = np.random.default_rng(seed)
        return _from_csc(gn, [U.er_csc(rng, n, 4 * n + 3) for n in (1501, 1777, 2003)])
    return make


# ---------------------------------------------------------------------------------------------------------------------------------------
# descriptors whose device pointers point into the arena
# ---------------------------------------------------------------------------------------------------------------------------------------
def _L(gn):
    return gn._lib


def _decl(a, name, arr):
    """an input carve for a numpy array / tensor (None: `nothing`); returns the carve's name or None"""
    if arr is None:
        return None
    return a.input(name, arr)


def _colmajor(W):
    """(out, in) weight -> the bytes of Flux's column-major Dense.weight: W[k * out + j]"""
    return np.ascontiguousarray(np.asarray(W, dtype=np.float32).T)


def _decl_dense(a, name, W, b):
    a.input(name + ".W", _colmajor(W))
    a.input(name + ".b", np.asarray(b, dtype=np.float32))


def _dense(gn, a, name, act, kind=0):
    p = lambda n: a.ptr(n) if a.nbytes(n) else None
    return _L(gn).Dense(p(name + ".W"), p(name + ".b"), int(act), kind)


def _decl_block(a, p, pfx="blk"):
    for fn, w, b in (("edgefn", "We", "be"), ("nodefn", "Wn", "bn"), ("graphfn", "Wg", "bg")):
        _decl_dense(a, f"{pfx}.{fn}", p[w], p[b])


def _block_params(gn, a, p, pfx="blk"):
    q = _L(gn).BlockParams()
    q.de, q.dn, q.dg = p["in_dims"]
    q.oe, q.on, q.og = p["out_dims"]
    q.edgefn, q.nodefn, q.graphfn = (_dense(gn, a, f"{pfx}.{fn}", p[k]) for fn, k in (("edgefn", "act_e"), ("nodefn", "act_n"), ("graphfn", "act_g")))
    return q


def _decl_core(a, p):
    _decl_block(a, p["block"], "core.blk")
    for t in "eng":
        for ln in ("ln1", "ln2"):
            a.input(f"core.{ln}_{t}.gamma", p[f"{ln}_{t}_gamma"])
            a.input(f"core.{ln}_{t}.beta", p[f"{ln}_{t}_beta"])
        _decl_dense(a, f"core.ff_{t}.fc1", p[f"ff_{t}_W1"], p[f"ff_{t}_b1"])
        _decl_dense(a, f"core.ff_{t}.fc2", p[f"ff_{t}_W2"], p[f"ff_{t}_b2"])


def _core_params(gn, a, p, hidden_act=1):
    q = _L(gn).CoreParams()
    q.block = _block_params(gn, a, p["block"], "core.blk")
    for i, t in enumerate("eng"):
        q.ln1[i].gamma, q.ln1[i].beta = a.ptr(f"core.ln1_{t}.gamma"), a.ptr(f"core.ln1_{t}.beta")
        q.ln2[i].gamma, q.ln2[i].beta = a.ptr(f"core.ln2_{t}.gamma"), a.ptr(f"core.ln2_{t}.beta")
        q.ff[i].fc1, q.ff[i].fc2 = _dense(gn, a, f"core.ff_{t}.fc1", hidden_act), _dense(gn, a, f"core.ff_{t}.fc2", 0)
    q.eps, q.eps_mode = p["eps"], p["eps_mode"]
    return q


def _rows(g):
    return (g.n_edges, g.n_nodes, g.n_graphs)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _decl_outputs(a, pfx, R, rows, widths, dtype=F32):
    """output carves [R][T][d] for every width > 0; names or None"""
    return [a.output(f"{pfx}{n}", (R, T, d), dtype) if d > 0 else None for n, T, d in zip(("ef_out", "nf_out", "gf_out"), rows, widths)]


def _check_outputs(a, names, ref, scale, what):
    for n, r, s in zip(names, ref, scale):
        if n is None:
            assert r is None, what
            continue
        U.assert_close(a.numpy(n), r, s, f"{what} {n}")


def _check_bf16_outputs(a, names, ref, scale, what):
    """bf16 outputs against the float64 oracle of the widened inputs: half a bf16 ulp of the result plus the fp32 bound 1e-5 . S
    (tests/test_gpu_bf16_block.py::test_oracle_readme_dims)"""
    for n, r, s in zip(names, ref, scale):
        if n is None:
            continue
        got = a.numpy(n).astype(np.float64)
        assert got.shape == r.shape, (what, n)
        ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(r), 1e-30))) - 7)
        bad = ~(np.abs(got - r) <= 0.5 * ulp + U.RTOL * s + 1e-30)
        assert not bad.any(), f"{what} {n}: {int(bad.sum())} of {bad.size} outside half a bf16 ulp + 1e-5 . S"


def _inputs(rng, R, g, dims, bf16=False):
    ef, nf, gf = U.packed_inputs(rng, R, g.n_edges, g.n_nodes, g.n_graphs, dims)
    if not bf16:
        return ef, nf, gf
    mk = lambda x: None if x is None else torch.from_numpy((x * 4 - 2).astype(np.float32)).to(BF16)  # both signs, a few binades; the inputs ARE bf16
    return mk(ef), mk(nf), mk(gf)


def _widen(x):
    return None if x is None else x.float().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GNBlock forward in its entry points
# ---------------------------------------------------------------------------------------------------------------------------------------
def block_case(graph, in_dims, out_dims, R=1, flags=0, act=(1, 0, 2), seed=0, entry="plain", bf16=False, n_steps=1, flag_names=()):
    """entry: plain (gnx_block_forward) | typed (gnx_block_forward_typed) | deferred (+ gnx_block_graph_update) | chained
    (gnx_block_forward_chained over n_steps batches on two alternating workspaces, then the flush) | steps (gnx_block_forward_steps; the last two
    steps share a workspace, as the contract allows) | steps_typed"""
    def setup(gn, a):
        L, lib = _L(gn), _L(gn).load()
        fl = flags
        for n in flag_names:
            fl |= getattr(L, "FLAG_" + n)
        g, csc = graph(gn)
        rng = np.random.default_rng(1000 + seed)
        p = O.make_block_params(rng, in_dims, out_dims, act=act)
        _decl_block(a, p)
        typed = entry in ("typed", "steps_typed")
        elem = L.ELEM_BF16 if bf16 else L.ELEM_F32
        dt = BF16 if bf16 else F32
        steps = []
        for i in range(n_steps):
            x = _inputs(rng, R, g, in_dims, bf16)
            ins = [_decl(a, f"s{i}.{n}", v) for n, v in zip(("ef", "nf", "gf"), x)]
            outs = _decl_outputs(a, f"s{i}.", R, _rows(g), out_dims, dt)
            steps.append((x, ins, outs))
        q = lambda: (lib.gnx_block_typed_workspace_bytes(g._h, C.byref(_block_params(gn, a, p)), R, elem, fl) if typed
                     else lib.gnx_block_workspace_bytes(g._h, C.byref(_block_params(gn, a, p)), R))
        if entry == "chained":
            n_ws = min(2, n_steps)
        elif entry in ("steps", "steps_typed"):
            n_ws = max(n_steps - 1, 1)  # the last two steps share one
        else:
            n_ws = 1
        wss = [a.workspace(f"ws{i}", q) for i in range(n_ws)]

        def run(a):
            for w in wss:
                assert a.nbytes(w) > 0, lib.gnx_last_error()
            bp = _block_params(gn, a, p)
            s = _stream()
            P = a.ptr
            if entry in ("plain", "typed", "deferred"):
                (x, ins, outs), w = steps[0], wss[0]
                if entry == "typed":
                    return lib.gnx_block_forward_typed(g._h, C.byref(bp), elem, *map(P, ins), R, *map(P, outs), P(w), a.nbytes(w), fl, s)
                if entry == "plain":
                    return lib.gnx_block_forward(g._h, C.byref(bp), *map(P, ins), R, *map(P, outs), P(w), a.nbytes(w), fl, s)
                rc = lib.gnx_block_forward(g._h, C.byref(bp), *map(P, ins), R, *map(P, outs), P(w), a.nbytes(w), fl | L.FLAG_DEFER_GRAPH_UPDATE, s)
                if rc or outs[2] is None:
                    return rc
                return lib.gnx_block_graph_update(g._h, C.byref(bp), P(ins[2]), R, P(outs[2]), P(w), a.nbytes(w), fl, s)
            if entry == "chained":
                pend = None
                for i, (x, ins, outs) in enumerate(steps):
                    w = wss[i & 1]
                    nxt = L.PendingUpdate()
                    rc = lib.gnx_block_forward_chained(g._h, C.byref(bp), *map(P, ins), R, *map(P, outs), P(w), a.nbytes(w), fl, s,
                                                       C.byref(pend) if pend is not None else None, C.byref(nxt))
                    if rc:
                        return rc
                    pend = nxt
                if pend is not None and pend.workspace:
                    return lib.gnx_block_graph_update(g._h, C.byref(bp), pend.gf, R, pend.gf_out, pend.workspace, pend.workspace_bytes, fl, s)
                return 0
            arr = (L.BlockStep * n_steps)()
            for i, (x, ins, outs) in enumerate(steps):
                w = wss[min(i, n_ws - 1)]
                arr[i] = L.BlockStep(*map(P, ins), *map(P, outs), P(w), a.nbytes(w))
            if entry == "steps":
                return lib.gnx_block_forward_steps(g._h, C.byref(bp), arr, n_steps, R, fl, s)
            return lib.gnx_block_forward_steps_typed(g._h, C.byref(bp), elem, arr, n_steps, R, fl, s)

        refs = []

        def verify(a, what):
            if not refs:  # (the oracle runs once per case)
                for x, _, _ in steps:
                    xs = [_widen(v) for v in x] if bf16 else x
                    refs.append(O.block_forward_sparse(p, csc, *xs, return_scale=True))
            for i, ((x, ins, outs), (ref, scale)) in enumerate(zip(steps, refs)):
                (_check_bf16_outputs if bf16 else _check_outputs)(a, outs, ref, scale, f"{what} step {i}")
        return run, verify
    return setup


# ---------------------------------------------------------------------------------------------------------------------------------------
# GNCore forward (test mode and training mode) and backward
# ---------------------------------------------------------------------------------------------------------------------------------------
def _torch_core(p, csc, xs, W, Wb, hidden_fn, masks=None):
    """float64 torch restatement of y = x + block(gn1(x)) + m .* ffwd(gn2(x)) (one replica) — tests/test_gpu_backward.py's, with the masks of
    tests/test_gpu_dropout.py"""
    em = p["eps_mode"]
    l1 = [_torch_ln(x, W[f"ln1_{t}_gamma"], W[f"ln1_{t}_beta"], p["eps"], em) for x, t in zip(xs, "eng")]
    l2 = [_torch_ln(x, W[f"ln2_{t}_gamma"], W[f"ln2_{t}_beta"], p["eps"], em) for x, t in zip(xs, "eng")]
    blk = _torch_block(p["block"], csc, l1[0], l1[1], l1[2], Wb)
    outs = []
    for i, (x, z, b, t) in enumerate(zip(xs, l2, blk, "eng")):
        f = hidden_fn(z @ W[f"ff_{t}_W1"].T + W[f"ff_{t}_b1"]) @ W[f"ff_{t}_W2"].T + W[f"ff_{t}_b2"]
        outs.append(x + b + (f if masks is None else masks[i] * f))
    return outs


def _core_leaves(p, dtype=torch.float64):
    T = lambda v: torch.tensor(v, dtype=dtype, requires_grad=True)
    return {k: T(v) for k, v in p.items() if isinstance(v, np.ndarray)}, {k: T(p["block"][k]) for k in ("We", "be", "Wn", "bn", "Wg", "bg")}


def core_case(graph, dims, R=1, flags=0, eps_mode=0, seed=0, flag_names=(), dropout=None, shift=0.0):
    def setup(gn, a):
        L, lib = _L(gn), _L(gn).load()
        fl = flags
        for n in flag_names:
            fl |= getattr(L, "FLAG_" + n)
        g, csc = graph(gn)
        rng = np.random.default_rng(2000 + seed)
        p = O.make_core_params(rng, dims, eps_mode=eps_mode)
        _decl_core(a, p)
        x = list(U.packed_inputs(rng, R, g.n_edges, g.n_nodes, g.n_graphs, dims))
        x[0] = (x[0] * 1.5 + shift).astype(np.float32)  # statistics that matter: a mean away from zero
        ins = [_decl(a, n, v) for n, v in zip(("ef", "nf", "gf"), x)]
        outs = _decl_outputs(a, "", R, _rows(g), dims)
        drop = None if dropout is None else L.Dropout(dropout, 0, 0x1234_5678_9ABC)
        if drop is None:
            w = a.workspace("ws", lambda: lib.gnx_core_workspace_bytes(g._h, C.byref(_core_params(gn, a, p)), R))
        else:
            assert R == 1
            w = a.workspace("ws", lambda: lib.gnx_core_train_workspace_bytes(g._h, C.byref(_core_params(gn, a, p)), R))

        def run(a):
            assert a.nbytes(w) > 0, lib.gnx_last_error()
            cp = _core_params(gn, a, p)
            P = a.ptr
            if drop is None:
                return lib.gnx_core_forward(g._h, C.byref(cp), *map(P, ins), R, *map(P, outs), P(w), a.nbytes(w), fl, _stream())
            return lib.gnx_core_forward_train(g._h, C.byref(cp), C.byref(drop), *map(P, ins), R, *map(P, outs), P(w), a.nbytes(w), fl, _stream())

        memo = {}

        def verify(a, what):
            if "ref" not in memo:
                memo["ref"] = O.core_forward_sparse(p, csc, *x, return_scale=True)
            ref, scale = memo["ref"]
            if drop is None:
                return _check_outputs(a, outs, ref, scale, what)
            # training mode: float64 restatement with the call's own masks, at the bound of tests/test_gpu_dropout.py
            if "train" not in memo:
                masks = []
                for t, (T, d) in enumerate(zip(_rows(g), dims)):
                    m = torch.empty((T, d), dtype=F32, device="cuda")
                    assert lib.gnx_dropout_mask(C.byref(drop), t, m.numel(), m.data_ptr(), _stream()) == 0, lib.gnx_last_error()
                    masks.append(m.double().cpu())
                W, Wb = _core_leaves(p)
                xs = [torch.tensor(v[0], dtype=torch.float64) for v in x]
                with torch.no_grad():
                    memo["train"] = [o.numpy() for o in _torch_core(p, csc, xs, W, Wb, torch.relu, masks)]
            for n, r, So in zip(outs, memo["train"], scale):
                err = np.abs(a.numpy(n)[0].astype(np.float64) - r)
                bound = 1e-5 * (1.0 + 2.0 / (1.0 - dropout)) * np.asarray(So[0], dtype=np.float64) + 1e-30
                assert np.isfinite(err).all() and float((err / bound).max()) <= 1.0, f"{what} {n}: worst ratio {float((err / bound).max()):.3f}"
        return run, verify
    return setup


def _grad_close(got, ref, what, bar):
    """tests/test_gpu_backward.py's `close`: max error against bar . max(1, max|ref|)"""
    ref = ref.detach().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.size == 0:
        return
    scale = max(1.0, float(np.abs(ref).max()))
    err = np.abs(got - ref)
    assert np.isfinite(got).all() and float(err.max()) <= bar * scale, f"{what}: max err {float(err.max()):.3e} (scale {scale:.3g})"


def _decl_dense_grad(a, name, W, b):
    """gradient outputs of one Dense: weight in the (out x in) column-major layout of the weights = an (in, out) array, and bias — a width-0
    function has carves of no bytes"""
    a.output(name + ".dW", tuple(reversed(np.asarray(W).shape)))
    a.output(name + ".db", np.asarray(b).shape)


def _dense_grad(gn, a, name):
    return _L(gn).DenseGrad(a.ptr(name + ".dW"), a.ptr(name + ".db"))


def block_backward_case(graph, in_dims, out_dims, act=(2, 3, 0), seed=0, R=1):
    """gnx_block_backward: forward inputs, forward outputs (the float64 forward rounded to fp32) and cotangents are inputs; d_ef / d_nf / d_gf
    and all six parameter gradients are outputs.  The torch restatement runs replica by replica on the same parameter leaves (R > 1: one graph,
    the parameter gradients are sums over the replicas)."""
    def setup(gn, a):
        lib = _L(gn).load()
        g, csc = graph(gn)
        rng = np.random.default_rng(3000 + seed)
        p = O.make_block_params(rng, in_dims, out_dims, act=act)
        _decl_block(a, p)
        x = U.packed_inputs(rng, R, g.n_edges, g.n_nodes, g.n_graphs, in_dims)
        W = {k: torch.tensor(p[k], dtype=torch.float64, requires_grad=True) for k in ("We", "be", "Wn", "bn", "Wg", "bg")}
        xs = [[None if v is None else torch.tensor(v[r], dtype=torch.float64, requires_grad=True) for v in x] for r in range(R)]
        outs_r = [_torch_block(p, csc, *xs[r], W) for r in range(R)]
        cot = [[rng.standard_normal(tuple(o.shape)) for o in outs_r[r]] for r in range(R)]
        sum((o * torch.from_numpy(c)).sum() for r in range(R) for o, c in zip(outs_r[r], cot[r]) if o.shape[1] > 0).backward()
        stack = lambda per_rep, k: np.stack([np.asarray(per_rep[r][k].detach() if isinstance(per_rep[r][k], torch.Tensor) else per_rep[r][k]) for r in range(R)]).astype(np.float32)
        ins = [_decl(a, n, v) for n, v in zip(("ef", "nf", "gf"), x)]
        fw = [_decl(a, n, stack(outs_r, k)) if d > 0 else None for k, (n, d) in enumerate(zip(("ef_out", "nf_out", "gf_out"), out_dims))]
        gs = [_decl(a, n, stack(cot, k)) if d > 0 else None for k, (n, d) in enumerate(zip(("g_ef_out", "g_nf_out", "g_gf_out"), out_dims))]
        dx = [a.output(n, v.shape) if v is not None else None for n, v in zip(("d_ef", "d_nf", "d_gf"), x)]
        for fn, w, b in (("edgefn", "We", "be"), ("nodefn", "Wn", "bn"), ("graphfn", "Wg", "bg")):
            _decl_dense_grad(a, f"grad.{fn}", p[w], p[b])
        ws = a.workspace("ws", lambda: lib.gnx_block_backward_workspace_bytes(g._h, C.byref(_block_params(gn, a, p)), R))

        def run(a):
            P = a.ptr
            gr = _L(gn).BlockGrads(*[_dense_grad(gn, a, f"grad.{fn}") for fn in ("edgefn", "nodefn", "graphfn")])
            return lib.gnx_block_backward(g._h, C.byref(_block_params(gn, a, p)), *map(P, ins), *map(P, fw), *map(P, gs), R, *map(P, dx), C.byref(gr),
                                          P(ws), a.nbytes(ws), _stream())

        def verify(a, what):
            for k, n in enumerate(dx):
                if n is not None:
                    for r in range(R):
                        _grad_close(a.numpy(n)[r], xs[r][k].grad, f"{what} {n}[{r}]", 2e-4)
            for fn, w, b in (("edgefn", "We", "be"), ("nodefn", "Wn", "bn"), ("graphfn", "Wg", "bg")):
                _grad_close(a.numpy(f"grad.{fn}.dW").T, W[w].grad, f"{what} dW {fn}", 2e-4)
                _grad_close(a.numpy(f"grad.{fn}.db"), W[b].grad, f"{what} db {fn}", 2e-4)
        return run, verify
    return setup


def core_backward_case(graph, dims, hidden_act="tanh", eps_mode=0, seed=0, dropout=None):
    """gnx_core_backward / gnx_core_backward_train: every one of the 30 parameter gradients and the three input gradients is an output carve"""
    def setup(gn, a):
        L, lib = _L(gn), _L(gn).load()
        g, csc = graph(gn)
        rng = np.random.default_rng(4000 + seed)
        p = O.make_core_params(rng, dims, eps_mode=eps_mode)
        _decl_core(a, p)
        x = U.packed_inputs(rng, 1, g.n_edges, g.n_nodes, g.n_graphs, dims)
        drop = None if dropout is None else L.Dropout(dropout, 0, 0xC0FFEE)
        masks = None
        if drop is not None:
            masks = []
            for t, (T, d) in enumerate(zip(_rows(g), dims)):
                m = torch.empty((T, d), dtype=F32, device="cuda")
                assert lib.gnx_dropout_mask(C.byref(drop), t, m.numel(), m.data_ptr(), _stream()) == 0, lib.gnx_last_error()
                masks.append(m.double().cpu())
        W, Wb = _core_leaves(p)
        xs = [torch.tensor(v[0], dtype=torch.float64, requires_grad=True) for v in x]
        hidden_fn = {"tanh": torch.tanh, "gelu": ACT[4]}[hidden_act]
        outs_r = _torch_core(p, csc, xs, W, Wb, hidden_fn, masks)
        cot = [rng.standard_normal(tuple(o.shape)) for o in outs_r]
        sum((o * torch.from_numpy(c)).sum() for o, c in zip(outs_r, cot)).backward()
        ins = [_decl(a, n, v) for n, v in zip(("ef", "nf", "gf"), x)]
        gs = [_decl(a, n, c.astype(np.float32)[None]) for n, c in zip(("g_ef_out", "g_nf_out", "g_gf_out"), cot)]
        dx = [a.output(n, v.shape) for n, v in zip(("d_ef", "d_nf", "d_gf"), x)]
        pb = p["block"]
        for fn, w, b in (("edgefn", "We", "be"), ("nodefn", "Wn", "bn"), ("graphfn", "Wg", "bg")):
            _decl_dense_grad(a, f"grad.{fn}", pb[w], pb[b])
        for t in "eng":
            for ln in ("ln1", "ln2"):
                a.output(f"grad.{ln}_{t}.gamma", p[f"{ln}_{t}_gamma"].shape)
                a.output(f"grad.{ln}_{t}.beta", p[f"{ln}_{t}_beta"].shape)
            _decl_dense_grad(a, f"grad.ff_{t}.fc1", p[f"ff_{t}_W1"], p[f"ff_{t}_b1"])
            _decl_dense_grad(a, f"grad.ff_{t}.fc2", p[f"ff_{t}_W2"], p[f"ff_{t}_b2"])
        act_code = L.ACT[hidden_act]
        ws = a.workspace("ws", lambda: lib.gnx_core_backward_workspace_bytes(g._h, C.byref(_core_params(gn, a, p, act_code)), 1))

        def run(a):
            P = a.ptr
            assert a.nbytes(ws) > 0, lib.gnx_last_error()
            gr = L.CoreGrads()
            gr.block = L.BlockGrads(*[_dense_grad(gn, a, f"grad.{fn}") for fn in ("edgefn", "nodefn", "graphfn")])
            for i, t in enumerate("eng"):
                gr.ln1[i].gamma, gr.ln1[i].beta = P(f"grad.ln1_{t}.gamma"), P(f"grad.ln1_{t}.beta")
                gr.ln2[i].gamma, gr.ln2[i].beta = P(f"grad.ln2_{t}.gamma"), P(f"grad.ln2_{t}.beta")
                gr.ff[i].fc1, gr.ff[i].fc2 = _dense_grad(gn, a, f"grad.ff_{t}.fc1"), _dense_grad(gn, a, f"grad.ff_{t}.fc2")
            cp = _core_params(gn, a, p, act_code)
            if drop is None:
                return lib.gnx_core_backward(g._h, C.byref(cp), *map(P, ins), *map(P, gs), 1, *map(P, dx), C.byref(gr), P(ws), a.nbytes(ws), _stream())
            return lib.gnx_core_backward_train(g._h, C.byref(cp), C.byref(drop), *map(P, ins), *map(P, gs), 1, *map(P, dx), C.byref(gr), P(ws),
                                               a.nbytes(ws), _stream())

        def verify(a, what):
            for n, t in zip(dx, xs):
                _grad_close(a.numpy(n)[0], t.grad, f"{what} {n}", 1e-3)
            for fn, w, b in (("edgefn", "We", "be"), ("nodefn", "Wn", "bn"), ("graphfn", "Wg", "bg")):
                _grad_close(a.numpy(f"grad.{fn}.dW").T, Wb[w].grad, f"{what} dW {fn}", 1e-3)
                _grad_close(a.numpy(f"grad.{fn}.db"), Wb[b].grad, f"{what} db {fn}", 1e-3)
            for t in "eng":
                for ln in ("ln1", "ln2"):
                    for k in ("gamma", "beta"):
                        _grad_close(a.numpy(f"grad.{ln}_{t}.{k}"), W[f"{ln}_{t}_{k}"].grad, f"{what} {ln}_{t}.{k}", 1e-3)
                for fc, wk, bk in (("fc1", "W1", "b1"), ("fc2", "W2", "b2")):
                    _grad_close(a.numpy(f"grad.ff_{t}.{fc}.dW").T, W[f"ff_{t}_{wk}"].grad, f"{what} ff_{t}.{fc} dW", 1e-3)
                    _grad_close(a.numpy(f"grad.ff_{t}.{fc}.db"), W[f"ff_{t}_{bk}"].grad, f"{what} ff_{t}.{fc} db", 1e-3)
        return run, verify
    return setup


# ---------------------------------------------------------------------------------------------------------------------------------------
# GNBlock with Chain update functions: forward and backward
# ---------------------------------------------------------------------------------------------------------------------------------------
def _decl_chains(a, p):
    for name in ("edge", "node", "graph"):
        for i, (w, b, c) in enumerate(p[name]):
            if isinstance(w, str):  # ("layernorm", gamma, beta)
                a.input(f"chain.{name}{i}.W", b)
                a.input(f"chain.{name}{i}.b", c)
            else:
                _decl_dense(a, f"chain.{name}{i}", w, b)


def _chain_params(gn, a, p, keep):
    L = _L(gn)
    q = L.ChainBlockParams()
    q.de, q.dn, q.dg = p["in_dims"]
    for name, field in (("edge", "edgefn"), ("node", "nodefn"), ("graph", "graphfn")):
        layers = p[name]
        arr = (L.Dense * max(len(layers), 1))()
        wid = (C.c_int32 * max(len(layers), 1))()
        for i, (w, b, c) in enumerate(layers):
            ln = isinstance(w, str)
            kind = 0 if not ln else (L.LAYER_LAYERNORM | L.LAYER_LN_SQRT_EPS if O.ln_eps_mode(w) == 1 else L.LAYER_LAYERNORM)
            arr[i] = _dense(gn, a, f"chain.{name}{i}", 0 if ln else c, kind)
            wid[i] = len(b) if ln else w.shape[0]
        keep += [arr, wid]
        ch = getattr(q, field)
        ch.layers, ch.widths, ch.n_layers = arr, wid, len(layers)
    return q


def _chain_out_widths(p):
    de, dn, dg = p["in_dims"]
    out, k = [], de + 2 * dn + dg
    for name in ("edge", "node", "graph"):
        if name == "node":
            k = out[0] + dn + dg
        elif name == "graph":
            k = out[0] + out[1] + dg
        for w, b, c in p[name]:
            k = k if isinstance(w, str) else w.shape[0]
        out.append(k if p[name] else 0)
    return out


def chain_case(graph, in_dims, ew, nw, gw, R=1, seed=0, backward=False, acts=(2, 3, 2)):
    def setup(gn, a):
        L, lib = _L(gn), _L(gn).load()
        g, csc = graph(gn)
        rng = np.random.default_rng(5000 + seed)
        p = O.make_chain_block_params(rng, in_dims, ew, nw, gw, acts=acts) if backward else O.make_chain_block_params(rng, in_dims, ew, nw, gw)
        _decl_chains(a, p)
        x = U.packed_inputs(rng, R, g.n_edges, g.n_nodes, g.n_graphs, in_dims)
        ins = [_decl(a, n, v) for n, v in zip(("ef", "nf", "gf"), x)]
        keep = []
        if not backward:
            outs = _decl_outputs(a, "", R, _rows(g), _chain_out_widths(p))
            ws = a.workspace("ws", lambda: lib.gnx_chain_block_workspace_bytes(g._h, C.byref(_chain_params(gn, a, p, keep)), R))

            def run(a):
                assert a.nbytes(ws) > 0, lib.gnx_last_error()
                P = a.ptr
                return lib.gnx_chain_block_forward(g._h, C.byref(_chain_params(gn, a, p, keep)), *map(P, ins), R, *map(P, outs), P(ws), a.nbytes(ws), 0, _stream())

            memo = []

            def verify(a, what):
                if not memo:
                    memo.append(O.chain_block_forward_sparse(p, csc, *x, return_scale=True))
                _check_outputs(a, outs, *memo[0], what)
            return run, verify
        assert R == 1
        T = lambda v: torch.tensor(v, dtype=torch.float64, requires_grad=True)
        W = {name: [(w, T(b), T(c)) if isinstance(w, str) else (T(w), T(b), c) for w, b, c in p[name]] for name in ("edge", "node", "graph")}
        xs = [None if v is None else T(v[0]) for v in x]
        outs_r, _ = _torch_chain_block(csc, *xs, W)
        cot = [None if o is None else rng.standard_normal(tuple(o.shape)) for o in outs_r]
        sum((o * torch.from_numpy(c)).sum() for o, c in zip(outs_r, cot) if o is not None).backward()
        gs = [None if c is None else _decl(a, n, c.astype(np.float32)[None]) for n, c in zip(("g_ef_out", "g_nf_out", "g_gf_out"), cot)]
        dx = [a.output(n, v.shape) if v is not None else None for n, v in zip(("d_ef", "d_nf", "d_gf"), x)]
        for name in ("edge", "node", "graph"):
            for i, (w, b, c) in enumerate(p[name]):
                if isinstance(w, str):
                    a.output(f"grad.{name}{i}.dW", b.shape)
                    a.output(f"grad.{name}{i}.db", c.shape)
                else:
                    _decl_dense_grad(a, f"grad.{name}{i}", w, b)
        ws = a.workspace("ws", lambda: lib.gnx_chain_block_backward_workspace_bytes(g._h, C.byref(_chain_params(gn, a, p, keep)), 1))

        def run(a):
            assert a.nbytes(ws) > 0, lib.gnx_last_error()
            P = a.ptr
            arrays = []
            for name in ("edge", "node", "graph"):
                arr = (L.DenseGrad * max(len(p[name]), 1))()
                for i in range(len(p[name])):
                    arr[i] = _dense_grad(gn, a, f"grad.{name}{i}")
                arrays.append(arr)
            gr = L.ChainBlockGrads(*[C.cast(x_, C.POINTER(L.DenseGrad)) for x_ in arrays])
            return lib.gnx_chain_block_backward(g._h, C.byref(_chain_params(gn, a, p, keep)), *map(P, ins), *map(P, gs), 1, *map(P, dx), C.byref(gr),
                                                P(ws), a.nbytes(ws), _stream())

        def verify(a, what):
            for n, t in zip(dx, xs):
                if n is not None:
                    _grad_close(a.numpy(n)[0], t.grad, f"{what} {n}", 1e-3)
            for name in ("edge", "node", "graph"):
                for i, (w, b, c) in enumerate(W[name]):
                    if isinstance(w, str):
                        _grad_close(a.numpy(f"grad.{name}{i}.dW"), b.grad, f"{what} {name}{i} gamma", 1e-3)
                        _grad_close(a.numpy(f"grad.{name}{i}.db"), c.grad, f"{what} {name}{i} beta", 1e-3)
                    else:
                        _grad_close(a.numpy(f"grad.{name}{i}.dW").T, w.grad, f"{what} {name}{i} dW", 1e-3)
                        _grad_close(a.numpy(f"grad.{name}{i}.db"), b.grad, f"{what} {name}{i} db", 1e-3)
        return run, verify
    return setup


# ---------------------------------------------------------------------------------------------------------------------------------------
# the small entry points
# ---------------------------------------------------------------------------------------------------------------------------------------
def xent_case(d, cols, seed=0):
    def setup(gn, a):
        lib = _L(gn).load()
        rng = np.random.default_rng(6000 + seed)
        logits = rng.standard_normal((cols, d)).astype(np.float32) * 3
        tgt = np.eye(d, dtype=np.float32)[rng.integers(0, d, cols)]
        up = np.array([0.75], dtype=np.float32)
        a.input("logits", logits); a.input("targets", tgt); a.input("upstream", up)
        a.output("loss", (1,))
        a.output("d_logits", (cols, d))
        a.workspace("ws", int(lib.gnx_xent_workspace_bytes(cols)))

        def run(a):
            P = a.ptr
            rc = lib.gnx_logit_cross_entropy(P("logits"), P("targets"), d, cols, P("loss"), P("ws"), a.nbytes("ws"), _stream())
            return rc or lib.gnx_logit_cross_entropy_backward(P("logits"), P("targets"), d, cols, P("upstream"), P("d_logits"), _stream())

        def verify(a, what):
            x = logits.astype(np.float64)
            lse = np.log(np.exp(x - x.max(1, keepdims=True)).sum(1, keepdims=True)) + x.max(1, keepdims=True)
            ref = float(np.mean(-(tgt * (x - lse)).sum(1)))
            got = float(a.numpy("loss")[0])
            assert abs(got - ref) <= 1e-5 * max(1.0, abs(ref)), (what, got, ref)      # tests/test_gpu_block.py::test_readout_logitcrossentropy
            dref = 0.75 * (tgt.sum(1, keepdims=True) * np.exp(x - lse) - tgt) / cols
            np.testing.assert_allclose(a.numpy("d_logits"), dref, rtol=1e-4, atol=1e-6)  # tests/test_gpu_backward.py::test_readout_loss_is_differentiable
        return run, verify
    return setup


def _slots(g, csc):
    """(slot of every edge, slot of every node) in the padded [B][PN^2] / [B][PN] grids (pad.jl:30: column-major i + PN j)"""
    colptr, rowval, node_off, edge_off = (np.asarray(v) for v in csc)
    PN = g.node_block_size
    dst = np.repeat(np.arange(g.n_nodes), np.diff(colptr))
    ng = np.repeat(np.arange(g.n_graphs), np.diff(node_off))
    eg = np.repeat(np.arange(g.n_graphs), np.diff(edge_off))
    nslot = np.arange(g.n_nodes) - node_off[ng]
    eslot = (rowval - node_off[eg]) + PN * (dst - node_off[eg])
    return (eg, eslot), (ng, nslot)


def pad_case(graph, d, R=1, seed=0):
    """gnx_pad_features + gnx_unpad_features, edges and nodes: packed -> padded (pads written as zeros) -> packed"""
    def setup(gn, a):
        lib = _L(gn).load()
        g, csc = graph(gn)
        rng = np.random.default_rng(7000 + seed)
        ef, nf, _ = U.packed_inputs(rng, R, g.n_edges, g.n_nodes, g.n_graphs, (d, d, 0))
        B = R if g.n_graphs == 1 else g.n_graphs
        a.input("ef", ef); a.input("nf", nf)
        a.output("ef_pad", (B, g.edge_block_size, d)); a.output("nf_pad", (B, g.node_block_size, d))
        a.output("ef_back", ef.shape); a.output("nf_back", nf.shape)

        def run(a):
            P = a.ptr
            for kind, n in ((0, "ef"), (1, "nf")):
                rc = lib.gnx_pad_features(g._h, kind, P(n), d, R, P(n + "_pad"), _stream())
                rc = rc or lib.gnx_unpad_features(g._h, kind, P(n + "_pad"), d, R, P(n + "_back"), _stream())
                if rc:
                    return rc
            return 0

        def verify(a, what):
            for (b, slot), n, x in zip(_slots(g, csc), ("ef", "nf"), (ef, nf)):
                ref = np.zeros(a.by_name[n + "_pad"].shape, dtype=np.float32)
                if g.n_graphs == 1:
                    ref[:, slot, :] = x
                else:
                    ref[b, slot, :] = x[0]
                assert np.array_equal(a.numpy(n + "_pad"), ref), f"{what}: {n} padded"
                assert np.array_equal(a.numpy(n + "_back"), x), f"{what}: {n} round trip"
        return run, verify
    return setup


def collapse_case(graph, d, R=1, seed=0):
    """gnx_collapse_edges + gnx_collapse_padded against a plain restatement: (P[i->j] + P[j->i]) / 2 over the zero-padded edge grid"""
    def setup(gn, a):
        lib = _L(gn).load()
        g, csc = graph(gn)
        rng = np.random.default_rng(8000 + seed)
        ef, _, _ = U.packed_inputs(rng, R, g.n_edges, g.n_nodes, g.n_graphs, (d, 0, 0))
        off = np.zeros(g.n_graphs + 1, dtype=np.int64)
        assert lib.gnx_collapse_offsets(g._h, off.ctypes.data_as(C.POINTER(C.c_int64))) == 0
        PN = g.node_block_size
        B = R if g.n_graphs == 1 else g.n_graphs
        a.input("ef", ef)
        a.output("flat", (R, int(off[-1]), d))
        a.output("padded", (B, PN * (PN + 1) // 2, d))

        def run(a):
            P = a.ptr
            return (lib.gnx_collapse_edges(g._h, P("ef"), d, R, P("flat"), _stream()) or
                    lib.gnx_collapse_padded(g._h, P("ef"), d, R, P("padded"), _stream()))

        def verify(a, what):
            (eg, eslot), _ = _slots(g, csc)
            grid = np.zeros((B, PN * PN, d), dtype=np.float64)
            if g.n_graphs == 1:
                grid[:, eslot, :] = ef
            else:
                grid[eg, eslot, :] = ef[0]
            grid = grid.reshape(B, PN, PN, d)  # [b][j][i]: slot = i + PN j
            sym = (grid + grid.transpose(0, 2, 1, 3)) / 2
            jj, ii = np.meshgrid(np.arange(PN), np.arange(PN), indexing="ij")
            low = (ii >= jj).reshape(-1)       # coordinates (i, j), i >= j, in column-major order = increasing slot
            ref_pad = sym.reshape(B, PN * PN, d)[:, low, :]
            np.testing.assert_allclose(a.numpy("padded"), ref_pad, rtol=1e-6, atol=1e-7, err_msg=what)
            i, j = eslot % PN, eslot // PN
            keep = i >= j                       # the real edges of the lower triangle, in edge order
            full = sym.reshape(B, PN * PN, d)
            ref_flat = full[:, eslot[keep], :] if g.n_graphs == 1 else full[eg[keep], eslot[keep], :][None]
            np.testing.assert_allclose(a.numpy("flat"), ref_flat, rtol=1e-6, atol=1e-7, err_msg=what)
        return run, verify
    return setup


def fn_input_case(graph, dims, R=1, seed=0):
    """gnx_fn_input kinds 0, 1, 2"""
    def setup(gn, a):
        lib = _L(gn).load()
        g, csc = graph(gn)
        de, dn, dg = dims
        rng = np.random.default_rng(9000 + seed)
        x = U.packed_inputs(rng, R, g.n_edges, g.n_nodes, g.n_graphs, dims)
        ins = [_decl(a, n, v) for n, v in zip(("ef", "nf", "gf"), x)]
        K = (de + 2 * dn + dg, de + dn + dg, de + dn + dg)
        outs = [a.output(f"X{k}", (R, T, K[k])) for k, T in enumerate(_rows(g))]

        def run(a):
            P = a.ptr
            for k in range(3):
                rc = lib.gnx_fn_input(g._h, k, P(ins[0]), de, P(ins[1]), dn, P(ins[2]), dg, R, P(outs[k]), _stream())
                if rc:
                    return rc
            return 0

        def verify(a, what):
            colptr, rowval, node_off, edge_off = (np.asarray(v) for v in csc)
            dst = np.repeat(np.arange(g.n_nodes), np.diff(colptr))
            ng = np.repeat(np.arange(g.n_graphs), np.diff(node_off))
            eg = np.repeat(np.arange(g.n_graphs), np.diff(edge_off))
            ef, nf, gf = (None if v is None else v.astype(np.float64) for v in x)
            cat = lambda parts: np.concatenate([q for q in parts if q is not None], axis=2)

            def seg(v, idx, n):
                out = np.zeros((R, n, v.shape[2]))
                np.add.at(out, (slice(None), idx), v)
                return out
            refs = [cat([ef, None if nf is None else nf[:, rowval], None if nf is None else nf[:, dst], None if gf is None else gf[:, eg]]),
                    cat([None if ef is None else seg(ef, dst, g.n_nodes), nf, None if gf is None else gf[:, ng]]),
                    cat([None if ef is None else seg(ef, eg, g.n_graphs), None if nf is None else seg(nf, ng, g.n_graphs), gf])]
            for n, r in zip(outs, refs):  # sums of up to a few hundred values in [0, 1): the bars of test_exported_fn_input_building_blocks
                np.testing.assert_allclose(a.numpy(n), r, rtol=1e-5, atol=1e-5, err_msg=f"{what} {n}")
        return run, verify
    return setup


def row_stats_case(rows, d, eps_mode, seed=0):
    def setup(gn, a):
        lib = _L(gn).load()
        rng = np.random.default_rng(9500 + seed)
        x = (rng.random((rows, d), dtype=np.float32) * 3 + 2).astype(np.float32)
        a.input("x", x)
        a.output("stats", (rows, 2))

        def run(a):
            return lib.gnx_row_stats(a.ptr("x"), rows, d, 1e-5, eps_mode, a.ptr("stats"), _stream())

        def verify(a, what):
            x64 = x.astype(np.float64)
            mu, var = x64.mean(1), x64.var(1)
            inv = 1 / (np.sqrt(var) + 1e-5) if eps_mode == 0 else 1 / np.sqrt(var + 1e-5)
            got = a.numpy("stats")
            np.testing.assert_allclose(got[:, 0], mu, rtol=1e-5, err_msg=what)
            np.testing.assert_allclose(got[:, 1], inv, rtol=1e-4, err_msg=what)  # 1 / sigma from an fp32 variance: a few 1e-6 relative, with margin
        return run, verify
    return setup


def dropout_mask_case(n, p, entity):
    def setup(gn, a):
        L, lib = _L(gn), _L(gn).load()
        drop = L.Dropout(p, 0, 987654321)
        a.output("mask", (n,))

        def run(a):
            return lib.gnx_dropout_mask(C.byref(drop), entity, n, a.ptr("mask"), _stream())

        def verify(a, what):
            m = a.numpy("mask")
            keep = m != 0
            assert np.all(m[keep] == np.float32(1.0) / (np.float32(1.0) - np.float32(p))), what  # Flux._dropout_kernel: 1 / q
            assert abs(keep.mean() - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n), (what, keep.mean())
        return run, verify
    return setup


# ---------------------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------------------
README = ((10, 5, 0), (3, 4, 5))
ODD = ((7, 3, 3), (5, 1, 3))       # run-time specialised, every width odd: R.T.d.4 is no multiple of 16 anywhere
EVEN = ((6, 4, 2), (4, 2, 2))      # run-time specialised, dword-pair rows
WIDE = ((128, 64, 32), (128, 64, 32))
BIG1 = g_er(1999, 20011)           # one graph: the two-launch narrow form
WIDE_G = g_hub(601, 4400, 300)     # > 4096 edges, a hub over several tiles, isolated nodes
CORE_W = (128, 64, 32)

CASES = {
    # ---- gnx_block_forward: the fused narrow kernel ----
    "block/readme/one-graph/R1": block_case(BIG1, *README),
    "block/readme/one-graph/R3": block_case(g_hub(1001, 7001, 333), *README, R=3, seed=1),
    "block/readme/small-graphs(pack)": block_case(g_small(), *README, seed=2),
    "block/readme/small-graphs/NO_PACK": block_case(g_small(), *README, seed=3, flag_names=("NO_PACK",)),
    "block/readme+gf/no-edges": block_case(g_no_edges, (10, 5, 3), (3, 4, 5), seed=4),
    "block/jit-odd/one-graph/R3": block_case(g_hub(997, 6007, 200), *ODD, R=3, seed=5),
    "block/jit-odd/small-graphs": block_case(g_small(seed=6), *ODD, seed=6),
    "block/jit-even/medium": block_case(g_medium(), *EVEN, seed=7),
    "block/readme/FORCE_GENERIC": block_case(g_medium(), *README, seed=8, flag_names=("FORCE_GENERIC",)),
    "block/odd/FORCE_GENERIC/R3": block_case(g_hub(333, 2001, 150), *ODD, R=3, seed=9, flag_names=("FORCE_GENERIC",)),
    "block/odd/NO_JIT": block_case(g_medium(), *ODD, seed=10, flag_names=("NO_JIT",)),
    "block/jit(5,6,7)/small-graphs": block_case(g_small(seed=11), (5, 6, 7), (7, 6, 5), seed=11),
    "block/mid-widths(40,36,8)": block_case(g_er(3001, 20003), (40, 36, 8), (36, 40, 8), seed=12),
    # ---- `nothing` combinations that change a buffer's presence ----
    "block/nothing/ef-only": block_case(g_small(seed=13), (3, 0, 0), (2, 3, 0), seed=13),
    "block/nothing/nf-only": block_case(g_small(seed=14), (0, 2, 0), (3, 4, 5), seed=14),
    "block/nothing/gf-only": block_case(g_small(seed=15), (0, 0, 4), (2, 0, 3), seed=15),
    "block/nothing/no-ef-out": block_case(g_small(seed=16), (3, 2, 4), (0, 2, 2), seed=16),
    "block/nothing/no-nf-out": block_case(g_medium(seed=17), (3, 2, 0), (2, 0, 3), seed=17),
    "block/nothing/no-gf-out/one-graph": block_case(BIG1, (10, 5, 0), (3, 4, 0), seed=18),
    "block/nothing/nf+gf/generic": block_case(g_small(seed=19), (0, 2, 4), (3, 4, 5), seed=19, flag_names=("FORCE_GENERIC",)),
    # ---- wide: matrix cores ----
    "block/wide/default": block_case(WIDE_G, *WIDE, seed=20, act=(1, 1, 0)),
    "block/wide/R3/4096-edges": block_case(g_er(601, 4096), *WIDE, R=3, seed=21, act=(1, 1, 0)),
    "block/wide/4095-edges": block_case(g_er(601, 4095), *WIDE, seed=22, act=(1, 1, 0)),
    "block/wide/4097-edges/4099-nodes": block_case(g_er(4099, 4097), *WIDE, seed=23, act=(1, 1, 0)),
    "block/wide/FP32_MFMA": block_case(WIDE_G, *WIDE, seed=24, act=(1, 1, 0), flags=0x60),
    "block/wide/PROJ_FP32": block_case(g_er(4099, 12007), *WIDE, seed=25, act=(1, 1, 0), flag_names=("PROJ_FP32",)),
    "block/wide/EDGE_N": block_case(WIDE_G, *WIDE, seed=26, act=(1, 1, 0), flag_names=("EDGE_N",)),
    "block/wide/NO_MFMA": block_case(g_hub(301, 2001, 150), *WIDE, seed=27, act=(1, 1, 0), flag_names=("NO_MFMA",)),
    "block/wide/128=>narrow": block_case(WIDE_G, (128, 64, 32), (20, 64, 32), seed=28, act=(1, 1, 0)),
    "block/wide/128=>narrow/EDGE_NARROW_FP32": block_case(WIDE_G, (128, 64, 32), (20, 64, 32), seed=29, act=(1, 1, 0), flag_names=("EDGE_NARROW_FP32",)),
    "block/wide/128=>(3,4,5)": block_case(WIDE_G, (128, 64, 32), (3, 4, 5), seed=54, act=(1, 1, 0)),
    "block/wide/128=>(3,4,5)/R3/EDGE_NARROW_FP32": block_case(g_er(601, 4099), (128, 64, 32), (3, 4, 5), R=3, seed=55, act=(1, 1, 0), flag_names=("EDGE_NARROW_FP32",)),
    "block/wide/128=>(3,4,5)/4095-edges": block_case(g_er(601, 4095), (128, 64, 32), (3, 4, 5), seed=56, act=(1, 1, 0)),
    "block/encoder(10,5,0)=>(128,64,32)": block_case(BIG1, (10, 5, 0), (128, 64, 32), seed=57, act=(1, 1, 0)),
    "block/encoder(10,5,3)=>(128,64,32)/R3": block_case(g_hub(1001, 7001, 333), (10, 5, 3), (128, 64, 32), R=3, seed=58, act=(1, 1, 0)),
    "block/wide/small-graphs": block_case(g_medium(seed=30), *WIDE, seed=30, act=(1, 1, 0)),
    # every replica stride (4097 . 33, 601 . 17, 4097 . 40, ... floats) is odd or 2 mod 4: replicas 1 and 2 start 4-byte aligned only, inside
    # an aligned buffer (tests/test_gpu_alignment.py)
    "block/wide-odd(33,17,5)=>(40,35,7)/R3": block_case(g_er(601, 4097), (33, 17, 5), (40, 35, 7), R=3, seed=59, act=(1, 1, 0)),
    # ---- deferred, chained, steps ----
    "block/deferred/readme": block_case(BIG1, *README, seed=31, entry="deferred"),
    "block/deferred/wide": block_case(WIDE_G, *WIDE, seed=32, act=(1, 1, 0), entry="deferred"),
    "block/deferred/generic": block_case(g_medium(seed=33), (5, 6, 7), (7, 6, 5), seed=33, entry="deferred"),
    "block/chained/one-graph": block_case(BIG1, *README, seed=34, entry="chained", n_steps=3),
    "block/chained/many-graphs": block_case(lambda gn: _from_csc(gn, [U.er_csc(np.random.default_rng(35 + i), n, 12 * n + 1) for i, n in enumerate((301, 457, 699))]),
                                            (10, 5, 3), (3, 4, 5), seed=35, entry="chained", n_steps=3),
    "block/chained/small-graphs": block_case(g_small(seed=36), *README, seed=36, entry="chained", n_steps=3),
    "block/steps/one-graph": block_case(BIG1, *README, seed=37, entry="steps", n_steps=4),
    "block/steps/one-graph/NO_FORK": block_case(BIG1, *README, seed=38, entry="steps", n_steps=4, flag_names=("NO_FORK",)),
    "block/steps/small-graphs": block_case(g_small(seed=39), *README, seed=39, entry="steps", n_steps=3),
    "block/steps/jit-odd/R3": block_case(g_hub(997, 6007, 200), *ODD, R=3, seed=40, entry="steps", n_steps=3),
    "block/steps/mid-widths": block_case(g_er(3001, 20003), (40, 36, 8), (36, 40, 8), seed=41, entry="steps", n_steps=3),
    # ---- bfloat16 features ----
    "bf16/readme/one-graph/R3": block_case(g_hub(1001, 7001, 333), *README, R=3, seed=42, entry="typed", bf16=True),
    "bf16/readme/small-graphs": block_case(g_small(seed=43), *README, seed=43, entry="typed", bf16=True),
    "bf16/jit-odd/medium": block_case(g_medium(seed=44), *ODD, seed=44, entry="typed", bf16=True),
    "bf16/fallback/FORCE_GENERIC/odd/R3": block_case(g_hub(333, 2001, 150), *ODD, R=3, seed=45, entry="typed", bf16=True, flag_names=("FORCE_GENERIC",)),
    "bf16/fallback/NO_JIT": block_case(g_medium(seed=46), *EVEN, seed=46, entry="typed", bf16=True, flag_names=("NO_JIT",)),
    "bf16/fallback/wide": block_case(WIDE_G, *WIDE, seed=47, act=(1, 1, 0), entry="typed", bf16=True),
    "bf16/fallback/nothing": block_case(g_small(seed=48), (0, 3, 0), (3, 0, 5), seed=48, entry="typed", bf16=True, flag_names=("FORCE_GENERIC",)),
    "bf16/typed-f32": block_case(g_medium(seed=49), *README, seed=49, entry="typed"),
    "bf16/steps/readme/one-graph": block_case(BIG1, *README, seed=50, entry="steps_typed", bf16=True, n_steps=4),
    "bf16/steps/jit-odd/small-graphs": block_case(g_small(seed=51), *ODD, seed=51, entry="steps_typed", bf16=True, n_steps=3),
    "bf16/steps/fallback/FORCE_GENERIC": block_case(g_medium(seed=52), *README, seed=52, entry="steps_typed", bf16=True, n_steps=3, flag_names=("FORCE_GENERIC",)),
    "bf16/steps/fallback/wide": block_case(WIDE_G, *WIDE, seed=53, act=(1, 1, 0), entry="steps_typed", bf16=True, n_steps=2),
    # ---- gnx_core_forward: narrow ----
    "core/narrow(10,5,3)/medium": core_case(g_medium(seed=60), (10, 5, 3), seed=60),
    "core/narrow(10,5,3)/R3/hub": core_case(g_hub(1001, 7001, 333), (10, 5, 3), R=3, seed=61),
    "core/narrow(10,5,3)/NO_FFE": core_case(g_medium(seed=62), (10, 5, 3), seed=62, flag_names=("NO_FFE",)),
    "core/narrow(10,5,3)/small-graphs/eps1": core_case(g_small(seed=63), (10, 5, 3), eps_mode=1, seed=63),
    "core/narrow(10,5,3)/post3(>=65536 rows)": core_case(g_er(65539, 70001), (10, 5, 3), seed=64),
    "core/narrow(10,5,3)/post3/NO_FFE": core_case(g_er(65539, 70001), (10, 5, 3), seed=65, flag_names=("NO_FFE",)),
    "core/narrow(3,4,5)/jit": core_case(g_medium(seed=66), (3, 4, 5), seed=66),
    "core/narrow(10,5,3)/FORCE_GENERIC": core_case(g_medium(seed=67), (10, 5, 3), seed=67, flag_names=("FORCE_GENERIC",)),
    "core/narrow(6,5,3)/no-edges": core_case(g_no_edges, (6, 5, 3), seed=68),
    "core/mid(40,36,33)": core_case(g_medium(seed=69), (40, 36, 33), seed=69),
    # ---- gnx_core_forward: wide ----
    "core/wide/default": core_case(WIDE_G, CORE_W, seed=70, shift=0.75),
    "core/wide/R3/eps1": core_case(g_er(601, 4137), CORE_W, R=3, eps_mode=1, seed=71, shift=0.75),
    "core/wide/4095-edges": core_case(g_er(601, 4095), CORE_W, seed=72, shift=0.75),
    "core/wide/4099-nodes": core_case(g_er(4099, 12007), CORE_W, seed=73, shift=0.75),
    "core/wide/FFN_FP32": core_case(WIDE_G, CORE_W, seed=74, shift=0.75, flag_names=("FFN_FP32",)),
    "core/wide/EDGE_FP32": core_case(WIDE_G, CORE_W, seed=75, shift=0.75, flag_names=("EDGE_FP32",)),
    "core/wide/NO_LN_FUSE": core_case(WIDE_G, CORE_W, seed=76, shift=0.75, flag_names=("NO_LN_FUSE",)),
    "core/wide/LN_STATS_PASS+CORE_EDGE_SPLIT": core_case(WIDE_G, CORE_W, seed=77, shift=0.75, flag_names=("LN_STATS_PASS", "CORE_EDGE_SPLIT")),
    "core/wide/CORE_EDGE_SPLIT/eps1": core_case(WIDE_G, CORE_W, eps_mode=1, seed=78, shift=0.75, flag_names=("CORE_EDGE_SPLIT",)),
    "core/wide/NO_FORK": core_case(WIDE_G, CORE_W, seed=79, shift=0.75, flag_names=("NO_FORK",)),
    "core/wide/LN_ON_LOAD": core_case(WIDE_G, CORE_W, seed=80, shift=0.75, flag_names=("LN_ON_LOAD",)),
    "core/wide/LN_ON_LOAD/4099-nodes/eps1": core_case(g_er(4099, 12007), CORE_W, eps_mode=1, seed=81, shift=0.75, flag_names=("LN_ON_LOAD",)),
    "core/wide/EDGE_N": core_case(WIDE_G, CORE_W, seed=82, shift=0.75, flag_names=("EDGE_N",)),
    "core/width-64(64,64,32)": core_case(g_er(4099, 12007), (64, 64, 32), seed=83),
    "core/width-64(64,48,32)/R2": core_case(g_hub(301, 2400, 150), (64, 48, 32), R=2, seed=84),
    "core/wide/medium-graphs": core_case(g_medium(seed=85), CORE_W, seed=85),
    # ---- training mode ----
    "core-train/narrow(10,5,3)": core_case(g_medium(seed=90), (10, 5, 3), seed=90, dropout=0.25),
    "core-train/wide": core_case(WIDE_G, CORE_W, seed=91, dropout=0.5),
    "core-train/backward/narrow": core_backward_case(g_medium(seed=92), (10, 5, 3), seed=92, dropout=0.25),
    "core-train/backward/big(64,32,16)": core_backward_case(g_big3(seed=93), (64, 32, 16), seed=93, dropout=0.5),
    # ---- Chain blocks ----
    "chain/forward/layernorm": chain_case(g_small(seed=100), (10, 5, 0), [16, "ln", 3], [8, "ln", 4], ["ln", 6, 5], seed=100),
    "chain/forward/ln-first-edge-layer/R3": chain_case(g_hub(333, 2001, 150), (10, 5, 3), ["ln", 12, 7], [6], [4], R=3, seed=101),
    "chain/forward/wide/layernorm": chain_case(g_hub(301, 2400, 150), (128, 64, 32), [256, "ln", 128], [128, "ln", 64], [64, 32], seed=102),
    "chain/backward/small/layernorm": chain_case(g_small(seed=103), (10, 5, 3), [16, "ln", 3], [8, "ln", 4, "ln"], ["ln", 6, 5], seed=103, backward=True),
    "chain/backward/small/ln-first+no-graphfn": chain_case(g_small(seed=104), (10, 5, 3), ["ln", 12, 7], [6, "ln"], [], seed=104, backward=True),
    "chain/backward/big": chain_case(g_big3(seed=105), (48, 24, 8), [64, "ln", 40], [48, 24], [32, 16], seed=105, backward=True),
    # ---- backward ----
    "block-backward/small/readme": block_backward_case(g_small(seed=110), *README, seed=110),
    "block-backward/small/gelu+gf": block_backward_case(g_medium(seed=111), (3, 2, 4), (3, 4, 5), act=(4, 4, 4), seed=111),
    "block-backward/small/width-0-nodefn": block_backward_case(g_small(seed=112), (6, 5, 0), (4, 0, 3), seed=112),
    "block-backward/small/no-edges": block_backward_case(g_no_edges, (4, 3, 2), (2, 3, 2), seed=113),
    "block-backward/big/odd(37,22,5)": block_backward_case(g_big3(seed=114), (37, 22, 5), (35, 19, 7), seed=114),
    "block-backward/big/odd(37,22,5)/R3": block_backward_case(g_er(4099, 12007), (37, 22, 5), (35, 19, 7), seed=121, R=3),
    "block-backward/big/wide": block_backward_case(g_big3(seed=115), *WIDE, seed=115),
    "block-backward/big/gelu": block_backward_case(g_big3(seed=116), (40, 24, 8), (36, 20, 12), act=(4, 4, 4), seed=116),
    "core-backward/small(10,5,3)": core_backward_case(g_small(seed=117), (10, 5, 3), seed=117),
    "core-backward/small/gelu/eps1": core_backward_case(g_medium(seed=118), (3, 4, 5), hidden_act="gelu", eps_mode=1, seed=118),
    "core-backward/big(40,36,33)": core_backward_case(g_big3(seed=119), (40, 36, 33), seed=119),
    "core-backward/big(64,32,16)/gelu": core_backward_case(g_big3(seed=120), (64, 32, 16), hidden_act="gelu", seed=120),
    # ---- the small entry points ----
    "xent/5x37": xent_case(5, 37),
    "xent/7x70001": xent_case(7, 70001, seed=1),
    "pad/small-graphs/d3": pad_case(g_small(seed=130), 3, seed=130),
    "pad/shared/R3/d5": pad_case(lambda gn: (lambda adjs: (gn.GNGraphBatch(adjs), O.csc_from_adj(adjs)))(U.random_graphs(np.random.default_rng(131), (23,), 0.3)), 5, R=3, seed=131),
    "collapse/small-graphs/d3": collapse_case(g_small(seed=132, n=12), 3, seed=132),
    "collapse/shared/R3/d5": collapse_case(lambda gn: (lambda adjs: (gn.GNGraphBatch(adjs), O.csc_from_adj(adjs)))(U.random_graphs(np.random.default_rng(133), (23,), 0.5)), 5, R=3, seed=133),
    "fn-input/small-graphs(3,2,4)": fn_input_case(g_small(seed=134), (3, 2, 4), seed=134),
    "fn-input/hub/R3(5,3,0)": fn_input_case(g_hub(333, 2001, 150), (5, 3, 0), R=3, seed=135),
    "fn-input/wide(128,64,32)": fn_input_case(WIDE_G, (128, 64, 32), seed=136),
    "row-stats/4099x128/eps0": row_stats_case(4099, 128, 0),
    "row-stats/333x64/eps1": row_stats_case(333, 64, 1, seed=1),
    "row-stats/1x512": row_stats_case(1, 512, 0, seed=2),
    "dropout-mask/100003": dropout_mask_case(100003, 0.3, 1),
    "dropout-mask/7": dropout_mask_case(7, 0.5, 0),
}


# every `nothing` combination of inputs and outputs (a buffer's presence changes which pointers a kernel dereferences) on the batch of small graphs
_PRESENT = [c for c in ((a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)) if any(c)]
for _i, _in in enumerate(_PRESENT):
    for _j, _out in enumerate(_PRESENT):
        _ind = tuple(w * m for w, m in zip((3, 2, 4), _in))
        _outd = tuple(w * m for w, m in zip((3, 4, 5), _out))
        CASES[f"block/nothing/{_ind}=>{_outd}"] = block_case(g_small(seed=200 + _i), _ind, _outd, seed=200 + 7 * _i + _j)


# That a case runs the FORM it is in the table for is asserted too, from its profiled run: case -> (names that must appear, names that must not).
# (Skipped — the case itself still runs — when the GNX_* environment switches forms on for the whole process: gnx_default_flags.)
_X6 = {"k_edge_x6_prep", "k_node_x6_prep", "k_proj_x6_prep", "k_ffn_x6_prep", "k_core_edge_x6", "k_ffn_x6"}
_GENERIC = {"k_edge_generic", "k_node_generic", "k_graph"}
_BF16 = {"k_bf16_widen", "k_bf16_round"}
EXPECT = {
    "block/readme/one-graph/R1": ({"k_block_wave", "k_graph_t"}, _GENERIC),
    "block/readme/small-graphs(pack)": ({"k_block_wave"}, {"k_graph_t"} | _GENERIC),
    "block/readme/small-graphs/NO_PACK": ({"k_block_wave", "k_graph_t"}, _GENERIC),
    "block/jit-odd/one-graph/R3": ({"k_block_wave", "k_graph_t"}, _GENERIC),
    "block/jit-even/medium": ({"k_block_wave"}, _GENERIC),
    "block/readme/FORCE_GENERIC": (_GENERIC, {"k_block_wave"}),
    "block/odd/NO_JIT": (_GENERIC, {"k_block_wave"}),
    "block/wide/default": ({"k_edge_x6_prep", "k_rows_gemm_proj", "k_graph_wide"}, _GENERIC),
    "block/wide/4095-edges": ({"k_rows_gemm_edge"}, _X6),
    "block/wide/R3/4096-edges": ({"k_edge_x6_prep"}, set()),
    "block/wide/4097-edges/4099-nodes": ({"k_node_x6_prep"}, set()),
    "block/wide/FP32_MFMA": ({"k_rows_gemm_edge"}, _X6),
    "block/wide/PROJ_FP32": ({"k_edge_x6_prep"}, {"k_node_x6_prep", "k_proj_x6_prep"}),
    "block/wide/NO_MFMA": (_GENERIC, {"k_rows_gemm_edge"}),
    "block/wide/128=>(3,4,5)": ({"k_edge_x6_prep"}, set()),
    "block/wide/128=>(3,4,5)/R3/EDGE_NARROW_FP32": ({"k_rows_gemm_edge"}, _X6),
    "block/wide/128=>(3,4,5)/4095-edges": ({"k_rows_gemm_edge"}, _X6),
    "block/encoder(10,5,0)=>(128,64,32)": ({"k_edge_x6_prep"}, {"k_rows_gemm_proj"}),
    "block/wide-odd(33,17,5)=>(40,35,7)/R3": ({"k_rows_gemm_proj", "k_rows_gemm_edge", "k_rows_gemm_node", "k_graph_wide"}, _GENERIC | _X6 | {"k_block_wave"}),
    "block/chained/one-graph": ({"k_block_wave", "k_graph_t"}, set()),
    "block/steps/mid-widths": ({"k_rows_gemm_edge"}, {"k_block_wave"}),
    "bf16/readme/one-graph/R3": ({"k_block_wave"}, _BF16),
    "bf16/jit-odd/medium": ({"k_block_wave"}, _BF16),
    "bf16/fallback/FORCE_GENERIC/odd/R3": (_BF16 | _GENERIC, {"k_block_wave"}),
    "bf16/fallback/NO_JIT": (_BF16 | _GENERIC, {"k_block_wave"}),
    "bf16/fallback/wide": (_BF16 | {"k_rows_gemm_edge"}, set()),
    "bf16/steps/readme/one-graph": ({"k_block_wave"}, _BF16),
    "bf16/steps/fallback/FORCE_GENERIC": (_BF16 | _GENERIC, {"k_block_wave"}),
    "bf16/steps/fallback/wide": (_BF16 | {"k_rows_gemm_edge"}, set()),
    "core/narrow(10,5,3)/medium": ({"k_block_wave", "k_core_post"}, {"k_ln1_rows"}),
    "core/narrow(10,5,3)/post3(>=65536 rows)": ({"k_block_wave", "k_core_post"}, {"k_graph_t"}),
    "core/narrow(10,5,3)/FORCE_GENERIC": (_GENERIC | {"k_layernorm2", "k_ffn_residual"}, {"k_block_wave"}),
    "core/narrow(6,5,3)/no-edges": ({"k_ln1_rows", "k_core_post"}, set()),
    "core/wide/default": ({"k_core_edge_x6", "k_ffn_fused"}, {"k_ln_stats", "k_rows_gemm_edge"}),
    "core/wide/4095-edges": ({"k_rows_gemm_edge"}, _X6),
    "core/wide/4099-nodes": ({"k_core_edge_x6", "k_ffn_x6", "k_node_x6_prep", "k_proj_x6_prep", "k_ln_stats"}, set()),
    "core/wide/FFN_FP32": ({"k_ffn_fused", "k_edge_x6_prep"}, {"k_ffn_x6", "k_core_edge_x6", "k_ffn_x6_prep"}),
    "core/wide/EDGE_FP32": ({"k_ffn_x6", "k_rows_gemm_edge"}, {"k_edge_x6_prep", "k_core_edge_x6"}),
    "core/wide/NO_LN_FUSE": ({"k_layernorm2", "k_rows_gemm_edge"}, {"k_ln_stats", "k_core_edge_x6"}),
    "core/wide/LN_STATS_PASS+CORE_EDGE_SPLIT": ({"k_ln_stats", "k_ffn_x6", "k_rows_gemm_edge"}, {"k_core_edge_x6"}),
    "core/wide/CORE_EDGE_SPLIT/eps1": ({"k_ffn_x6", "k_rows_gemm_edge"}, {"k_core_edge_x6"}),
    "core/wide/LN_ON_LOAD": ({"k_ln_stats", "k_core_edge_x6"}, set()),
    "core/wide/EDGE_N": ({"k_ffn_x6", "k_rows_gemm_edge"}, {"k_core_edge_x6"}),
    "core/width-64(64,64,32)": ({"k_ffn_x6"}, {"k_core_edge_x6"}),
    "core-train/narrow(10,5,3)": ({"k_dropout", "train_ff1", "train_ff2"}, set()),
    "core-train/wide": ({"k_dropout", "train_ff1", "train_ff2", "k_core_edge_x6"}, set()),
    "core-train/backward/big(64,32,16)": ({"k_dropout", "k_dw_gemm", "bw_dx_node"}, set()),
    "chain/forward/layernorm": ({"k_chain_layernorm", "k_rows_gemm_chain_e", "k_rows_gemm_chain_n", "k_rows_gemm_chain_g"}, set()),
    "chain/backward/big": ({"k_dw_gemm", "bw_dx_chain", "bw_layernorm"}, set()),
    "block-backward/small/readme": ({"bw_dx_generic", "bw_dw_generic", "bw_dnf"}, {"k_dw_gemm", "bw_dx_node"}),
    "block-backward/small/gelu+gf": ({"bw_gelu_preact", "bw_dgf"}, {"k_dw_gemm"}),
    "block-backward/big/odd(37,22,5)/R3": ({"k_dw_gemm", "bw_dx_node", "bw_dx_edge_ef", "bw_segsum_src", "bw_segsum_dst", "bw_dx_nf_src", "bw_dx_nf_dst"},
                                           set()),
    "block-backward/big/wide": ({"k_dw_gemm", "k_dw_final2", "bw_dx_node", "bw_dx_edge_ef", "bw_segsum_src", "bw_segsum_dst"}, set()),
    "block-backward/big/gelu": ({"k_dw_gemm", "bw_gelu_preact", "bw_dx_node"}, set()),
    "core-backward/small/gelu/eps1": ({"bw_gelu_hidden", "bw_layernorm"}, {"k_dw_gemm"}),
    "core-backward/big(64,32,16)/gelu": ({"bw_gelu_hidden", "k_dw_gemm", "bw_ff1_recompute"}, set()),
}
assert set(EXPECT) <= set(CASES), set(EXPECT) - set(CASES)


def _run_case(gn, cid):
    L, lib = _L(gn), _L(gn).load()
    a = AR.Arena("cuda")
    run, verify = CASES[cid](gn, a)
    a.build(ws_fill=0x00)
    bits = []
    for fill, profiled in ((0x00, False), (0xFF, False), (0xFF, True)):
        what = f"{cid} [workspace {fill:#04x}{', profiled' if profiled else ''}]"
        a.refill(fill)
        torch.cuda.synchronize()
        if profiled:
            L.profile_reset()
            L.profile_enable(True)
        try:
            rc = run(a)
            torch.cuda.synchronize()
        finally:
            if profiled:
                L.profile_enable(False)
        assert rc == 0, f"{what}: status {rc}: {lib.gnx_last_error()}"
        a.check(what)
        verify(a, what)
        if profiled:
            SEEN[cid] = set(L.profile_read())
            L.profile_reset()
            if cid in EXPECT and U.default_flags(gn) == 0:
                must, must_not = EXPECT[cid]
                assert must <= SEEN[cid] and not (must_not & SEEN[cid]), \
                    f"{cid}: not the form this case stands for: missing {sorted(must - SEEN[cid])}, unexpected {sorted(must_not & SEEN[cid])}; saw {sorted(SEEN[cid])}"
        else:
            bits.append(a.output_bits())
    for k in bits[0]:
        same = torch.equal(bits[0][k], bits[1][k])
        if not same:
            d = (bits[0][k] != bits[1][k]).nonzero().view(-1)
            raise AssertionError(f"{cid}: output '{k}' depends on what the workspace held before the call: {int(d.numel())} bytes differ between a 0x00 "
                                 f"and a 0xFF workspace, first at byte {int(d[0])}, last at {int(d[-1])}")
    DONE.add(cid)


@pytest.mark.parametrize("cid", list(CASES), ids=list(CASES))
def test_memory_contract(gn, cid):
    _run_case(gn, cid)


def profiler_names():
    """every name the sources can hand to the profiler: the literals of `ProfScope ps("...")`, and — where a ProfScope takes a `name` parameter —
    the literals at the call sites of the functions that pass one down"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphnets.jl_amd", "csrc")
    text = {f: open(os.path.join(src, f), encoding="utf-8").read() for f in sorted(os.listdir(src)) if f.endswith((".hip", ".cpp", ".h"))}
    names = set()
    for t in text.values():
        names |= set(re.findall(r'ProfScope\s+\w+\(\s*"([^"]+)"', t))
    # functions with a `const char* name` parameter (definitions and declarations), transitively: whoever forwards `name` to one of them
    takers = set()
    for t in text.values():
        takers |= set(re.findall(r'\b(\w+)\s*\([^;{}()]*\bconst char\*\s*name\b[^;{}()]*\)\s*[;{]', t))
    takers -= {"ProfScope", "env_int", "env_on"}
    assert {"segsum_rows", "launch_gemm"} <= takers, takers
    for t in text.values():
        for fn in takers:
            for m in re.finditer(r'\b' + fn + r'\s*\(', t):
                depth, i = 1, m.end()
                while depth and i < len(t):
                    depth += {"(": 1, ")": -1}.get(t[i], 0)
                    i += 1
                names |= set(re.findall(r'"([A-Za-z_][A-Za-z0-9_]*)"', t[m.end():i]))
    return names


def test_every_profiled_kernel_name_is_covered(gn):
    """Completeness: each profiler name of csrc/ was seen in some case's profiled run, or stands in NOT_COVERED (at most 4 names, none of them a
    kernel that writes a buffer the caller passed)."""
    names = profiler_names()
    assert len(names) >= 41, sorted(names)
    assert len(NOT_COVERED) <= 4 and set(NOT_COVERED) <= names, NOT_COVERED
    for cid in CASES:  # (a selection of cases, or this test alone: run what has not run)
        if cid not in DONE:
            _run_case(gn, cid)
    seen = set().union(*SEEN.values())
    missing = sorted(names - seen - set(NOT_COVERED))
    assert not missing, f"no memory-contract case ran these kernels: {missing}; seen: {sorted(seen)}"
    unknown = sorted(seen - names)
    assert not unknown, f"the profiler reported names the source scan does not find: {unknown}"
