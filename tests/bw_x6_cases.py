"""The cases, references and comparisons of the backward's arithmetic stress: shared by tests/test_bw_x6_stress_cpu.py (no GPU: the oracle's values,
the soundness of the bar on every case, the controls), tests/bw_x6_stress_child.py (runs the cases on the device) and tests/test_gpu_bw_x6_stress.py
(compares on the CPU).  Nothing here touches the device or the library.

One graph, N = 1031 nodes and E = 4099 edges: 33 chunks of 128 rows for k_dw_gemm, the last with 3 rows (a partial chunk and a partial 32-row
panel).  A case is (id, kind, widths, activations, variant); `data(cid)` draws it — seeded by the id's position, the same in every process — and
`reference(cid)` evaluates, once per process: the float64 oracle with its scale S (oracle/gn_oracle.py: *_backward_sparse) and the YARDSTICK, the same
pullback evaluated by plain torch float32 autograd on the CPU.  For gnx_block_backward the forward outputs are inputs at the ABI — the float64
forward rounded to fp32 — and both references take them as given (`_GivenY`): what follows a level is built from the given output and
act' of tanh / sigmoid is taken from it; a gelu level differentiates its recomputed pre-activation.

The bar: |got - ref| <= 1e-5 . S for every element (U.RTOL, the forward's own bar).  The statistical criterion, for tensors of >= 4096 elements: the
mean of |got - ref| / S is at most K_MEAN = 4 times the yardstick's mean (the controls of tests/test_bw_x6_stress_cpu.py put a six-term product at
about 0.5 x and a three-term product at more than 8 x a torch fp32 matmul: a factor >= 2 on both sides of 4)."""
import functools

import numpy as np
import torch

from oracle import gn_oracle as O
from tests import util as U
from tests.test_gpu_backward import ACT, _torch_block

N_NODES, N_EDGES, GRAPH_SEED = 1031, 4099, 11
K_MEAN = 4.0
MIN_STAT = 4096
BLOCK_BAR, CORE_BAR = 2e-4, 1e-3  # the legacy normwise bars (tests/test_gpu_backward.py, tests/test_gpu_chain.py): bar . max(1, max|ref|)
DX = ("d_ef", "d_nf", "d_gf")
FNS = (("edgefn", "We", "be"), ("nodefn", "Wn", "bn"), ("graphfn", "Wg", "bg"))
BLOCK_NAMES = set(DX) | set(O.BLOCK_GRAD_NAMES)
CORE_NAMES = BLOCK_NAMES | {f"grad.{ln}_{t}.{k}" for ln in ("ln1", "ln2") for t in "eng" for k in ("gamma", "beta")} \
    | {f"grad.ff_{t}.{fc}.{k}" for t in "eng" for fc in ("fc1", "fc2") for k in ("dW", "db")}
assert len(BLOCK_NAMES) == 9 and len(CORE_NAMES) == 33
F64, F32 = torch.float64, torch.float32

W = (128, 64, 32)
B1, B2, B3, B4 = (W, W), ((37, 22, 5), (35, 19, 7)), ((40, 24, 8), (132, 20, 12)), ((40, 24, 8), (36, 20, 12))
SMOOTH, IDENT, GELU = (2, 3, 0), (0, 0, 0), (4, 4, 4)
# (id, kind, widths, activations | hidden activation, variant)
CASES = [
    ("B1-plain", "block", B1, SMOOTH, "plain"),
    ("B1-log_uniform_inputs", "block", B1, SMOOTH, "log_uniform_inputs"),
    ("B1-log_uniform_cotangents", "block", B1, SMOOTH, "log_uniform_cotangents"),
    ("B1-log_uniform_weights", "block", B1, SMOOTH, "log_uniform_weights"),
    ("B1-cancelling_dW", "block", B1, IDENT, "cancelling_dW"),
    ("B1-cancelling_dX", "block", B1, IDENT, "cancelling_dX"),
    ("B2-plain", "block", B2, SMOOTH, "plain"),
    ("B2-log_uniform_cotangents", "block", B2, SMOOTH, "log_uniform_cotangents"),
    ("B3-plain", "block", B3, SMOOTH, "plain"),
    ("B3-log_uniform_cotangents", "block", B3, SMOOTH, "log_uniform_cotangents"),
    # plain inputs, centred (2 x - 1): on U[0, 1) features the gelu outputs are mostly positive and torch's sequential fp32 sum of the 4099 of them
    # drifts to 0.2565 of 1e-5 . S on dWg — above the quarter that tests/test_bw_x6_stress_cpu.py asks of plain fp32; the case moves, not the bar
    ("B4-gelu-plain", "block", B4, GELU, "plain_centred"),
    ("C1-plain", "core", W, "tanh", "plain"),
    ("C1-wide_gamma", "core", W, "tanh", "wide_gamma"),
    ("C1-log_uniform_ffn_weights", "core", W, "tanh", "log_uniform_ffn_weights"),
    ("C1-log_uniform_cotangents", "core", W, "tanh", "log_uniform_cotangents"),
    ("C1-cancelling_hidden", "core", W, "tanh", "cancelling_hidden"),
    ("C2-relu-plain", "core", W, "relu", "plain"),
    ("C3-10x5x3-relu", "core", (10, 5, 3), "relu", "plain"),
    ("C4-40x36x33-gelu", "core", (40, 36, 33), "gelu", "plain"),
]
CASE_IDS = [c[0] for c in CASES]
ROWS = (N_EDGES, N_NODES, 1)
HIDDEN_CODE = dict(tanh=O.ACT_TANH, relu=O.ACT_RELU, gelu=O.ACT_GELU)


@functools.lru_cache(maxsize=None)
def graph_parts():
    """(colptr, rowval) of the one graph"""
    return U.er_csc(np.random.default_rng(GRAPH_SEED), N_NODES, N_EDGES)


def csc():
    colptr, rowval = graph_parts()
    return colptr, rowval, np.array([0, N_NODES], dtype=np.int64), np.array([0, N_EDGES], dtype=np.int64)


def log_uniform(rng, shape, lo=-6.0, hi=6.0):
    """every element its own magnitude, 10^lo .. 10^hi, random sign"""
    return (10.0 ** rng.uniform(lo, hi, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def data(cid):
    """block: dict(p, x, y (the float64 forward rounded to fp32), cot); core: dict(p, x, cot, act).  All packed [1][T][d] float32."""
    i = CASE_IDS.index(cid)
    _, kind, dims, act, variant = CASES[i]
    rng = np.random.default_rng(9000 + i)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    if kind == "block":
        din, dout = dims
        p = O.make_block_params(rng, din, dout, act=act)
        x = list(U.packed_inputs(rng, 1, *ROWS, din))
        cot = [f32(rng.standard_normal((1, T, d))) for T, d in zip(ROWS, dout)]
        if variant == "log_uniform_inputs":
            x = [log_uniform(rng, v.shape) for v in x]
        elif variant == "plain_centred":
            x = [f32(2 * v - 1) for v in x]
        elif variant == "log_uniform_cotangents":
            cot = [log_uniform(rng, c.shape) for c in cot]
        elif variant == "log_uniform_weights":
            p["We"] = f32(p["We"] * 10.0 ** rng.uniform(-4, 4, size=p["We"].shape))
        elif variant == "cancelling_dW":  # a common mode of 1e4 on the features against cotangent columns that sum to zero over the rows
            x = [f32(v + 1e4) for v in x]
            g = cot[0].astype(np.float64)
            cot = [f32(g - g.mean(axis=1, keepdims=True)), np.zeros_like(cot[1]), np.zeros_like(cot[2])]
        elif variant == "cancelling_dX":  # a common mode of 1e4 on the cotangent against weights whose sum over the outputs is zero for every input
            cot[0] = f32(1e4 + cot[0])
            We = p["We"].astype(np.float64)
            p["We"] = f32(We - We.mean(axis=0, keepdims=True))
        else:
            assert variant == "plain", variant
        y = [f32(v) for v in O.block_forward_sparse(p, csc(), *x)]
        return dict(kind=kind, p=p, x=tuple(x), y=tuple(y), cot=tuple(cot))
    p = O.make_core_params(rng, dims)
    if variant == "wide_gamma":  # the FeedForward's input (and the cotangent of gn2) then spans six decades
        for t, d in zip("en", dims):
            p[f"ln2_{t}_gamma"], p[f"ln2_{t}_beta"] = log_uniform(rng, (d,), -3, 3), log_uniform(rng, (d,), -3, 3)
    elif variant == "log_uniform_ffn_weights":
        for t in "en":
            for k in ("W1", "W2"):
                p[f"ff_{t}_{k}"] = f32(p[f"ff_{t}_{k}"] * 10.0 ** rng.uniform(-4, 4, size=p[f"ff_{t}_{k}"].shape))
    elif variant == "cancelling_hidden":  # hidden units in identical pairs whose second-layer weights are opposite up to 1e-4 (tests/test_gpu_x6_stress.py)
        for t in "en":
            W1, W2 = p[f"ff_{t}_W1"], p[f"ff_{t}_W2"]
            W1[1::2] = W1[0::2]
            p[f"ff_{t}_b1"][1::2] = p[f"ff_{t}_b1"][0::2]
            W2[:, 1::2] = -W2[:, 0::2] * np.float32(1.0001)
    if act == "relu":
        x, rounds, _ = U.kinkfree_core_inputs(rng, p, 1, *ROWS)
        for t, v in zip("eng", x):
            assert not U.relu_kink_rows(p, t, v).any(), (cid, t)
    else:
        x = U.packed_inputs(rng, 1, *ROWS, dims)
    cot = [f32(rng.standard_normal(v.shape)) for v in x]
    if variant == "log_uniform_cotangents":
        cot = [log_uniform(rng, c.shape) for c in cot]
    return dict(kind=kind, p=p, x=tuple(x), cot=tuple(cot), act=act)


# ---------------------------------------------------------------------------------------------------------------------------------------
# torch restatements of the pullbacks
# ---------------------------------------------------------------------------------------------------------------------------------------
class _GivenY(torch.autograd.Function):
    """An activation level as gnx_block_backward sees it: the level's output is the GIVEN forward output y, and the derivative is taken from it
    (identity 1, relu y > 0, tanh 1 - y^2, sigmoid y (1 - y))."""

    @staticmethod
    def forward(ctx, z, y, code):
        ctx.save_for_backward(y)
        ctx.code = code
        return y.clone()

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        d = {0: torch.ones_like(y), 1: (y > 0).to(y.dtype), 2: 1 - y * y, 3: y * (1 - y)}[ctx.code]
        return g * d, None, None


def _given(code, y):
    if code == 4:  # gelu: the value is the given output (gelu(z) - gelu(z) is exactly zero), the derivative that of gelu at the recomputed z
        return lambda z: y + (ACT[4](z) - ACT[4](z).detach())
    return lambda z: _GivenY.apply(z, y, code)


def torch_block_grads(p, csc_, x, cot, dt, y=None):
    """The nine gradients of a block by torch autograd in `dt`, replica by replica on one set of parameter leaves, in the layout of the ABI, as
    float64 numpy ({name: array | None}).  `y` (packed, None for a zero width): the forward outputs as given; without it the forward's own."""
    Wt = {k: torch.tensor(p[k], dtype=dt, requires_grad=True) for k in ("We", "be", "Wn", "bn", "Wg", "bg")}
    R = next(v.shape[0] for v in x if v is not None)
    T = lambda v, r, grad: None if v is None else torch.tensor(v[r], dtype=dt, requires_grad=grad)
    xs = [[T(v, r, True) for v in x] for r in range(R)]
    codes = (p["act_e"], p["act_n"], p["act_g"])
    loss = 0.0
    for r in range(R):
        acts = None
        if y is not None:
            rows = (len(csc_[1]), len(csc_[0]) - 1, len(csc_[2]) - 1)
            ys = [torch.zeros((t, 0), dtype=dt) if v is None else T(v, r, False) for v, t in zip(y, rows)]
            acts = [_given(c, v) for c, v in zip(codes, ys)]
        outs = _torch_block(p, csc_, *xs[r], Wt, acts=acts)
        loss = loss + sum((o * torch.tensor(c[r], dtype=dt)).sum() for o, c in zip(outs, cot) if c is not None)
    loss.backward()
    f = lambda t: (torch.zeros_like(t) if t.grad is None else t.grad).double().numpy()  # (a zero-width function: no gradient flows)
    ref = {n: None if x[k] is None else np.stack([f(xs[r][k]) for r in range(R)]) for k, n in enumerate(DX)}
    for fn, w, b in FNS:
        ref[f"grad.{fn}.dW"], ref[f"grad.{fn}.db"] = f(Wt[w]).T, f(Wt[b])
    return ref


def torch_core_grads(p, csc_, x, cot, act, dt):
    """The 33 gradients of a core by torch autograd of tests/test_gpu_memory_contract.py's _torch_core in `dt`, replica by replica on one set of
    leaves, in the layout of the ABI, as float64 numpy (tests/test_gpu_backward_replicas.py's _core_reference, with tanh among the activations)"""
    from tests import test_gpu_memory_contract as MC
    Wl, Wb = MC._core_leaves(p, dt)
    hidden = {"tanh": torch.tanh, "relu": torch.relu, "gelu": ACT[4]}[act]
    R = x[0].shape[0]
    xs = [[torch.tensor(v[r], dtype=dt, requires_grad=True) for v in x] for r in range(R)]
    loss = 0.0
    for r in range(R):
        outs = MC._torch_core(p, csc_, xs[r], Wl, Wb, hidden)
        loss = loss + sum((o * torch.tensor(c[r], dtype=dt)).sum() for o, c in zip(outs, cot))
    loss.backward()
    f = lambda t: t.grad.double().numpy()
    ref = {n: np.stack([f(xs[r][k]) for r in range(R)]) for k, n in enumerate(DX)}
    for fn, w, b in FNS:
        ref[f"grad.{fn}.dW"], ref[f"grad.{fn}.db"] = f(Wb[w]).T, f(Wb[b])
    for t in "eng":
        for ln in ("ln1", "ln2"):
            for k in ("gamma", "beta"):
                ref[f"grad.{ln}_{t}.{k}"] = f(Wl[f"{ln}_{t}_{k}"])
        for fc, wk, bk in (("fc1", "W1", "b1"), ("fc2", "W2", "b2")):
            ref[f"grad.ff_{t}.{fc}.dW"], ref[f"grad.ff_{t}.{fc}.db"] = f(Wl[f"ff_{t}_{wk}"]).T, f(Wl[f"ff_{t}_{bk}"])
    return ref


@functools.lru_cache(maxsize=None)
def reference(cid):
    """(ref, S, yard): the float64 oracle's gradients, their scales, the float32 torch evaluation — {name: float64 array}"""
    d = data(cid)
    if d["kind"] == "block":
        ref, S = O.block_backward_sparse(d["p"], csc(), d["x"], d["y"], d["cot"])
        yard = torch_block_grads(d["p"], csc(), d["x"], d["cot"], F32, y=d["y"])
    else:
        ref, S = O.core_backward_sparse(d["p"], csc(), d["x"], d["cot"], hidden_act=HIDDEN_CODE[d["act"]])
        yard = torch_core_grads(d["p"], csc(), d["x"], d["cot"], d["act"], F32)
    assert set(ref) == set(S) == set(yard) == names(cid)
    return ref, S, yard


def names(cid):
    return BLOCK_NAMES if CASES[CASE_IDS.index(cid)][1] == "block" else CORE_NAMES


# ---------------------------------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------------------------------
def ratios(got, ref, S):
    """(worst, mean) of |got - ref| / (1e-5 . S) over the elements with S > 0, and whether every element with S = 0 is exactly 0"""
    got, ref, S = (np.asarray(a, dtype=np.float64) for a in (got, ref, S))
    assert got.shape == ref.shape == S.shape, (got.shape, ref.shape, S.shape)
    pos = S > 0
    r = np.abs(got - ref)[pos] / (U.RTOL * S[pos])
    return (float(r.max()) if r.size else 0.0, float(r.mean()) if r.size else 0.0), bool((got[~pos] == 0).all())


def check_elementwise(got, ref, S, what):
    """assertions a and b of one tensor; returns (worst, mean) ratio to 1e-5 . S"""
    assert np.isfinite(np.asarray(got)).all(), f"{what}: not finite"
    (worst, mean), zeros = ratios(got, ref, S)
    assert zeros, f"{what}: an element whose scale is 0 is not exactly 0"
    assert worst <= 1.0, f"{what}: worst |got - ref| / (1e-5 . S) = {worst:.3f}"
    return worst, mean


def check_statistical(mean, yard_mean, size, what, k=K_MEAN):
    """assertion c; returns mean / yardstick mean (None for a tensor too small for statistics)"""
    if size < MIN_STAT:
        return None
    assert mean <= k * yard_mean, f"{what}: mean |got - ref| / S is {mean / max(yard_mean, 1e-300):.2f} x the float32 evaluation's ({mean * U.RTOL:.3e} against {yard_mean * U.RTOL:.3e})"
    return mean / yard_mean if yard_mean > 0 else (0.0 if mean == 0 else float("inf"))


def legacy_close(got, ref, bar):
    """the normwise bar of tests/test_gpu_backward*.py: max|got - ref| <= bar . max(1, max|ref|)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.isfinite(got).all() and np.abs(got - ref).max() <= bar * max(1.0, float(np.abs(ref).max())))


# ---------------------------------------------------------------------------------------------------------------------------------------
# which code a case must run (csrc/gnx_backward_wide.hip: bw_use_mfma, bw_use_mfma_dw; csrc/gnx_backward.hip: the scopes)
# ---------------------------------------------------------------------------------------------------------------------------------------
def bw_use_mfma(rows, J, K):
    return rows >= 64 and J * K >= 64 and J >= 2 and K >= 2


def bw_use_mfma_dw(rows, J, K):
    return rows >= 64 and J * K >= 1024 and J >= 8 and K >= 8


def _block_scopes(din, dout, acts, rows=ROWS):
    """(must, must_not) of one gnx_block_backward"""
    (de, dn, dg), (oe, on, og) = din, dout
    E, N, G = rows
    Ke, Kn = de + 2 * dn + dg, oe + dn + dg
    must, dw = set(), False
    edge = acts[0] != 4 and bw_use_mfma(E, oe, Ke)
    if edge:
        must |= {"bw_dx_edge_ef", "bw_segsum_dst", "bw_segsum_src", "bw_dx_nf_src", "bw_dx_nf_dst"}
        dw |= bw_use_mfma_dw(E, oe, de) or bw_use_mfma_dw(N, oe, dn) or bw_use_mfma_dw(G, oe, dg)
    if bw_use_mfma(N, on, Kn):
        must.add("bw_dx_node")
        dw |= bw_use_mfma_dw(N, on, Kn)
    if 4 in acts:
        must.add("bw_gelu_preact")
    if dw:
        must.add("k_dw_gemm")
    must_not = set() if dw else {"k_dw_gemm"}
    if not edge:
        must_not |= {"bw_dx_edge_ef"}
    if 4 not in acts:
        must_not.add("bw_gelu_preact")
    return must, must_not


def expected_scopes(cid):
    """(must, must_not): profiler scope names of the case under the default selection of kernels"""
    _, kind, dims, act, _ = CASES[CASE_IDS.index(cid)]
    if kind == "block":
        return _block_scopes(*dims, act)
    must, must_not = _block_scopes(dims, dims, IDENT)  # the core's block: identity activations
    ff_dx = ff_dw = False
    for rows, D in zip(ROWS, dims):
        if bw_use_mfma(rows, D, 4 * D):
            ff_dx = True
            ff_dw |= bw_use_mfma_dw(rows, 4 * D, D) or bw_use_mfma_dw(rows, D, 4 * D)
    assert ff_dx
    must |= {"bw_dx_ff2", "bw_dx_ff1", "bw_ff1_recompute", "bw_layernorm"}
    if ff_dw:
        must.add("k_dw_gemm")
        must_not.discard("k_dw_gemm")
    # gelu: the core recomputes the hidden pre-activation under bw_ff1_recompute and turns it into the hidden units under bw_gelu_hidden
    (must if act == "gelu" else must_not).add("bw_gelu_hidden")
    return must, must_not
