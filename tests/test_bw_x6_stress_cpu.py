"""What tests/test_gpu_bw_x6_stress.py rests on, checked without a GPU:

1. the float64 pullback oracle (oracle/gn_oracle.py: block_backward_sparse, core_backward_sparse) equals torch float64 autograd of the restatements
   the backward tests already use, to 1e-11 . S, and S >= |value| everywhere;
2. the bar is sound on every case of the GPU module: the same pullback evaluated by plain torch float32 stays within a quarter of 1e-5 . S;
3. the bar is not vacuous: one element of a low-magnitude row off by 1e-3 of its value fails it, and passes the legacy normwise bar;
4. the statistical criterion separates: an emulation of k_dw_gemm's arithmetic (16 rows per step, the terms of x6_mma small first, 128-row chunks,
   X6Frag's round-to-nearest split) measures the six-term product at <= 2 x a torch fp32 matmul's mean error / S and a three-term product
   (16 mantissa bits) at >= 8 x, while that three-term product passes both legacy bars; a one-plane (bf16) product fails 1e-5 . S."""
import numpy as np
import pytest
import torch

from oracle import gn_oracle as O
from tests import bw_x6_cases as BC
from tests import util as U


def _small_graphs():
    """three graphs, nodes without edges inside them, one graph without any edge"""
    rng = np.random.default_rng(5)
    adjs = U.random_graphs(rng, [7, 4, 9], 0.35)
    adjs[0][2, :] = 0; adjs[0][:, 2] = 0   # an isolated node
    adjs[2][:, 5:] = 0                      # nodes without in-edges
    adjs[1][:] = 0                          # a graph without edges
    return O.csc_from_adj(adjs)


def _assert_oracle(val, S, ref, what):
    assert set(val) == set(S) == set(ref), what
    for n in sorted(ref):
        if ref[n] is None:
            assert val[n] is None and S[n] is None, (what, n)
            continue
        v, s, r = val[n], S[n], np.asarray(ref[n])
        assert v.shape == s.shape == r.shape, (what, n, v.shape, s.shape, r.shape)
        assert (s >= np.abs(v)).all(), f"{what} {n}: a scale below the value"
        assert (np.abs(v - r) <= 1e-11 * s).all(), f"{what} {n}: {float(np.max(np.abs(v - r) / (s + 1e-300))):.3e} of S"


BLOCK_DIMS = [((10, 5, 3), (3, 4, 5)), ((10, 5, 0), (3, 4, 5)), ((0, 2, 0), (2, 2, 2)), ((4, 0, 3), (2, 3, 2)), ((6, 5, 0), (4, 3, 0))]
BLOCK_ACTS = [(0, 0, 0), (1, 2, 3), (2, 3, 4), (3, 4, 1), (4, 1, 2)]  # every activation at every level


@pytest.mark.parametrize("acts", BLOCK_ACTS, ids=lambda a: "act" + "".join(map(str, a)))
@pytest.mark.parametrize("dims", BLOCK_DIMS, ids=lambda d: "x".join(map(str, d[0])) + "=>" + "x".join(map(str, d[1])))
def test_block_oracle_equals_float64_autograd(dims, acts):
    csc = _small_graphs()
    rows = (len(csc[1]), len(csc[0]) - 1, len(csc[2]) - 1)
    R = 2
    rng = np.random.default_rng(100 + sum(dims[0]) + 7 * sum(acts))
    p = O.make_block_params(rng, *dims, act=acts)
    x = tuple(None if v is None else (v * 3 - 1).astype(np.float32) for v in U.packed_inputs(rng, R, *rows, dims[0]))
    cot = tuple(rng.standard_normal((R, T, d)).astype(np.float32) if d else None for T, d in zip(rows, dims[1]))
    y64 = O.block_forward_sparse(p, csc, *x)
    # the forward's own outputs: plain autograd of the restatement
    val, S = O.block_backward_sparse(p, csc, x, y64, cot)
    _assert_oracle(val, S, BC.torch_block_grads(p, csc, x, cot, BC.F64), "own outputs")
    # the outputs as given (rounded to fp32, as at the ABI): what follows a level and act' come from them
    y32 = tuple(None if v is None else v.astype(np.float32) for v in y64)
    val, S = O.block_backward_sparse(p, csc, x, y32, cot)
    _assert_oracle(val, S, BC.torch_block_grads(p, csc, x, cot, BC.F64, y=y32), "given outputs")
    assert set(val) == BC.BLOCK_NAMES


@pytest.mark.parametrize("eps_mode", [0, 1])
@pytest.mark.parametrize("act", ["relu", "tanh", "gelu"])
def test_core_oracle_equals_float64_autograd(act, eps_mode):
    csc = _small_graphs()
    rows = (len(csc[1]), len(csc[0]) - 1, len(csc[2]) - 1)
    R, dims = 2, (6, 5, 4)
    rng = np.random.default_rng(200 + eps_mode)
    p = O.make_core_params(rng, dims, eps_mode=eps_mode)
    x = tuple((v * 3 - 1).astype(np.float32) for v in U.packed_inputs(rng, R, *rows, dims))
    cot = tuple(rng.standard_normal(v.shape).astype(np.float32) for v in x)
    val, S = O.core_backward_sparse(p, csc, x, cot, hidden_act=BC.HIDDEN_CODE[act])
    assert set(val) == BC.CORE_NAMES
    _assert_oracle(val, S, BC.torch_core_grads(p, csc, x, cot, act, BC.F64), f"core {act} eps_mode {eps_mode}")


@pytest.mark.parametrize("cid", BC.CASE_IDS)
def test_bar_is_sound_on_every_case(cid):
    """plain torch float32 keeps a 4 x margin to 1e-5 . S on every element of every gradient: what a kernel misses is the kernel's"""
    ref, S, yard = BC.reference(cid)
    worst = {}
    for n in sorted(ref):
        assert np.isfinite(ref[n]).all() and np.isfinite(S[n]).all() and (S[n] >= np.abs(ref[n])).all(), (cid, n)
        (w, _), zeros = BC.ratios(yard[n], ref[n], S[n])
        worst[n] = w
        assert zeros, (cid, n)
    print(f"SOUND {cid}: worst float32 error / (1e-5 . S) = {max(worst.values()):.4f} ({max(worst, key=worst.get)})")
    assert max(worst.values()) <= 0.25, (cid, {n: round(w, 4) for n, w in worst.items() if w > 0.25})


def test_cancelling_cases_cancel():
    for cid, n in (("B1-cancelling_dW", "grad.edgefn.dW"), ("B1-cancelling_dX", "d_ef")):
        ref, S, _ = BC.reference(cid)
        assert np.median(S[n] / (np.abs(ref[n]) + 1e-300)) >= 1e4, (cid, n)


def test_bar_is_not_vacuous():
    """one element of a low-magnitude row, off by 1e-3 of its value: the elementwise bar fails, the legacy normwise bar passes"""
    ref, S, _ = BC.reference("B1-log_uniform_cotangents")
    name = "grad.graphfn.dW"  # [in][out]: the row of output j of the (out x in) weight gradient is column j here, of the magnitude of g_gf_out[j]
    r, s = ref[name].T, S[name].T
    row_max = np.abs(r).max(axis=1)
    row = int(np.argsort(row_max)[len(row_max) // 4])  # a row in the lowest quarter of magnitudes
    assert 0 < row_max[row] <= 1e-4 * np.abs(r).max()
    col = int(np.argmin(s[row] / (np.abs(r[row]) + 1e-300)))  # its best-conditioned element
    assert s[row, col] <= 50 * abs(r[row, col]), "no element of the row carries its value in few terms"
    got = {n: v.copy() for n, v in ref.items()}
    got[name][col, row] *= 1 + 1e-3
    assert got[name][col, row] != ref[name][col, row]
    for n in ref:
        assert BC.legacy_close(got[n], ref[n], BC.BLOCK_BAR) and BC.legacy_close(got[n], ref[n], BC.CORE_BAR), n
        if n != name:
            BC.check_elementwise(got[n], ref[n], S[n], n)
    with pytest.raises(AssertionError, match="worst"):
        BC.check_elementwise(got[name], ref[name], S[name], name)


# ---------------------------------------------------------------------------------------------------------------------------------------
# controls: k_dw_gemm's arithmetic emulated
# ---------------------------------------------------------------------------------------------------------------------------------------
def bf16_rn(x):
    """float32 -> nearest bfloat16 (ties to even), as float32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    """X6Frag: x = h + m + l, h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)"""
    x = np.asarray(x, dtype=np.float32)
    h = bf16_rn(x)
    r = x - h
    m = bf16_rn(r)
    return h, m, bf16_rn(r - m)


SIX = ("mm", "lh", "hl", "mh", "hm", "hh")   # x6_mma's order (A part, B part), small terms first
THREE = ("mh", "hm", "hh")                   # 16 mantissa bits
ONE = ("hh",)                                # a plain bf16 product


def dw_emulated(X, D, terms, step=16, chunk=128):
    """dW = X^T D as k_dw_gemm<., X6> forms it: per 128-row chunk an fp32 accumulator that takes, for every 16 rows, one matrix instruction per term
    (the 16 products of bf16 parts are exact, their sum is rounded into the accumulator once); the chunks are added in order in fp32."""
    px, pd = dict(zip("hml", split3(X))), dict(zip("hml", split3(D)))
    px = {k: v.astype(np.float64) for k, v in px.items()}
    pd = {k: v.astype(np.float64) for k, v in pd.items()}
    total = np.zeros((X.shape[1], D.shape[1]), dtype=np.float32)
    for c0 in range(0, X.shape[0], chunk):
        acc = np.zeros_like(total)
        for r0 in range(c0, min(c0 + chunk, X.shape[0]), step):
            r1 = min(r0 + step, c0 + chunk, X.shape[0])
            for a, b in terms:
                acc = (acc.astype(np.float64) + px[a][r0:r1].T @ pd[b][r0:r1]).astype(np.float32)
        total = total + acc
    return total


def _operands(kind):
    """4099 rows, K = J = 128, rng seed 1"""
    rng = np.random.default_rng(1)
    shape = (4099, 128)
    if kind == "plain":  # X ~ U[0, 1), delta = N(0, 1) . U[0, 1)
        X = rng.random(shape, dtype=np.float32)
        D = (rng.standard_normal(shape) * rng.random(shape)).astype(np.float32)
    else:
        X, D = BC.log_uniform(rng, shape), BC.log_uniform(rng, shape)
    return X, D


CONTROL = {}


@pytest.mark.parametrize("kind", ["plain", "log_uniform"])
def test_controls_of_the_statistical_criterion(kind):
    X, D = _operands(kind)
    ref = X.astype(np.float64).T @ D.astype(np.float64)
    S = np.abs(X).astype(np.float64).T @ np.abs(D).astype(np.float64)
    err = lambda got: np.abs(np.asarray(got, dtype=np.float64) - ref) / S
    yard = err((torch.from_numpy(X).T @ torch.from_numpy(D)).numpy())
    six, three, one = (dw_emulated(X, D, t) for t in (SIX, THREE, ONE))
    e6, e3, e1 = err(six), err(three), err(one)
    CONTROL[kind] = dict(yard=(yard.max(), yard.mean()), six=(e6.max(), e6.mean()), three=(e3.max(), e3.mean()), one=(e1.max(), e1.mean()))
    print(f"CONTROL {kind}: torch fp32 matmul max {yard.max():.2e} mean {yard.mean():.2e} | six terms max {e6.max():.2e} mean {e6.mean():.2e} "
          f"({e6.mean() / yard.mean():.2f} x) | three terms max {e3.max():.2e} mean {e3.mean():.2e} ({e3.mean() / yard.mean():.1f} x) | one plane max {e1.max():.2e}")
    assert e6.max() <= U.RTOL and e6.mean() <= 2.0 * yard.mean()
    assert e3.mean() >= 8.0 * yard.mean()
    # so K_MEAN = 4 has a factor >= 2 on both sides
    assert e6.mean() * 2.0 <= BC.K_MEAN * yard.mean() <= e3.mean() / 2.0
    assert BC.legacy_close(three, ref, BC.BLOCK_BAR) and BC.legacy_close(three, ref, BC.CORE_BAR), "the three-term product must pass both legacy bars"
    assert e1.max() > U.RTOL, "the one-plane product must fail 1e-5 . S"
