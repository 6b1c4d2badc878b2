"""What tests/test_gpu_chain_bw_stress.py rests on, checked without a GPU:

1. the float64 pullback oracle of a block with Chain update functions (oracle/gn_oracle.py: chain_block_backward_sparse) equals torch float64
   autograd of tests/chain_torch.py's _torch_chain_block to 1e-11 . S per element — on every case of tests/chain_bw_cases.py and on small random
   chains with both eps modes, every activation as hidden and as last layer, `nothing` inputs and an empty chain —, S >= |value| everywhere, and the
   sqrt-eps forward equals float64 torch to the same bar;
2. the scale.  S is the pullback's first-order error scale (oracle: _dense_pullback1, _ln_pullback1).  The product rule the block and the core use
   (S_a . S_b for a . b) multiplies, layer after layer and level after level, the ratio S / |value| of every recomputed operand, and on this batch —
   sums over up to 2150 edges in front of tanh, sigmoid, gelu and LayerNorm — gives scales of up to 1e27 times the gradient: a bar nothing can
   fail.  The first-order rule is asserted to lie at or below the product rule's S on every element of every case (a bound that is never wider),
   and its median S / |ref| per case is printed.  It is still a worst-case bound through a forward chain of three levels, and stays loose where
   LayerNorms follow sums (1e7 .. 1e9 in the LayerNorm cases): there the statistical criterion of the GPU module, which compares with a float32
   evaluation and does not depend on how loose S is, is what carries weight.
3. the bar is sound on every case: the same pullback by plain torch float32 stays within a quarter of 1e-5 . S on every element;
4. controls: a plain numpy float32 restatement of the fused kernel's per-row arithmetic (k_chain_mlp_bw: the row's forward, k_ln_backward's formula,
   parameter gradients summed per 64-row chunk) passes the bar as it stands and is then mutated three ways, each on a named case on which the
   mutation FAILS the elementwise bar: (a) the eps-mode-0 formula on the sqrt-eps layer, on N-ln-sqrt-first; (b) the rows 1024..1030 left out of
   one dW, on N-w8; (c) a relative error of 1e-3 in the d_ef rows whose cotangent is smallest, on N-log_uniform_edge_cotangents.  For each the
   test prints which of the old bars (1e-3 . max(1, max|ref|), and max(4 . generic error, 1e-5 . max(1, max|ref|)) with the unmutated
   restatement standing in for the generic entry) see it: c passes both, b is seen by both (7 rows of 1031 are 0.7 % of a sum that does not
   cancel).  Where S is the worst-case scale of several levels the bar is looser (the SOUND lines print by how much), which is why the GPU module
   also holds every tensor to the old normwise bar.  Nothing mutated ever runs on a device;
5. the mask: the rule's restatement gives every narrow case's asserted mask on this batch's row counts."""
import numpy as np
import pytest
import torch

from oracle import gn_oracle as O
from tests import bw_x6_cases as BC
from tests import chain_bw_cases as CC
from tests import util as U
from tests.test_bw_x6_stress_cpu import _small_graphs
from tests.chain_torch import _torch_chain_block


def _assert_oracle(val, S, ref, what):
    val, S = CC._drop_none(val), CC._drop_none(S)
    assert set(val) == set(S) == set(ref), (what, sorted(set(val) ^ set(ref)))
    for n in sorted(ref):
        v, s, r = val[n], S[n], np.asarray(ref[n])
        assert v.shape == s.shape == r.shape, (what, n, v.shape, s.shape, r.shape)
        assert (s >= np.abs(v)).all(), f"{what} {n}: a scale below the value"
        assert (np.abs(v - r) <= 1e-11 * s).all(), f"{what} {n}: {float(np.max(np.abs(v - r) / (s + 1e-300))):.3e} of S"


LNS, LN = "ln_sqrt", "ln"
SMALL = [  # (in_dims, edge, node, graph, hidden acts, last acts)
    ((4, 3, 2), [5, LN, 4], [6, LNS, 3], [LNS, 5, 3, LN], (2, 3, 4), (3, 4, 2)),
    ((4, 3, 2), [5, LNS, 4, LN], [LN, 3], [4, 3], (4, 2, 3), (0, 0, 0)),
    ((4, 3, 2), [5, 4], [6, 3], [5, 3], (1, 1, 1), (1, 1, 1)),          # relu hidden and last (random inputs sit far from the kinks in float64)
    ((4, 3, 2), [5, 4], [6, 3], [5, 3], (3, 4, 2), (4, 2, 3)),
    ((0, 3, 2), [5, 4], [], [3], (4, 1, 2), (2, 0, 4)),                  # ef nothing, no node function
    ((4, 0, 0), [5, 3], [4], [], (2, 2, 3), (3, 3, 0)),                  # nf and gf nothing, no graph function
    ((3, 2, 0), [LNS], [LN, 4], [3], (2, 3, 2), None),                   # the edge function IS a LayerNorm
]


@pytest.mark.parametrize("i", range(len(SMALL)))
def test_oracle_equals_float64_autograd_on_small_chains(i):
    in_dims, ew, nw, gw, acts, last = SMALL[i]
    csc = _small_graphs()
    rows = (len(csc[1]), len(csc[0]) - 1, len(csc[2]) - 1)
    rng = np.random.default_rng(300 + i)
    p = O.make_chain_block_params(rng, in_dims, ew, nw, gw, acts=acts, last_acts=last)
    x = tuple(None if v is None else (v * 3 - 1).astype(np.float32) for v in U.packed_inputs(rng, 1, *rows, in_dims))
    outs, souts = O.chain_block_forward_sparse(p, csc, *x, return_scale=True)
    # the forward (both eps modes) against float64 torch
    T = lambda v: None if v is None else torch.tensor(v[0], dtype=torch.float64)
    Tw = lambda v: torch.tensor(v, dtype=torch.float64)
    W = {n: [(w, Tw(b), Tw(a)) if isinstance(w, str) else (Tw(w), Tw(b), a) for w, b, a in p[n]] for n in CC.FN}
    touts, _ = _torch_chain_block(csc, *map(T, x), W)
    for o, s, t in zip(outs, souts, touts):
        assert (o is None) == (t is None or t.shape[1] == 0)
        if o is not None:
            assert (np.abs(o[0] - t.numpy()) <= 1e-11 * s[0]).all()
    cot = tuple(None if o is None else rng.standard_normal(o.shape).astype(np.float32) for o in outs)
    for first_order in (True, False):
        val, S = O.chain_block_backward_sparse(p, csc, x, cot, first_order=first_order)
        _assert_oracle(val, S, CC.torch_chain_grads(p, csc, x, cot, CC.F64), f"small {i} first_order={first_order}")


def test_the_new_parameters_leave_every_seed_its_draws():
    """last_acts and the sqrt-eps token draw nothing: the same seed gives the same numbers with and without them"""
    a = O.make_chain_block_params(np.random.default_rng(3), (10, 5, 3), [16, "ln", 3], [8, 4], ["ln", 6, 5])
    b = O.make_chain_block_params(np.random.default_rng(3), (10, 5, 3), [16, "ln_sqrt", 3], [8, 4], ["ln_sqrt", 6, 5], last_acts=(2, 3, 4))
    for n in CC.FN:
        for (w0, b0, c0), (w1, b1, c1) in zip(a[n], b[n]):
            if isinstance(w0, str):
                assert (w0, w1) == ("layernorm", "layernorm_sqrt_eps") and np.array_equal(b0, b1) and np.array_equal(c0, c1)
            else:
                assert np.array_equal(w0, w1) and np.array_equal(b0, b1)
    assert [l[2] for l in a["edge"] if not isinstance(l[0], str)] == [1, 0] and [l[2] for l in b["edge"] if not isinstance(l[0], str)] == [1, 2]


@pytest.mark.parametrize("cid", CC.CASE_IDS)
def test_oracle_equals_float64_autograd_and_the_bar_is_sound(cid):
    """on every case: the oracle's values; S >= |value|; the first-order S never above the product rule's; plain torch float32 within a quarter of
    1e-5 . S on every element of every gradient (what a kernel misses is the kernel's), and of the forward's outputs"""
    d = CC.data(cid)
    ref, S, yard = CC.reference(cid)
    _assert_oracle(ref, S, CC.torch_chain_grads(d["p"], CC.csc(cid), d["x"], d["cot"], CC.F64), cid)
    _, Sp = O.chain_block_backward_sparse(d["p"], CC.csc(cid), d["x"], d["cot"], first_order=False)
    worst, tight = {}, {}
    for n in sorted(ref):
        assert np.isfinite(ref[n]).all() and np.isfinite(S[n]).all(), (cid, n)
        assert (S[n] <= Sp[n] * (1 + 1e-12)).all(), f"{cid} {n}: the first-order scale above the product rule's"
        (w, _), zeros = BC.ratios(yard[n], ref[n], S[n])
        assert zeros, (cid, n)
        worst[n] = w
        nz = np.abs(ref[n]) > 0
        tight[n] = float(np.median(S[n][nz] / np.abs(ref[n][nz]))) if nz.any() else 0.0
    print(f"SOUND {cid}: worst float32 error / (1e-5 . S) = {max(worst.values()):.4f} ({max(worst, key=worst.get)}); median S / |ref| per tensor "
          f"{min(tight.values()):.3g} .. {max(tight.values()):.3g}")
    assert max(worst.values()) <= 0.25, (cid, {n: round(w, 4) for n, w in worst.items() if w > 0.25})
    # the old normwise bar, asserted on the device as well wherever CC.normwise_applies: plain float32 keeps half of it there, and misses it where not
    for n in sorted(ref):
        r = float(np.abs(yard[n] - ref[n]).max()) / (CC.CHAIN_BAR * max(1.0, float(np.abs(ref[n]).max())))
        assert (r <= 0.5) if CC.normwise_applies(cid, n) else (r > 1.0), (cid, n, r)
    fref, fS = CC.forward_reference(cid)
    T = lambda v, r: None if v is None else torch.tensor(v[r], dtype=torch.float32)
    W = {n: [(w, torch.tensor(b), torch.tensor(a)) if isinstance(w, str) else (torch.tensor(w), torch.tensor(b), a) for w, b, a in d["p"][n]] for n in CC.FN}
    for r in range(d["R"]):
        outs, _ = _torch_chain_block(CC.csc(cid), *(T(v, r) for v in d["x"]), W)
        for n, o in zip(CC.FW, outs):
            if fref[n] is None:
                continue
            (w, _), zeros = BC.ratios(o.double().numpy(), fref[n][r], fS[n][r])
            assert zeros and w <= 0.25, (cid, n, w)


def test_cancelling_cases_cancel():
    for cid in ("N-cancelling_dW", "W-cancelling_dW"):
        ref, S, _ = CC.reference(cid)
        assert np.median(S["edge0.dW"] / (np.abs(ref["edge0.dW"]) + 1e-300)) >= 1e4, cid


def test_relu_case_is_kink_free_and_relu_is_nowhere_else():
    d = CC.data("N-relu")
    assert not any(b.any() for b in CC.relu_kink_rows(d["p"], CC.csc("N-relu"), [v[0] for v in d["x"]]))
    for cid in CC.CASE_IDS:
        has = any(a == O.ACT_RELU for fa in CC.acts_of(cid) for a in fa)
        assert has == (cid == "N-relu"), cid


def test_masks_are_the_rules():
    assert all(CC.want_mask(c) == 7 for c in CC.NARROW_IDS if c not in ("N-mixed", "N-ln-sqrt-first")) and CC.want_mask("N-ln-sqrt-first") == 1
    for cid in CC.NARROW_IDS:
        assert CC.want_mask(cid) == CC.formula_mask(cid), cid
    assert CC.formula_mask("N-mixed") == 2
    assert all(CC.formula_mask(c) == 0 for c in CC.CASE_IDS if CC.CASE[c]["family"] == "wide")
    for cid in CC.NARROW_IDS:
        if CC.want_mask(cid) == 7:
            must, must_not, kernels = CC.expected_scopes(cid, "narrow")
            assert kernels == {"bw_delta": 2, "bw_delta_edge": 1} and {"bw_dx_chain", "bw_layernorm", "bw_gelu_preact"} <= must_not
    for cid, want in (("W-plain", {"bw_dx_chain", "k_dw_gemm", "bw_layernorm"}), ("W-tails", {"bw_dx_chain", "k_dw_gemm", "bw_layernorm"}),
                      ("W-gelu-last-act", {"bw_dx_chain", "k_dw_gemm", "bw_gelu_preact"})):
        must, must_not, _ = CC.expected_scopes(cid, "generic")
        assert want <= must and not (must & must_not), (cid, must, must_not)
    assert "bw_layernorm" in CC.expected_scopes("W-gelu-last-act", "generic")[1] and "bw_gelu_preact" in CC.expected_scopes("W-plain", "generic")[1]


def test_library_gives_every_case_its_mask():
    """gnx_chain_block_backward_narrow_applies on a fake handle with the batch's counts (no table is read) and the cases' widths, LayerNorm kinds
    (the sqrt-eps bit included) and activations (on last layers too): the asserted masks; the forward's rule takes what the backward's takes"""
    import ctypes as C
    import __graft_entry__ as ge
    from tests.test_chain_narrow_abi import _fake_handle, _params
    ge.build()
    import graphnets_jl_amd as gn
    L, lib = gn._lib, gn._lib.load()
    for cid in CC.CASE_IDS:
        E, N, G = CC.rows(cid)
        shape = CC.shape(cid)
        cp, _keep = _params(gn, in_dims=CC.CASE[cid]["in_dims"], widths=tuple(tuple(l[0] for l in layers) for _, layers in shape))
        for ch, (_, layers), acts in zip((cp.edgefn, cp.nodefn, cp.graphfn), shape, CC.acts_of(cid)):
            for i, ((J, K, kind), act) in enumerate(zip(layers, acts)):
                ch.layers[i].kind = {"dense": 0, "ln": L.LAYER_LAYERNORM, "ln_sqrt": L.LAYER_LAYERNORM | L.LAYER_LN_SQRT_EPS}[kind]
                ch.layers[i].act = 0 if act is None else act
        hbuf = _fake_handle(G=G, N=N, E=E)
        fake = C.c_void_p(hbuf.ctypes.data)
        R = CC.CASE[cid]["R"]
        bw = lib.gnx_chain_block_backward_narrow_applies(fake, C.byref(cp), R)
        assert bw == CC.want_mask(cid), (cid, bw, lib.gnx_last_error())
        assert lib.gnx_chain_block_forward_narrow_applies(fake, C.byref(cp), R) & bw == bw, cid


# ---------------------------------------------------------------------------------------------------------------------------------------
# controls: the fused kernel's per-row arithmetic in numpy float32, and three mutations of it
# ---------------------------------------------------------------------------------------------------------------------------------------
f32 = np.float32
EPS = f32(1e-5)


def _gelu32(z):
    c, a = f32(np.sqrt(2.0 / np.pi)), f32(0.044715)
    t = np.tanh(c * (z + a * z * z * z))
    return f32(0.5) * z * (f32(1) + t), t


def _act32(z, act):
    if act == 0:
        return z
    if act == 1:
        return np.maximum(z, f32(0))
    if act == 2:
        return np.tanh(z)
    if act == 3:
        return f32(1) / (f32(1) + np.exp(-z))
    return _gelu32(z)[0]


def _act_grad32(v, act):
    """act' from the layer's output (gelu: from its pre-activation), act_grad_bw's formulas"""
    if act == 0:
        return np.ones_like(v)
    if act == 1:
        return (v > 0).astype(f32)
    if act == 2:
        return f32(1) - v * v
    if act == 3:
        return v * (f32(1) - v)
    c, a = f32(np.sqrt(2.0 / np.pi)), f32(0.044715)
    _, t = _gelu32(v)
    return f32(0.5) * (f32(1) + t) + f32(0.5) * v * (f32(1) - t * t) * c * (f32(1) + f32(3) * a * v * v)


def _chunk_sum(A, B, drop=None):
    """A^T B (B None: column sums of A) in float32, one partial per 64-row chunk, the partials added in order; `drop`: rows left out"""
    tot = None
    for c0 in range(0, A.shape[0], 64):
        a = A[c0:c0 + 64]
        b = None if B is None else B[c0:c0 + 64]
        if drop is not None:
            keep = ~np.isin(np.arange(c0, c0 + a.shape[0]), drop)
            a, b = a[keep], (None if b is None else b[keep])
        part = a.sum(axis=0, dtype=f32) if b is None else a.T @ b
        tot = part if tot is None else tot + part
    return tot


def _chain32(layers, X, g_of, mode0_everywhere=False, drop=None):
    """one Chain on rows in float32: forward, `g_of(output)` -> the cotangent of the output, then back.  Returns (output, dX, [(dW, db)])"""
    tape, x = [], X
    for W, b, act in layers:
        if isinstance(W, str):
            mode = 0 if mode0_everywhere else O.ln_eps_mode(W)
            mu = x.mean(axis=1, keepdims=True, dtype=f32)
            c = x - mu
            v = (c * c).mean(axis=1, keepdims=True, dtype=f32)
            sden = np.sqrt(v) + EPS if mode == 0 else np.sqrt(v + EPS)
            y = c / sden * b + act
            tape.append((x, None, y))
        else:
            z = x @ W.T + b
            y = _act32(z, act)
            tape.append((x, z, y))
        x = y
    out, grads = x, [None] * len(layers)
    g = g_of(out)
    for i in range(len(layers) - 1, -1, -1):
        W, b, act = layers[i]
        xin, z, y = tape[i]
        dr = drop.get(i) if drop else None
        if isinstance(W, str):
            mode = 0 if mode0_everywhere else O.ln_eps_mode(W)
            width = f32(xin.shape[1])
            mu = xin.mean(axis=1, keepdims=True, dtype=f32)
            c = xin - mu
            v = (c * c).mean(axis=1, keepdims=True, dtype=f32)
            sigma = np.sqrt(v)
            sden = sigma + EPS if mode == 0 else np.sqrt(v + EPS)
            q = sigma * sden * sden if mode == 0 else sden * sden * sden
            dxh = g * b
            with np.errstate(divide="ignore", invalid="ignore"):
                coef = np.where(q > 0, (dxh * c).sum(axis=1, keepdims=True, dtype=f32) / (width * q), f32(0))  # (the kernel's guard)
            grads[i] = (_chunk_sum(g * (c / sden), None, dr), _chunk_sum(g, None, dr))
            g = (dxh - dxh.mean(axis=1, keepdims=True, dtype=f32)) / sden - c * coef
        else:
            d = g * _act_grad32(z if act == 4 else y, act)
            grads[i] = (_chunk_sum(xin, d, dr), _chunk_sum(d, None, dr))
            g = d @ W
    return out, g, grads


def narrow_restatement(cid, mode0_everywhere=False, drop=None):
    """every gradient of a one-replica case as the fused call forms it, in numpy float32; `drop`: {(function, layer): rows left out of its dW}"""
    d = CC.data(cid)
    assert d["R"] == 1
    p = {n: [tuple(np.asarray(v, dtype=f32) if not isinstance(v, (str, int)) else v for v in l) for l in d["p"][n]] for n in CC.FN}
    colptr, rowval, node_off, edge_off = CC.csc(cid)
    N, E, G = len(colptr) - 1, len(rowval), len(node_off) - 1
    dst = np.repeat(np.arange(N), np.diff(colptr))
    ng, eg = np.repeat(np.arange(G), np.diff(node_off)), np.repeat(np.arange(G), np.diff(edge_off))
    de, dn, dg = d["p"]["in_dims"]
    z0 = lambda v, T: np.zeros((T, 0), dtype=f32) if v is None else v[0]
    ef, nf, gf = (z0(v, T) for v, T in zip(d["x"], (E, N, G)))
    ce, cn, cg = (z0(v, T) for v, T in zip(d["cot"], (E, N, G)))
    seg = lambda v, idx, n: O._segsum(v, idx, n).astype(f32)
    dr = lambda name: {i: rows for (fn, i), rows in (drop or {}).items() if fn == name}
    cat = lambda parts: np.concatenate(parts, axis=1)

    def chain(name, X, g_of, T):  # (a function without layers: a zero-width output, no gradient into its input)
        if not p[name]:
            return np.zeros((T, 0), dtype=f32), np.zeros_like(X), []
        return _chain32(p[name], X, g_of, mode0_everywhere, dr(name))

    # forward of the lower levels (the call runs them again), then the three pullbacks top down
    zero = lambda o: np.zeros_like(o)
    he, _, _ = chain("edge", cat([ef, nf[rowval], nf[dst], gf[eg]]), zero, E)
    hn, _, _ = chain("node", cat([seg(he, dst, N), nf, gf[ng]]), zero, N)
    oe, on = he.shape[1], hn.shape[1]
    _, dXg, gg = chain("graph", cat([seg(he, eg, G), seg(hn, ng, G), gf]), lambda o: cg, G)
    _, dXn, gn_ = chain("node", cat([seg(he, dst, N), nf, gf[ng]]), lambda o: cn + dXg[ng][:, oe:oe + on], N)
    _, dXe, ge = chain("edge", cat([ef, nf[rowval], nf[dst], gf[eg]]), lambda o: ce + dXg[eg][:, :oe] + dXn[dst][:, :oe], E)
    out = {"d_ef": dXe[None, :, :de],
           "d_nf": (seg(dXe[:, de:de + dn], rowval, N) + seg(dXe[:, de + dn:de + 2 * dn], dst, N) + dXn[:, oe:oe + dn])[None],
           "d_gf": (seg(dXe[:, de + 2 * dn:], eg, G) + seg(dXn[:, oe + dn:], ng, G) + dXg[:, oe + on:])[None]}
    out = {n: v for n, v, w in zip(CC.DX, out.values(), (de, dn, dg)) if w}
    for name, gr in zip(CC.FN, (ge, gn_, gg)):
        for i, (dW, db) in enumerate(gr):
            out[f"{name}{i}.dW"], out[f"{name}{i}.db"] = dW, db
    return out


def _verdicts(cid, got, base):
    """which checks see `got`: the elementwise bar, the statistical criterion, the old normwise bar, the old narrow-against-generic rule (the
    unmutated restatement `base` standing in for the generic entry) — each a sorted list of the tensors that FAIL it"""
    ref, S, yard = CC.reference(cid)
    fails = dict(elementwise=[], statistical=[], legacy_1e3=[], narrow_rule=[])
    worst = 0.0
    for n in sorted(ref):
        (w, m), zeros = BC.ratios(got[n], ref[n], S[n])
        worst = max(worst, w)
        if w > 1.0 or not zeros:
            fails["elementwise"].append(n)
        (_, ym), _ = BC.ratios(yard[n], ref[n], S[n])
        if ref[n].size >= BC.MIN_STAT and m > BC.K_MEAN * ym:
            fails["statistical"].append(n)
        if not BC.legacy_close(got[n], ref[n], CC.CHAIN_BAR):
            fails["legacy_1e3"].append(n)
        en, eg = float(np.abs(got[n] - ref[n]).max()), float(np.abs(np.asarray(base[n], dtype=np.float64) - ref[n]).max())
        if en > max(4.0 * eg, 1e-5 * max(1.0, float(np.abs(ref[n]).max()))):
            fails["narrow_rule"].append(n)
    return fails, worst


CONTROLS = {}


@pytest.mark.parametrize("cid", ["N-w8", "N-ln-both-modes", "N-log_uniform_inputs", "N-log_uniform_cotangents", "N-gelu-hidden", "N-last-act", "N-log_uniform_edge_cotangents",
                                 "N-ln-sqrt-first"])
def test_the_restatement_passes_as_it_stands(cid):
    ref, S, yard = CC.reference(cid)
    got = narrow_restatement(cid)
    assert set(got) == set(ref)
    for n in sorted(ref):
        w, m = BC.check_elementwise(got[n], ref[n], S[n], f"{cid} {n}")
        (_, ym), _ = BC.ratios(yard[n], ref[n], S[n])
        BC.check_statistical(m, ym, ref[n].size, f"{cid} {n}")


def _record(name, cid, fails, worst):
    CONTROLS[name] = (cid, fails, worst)
    print(f"CONTROL {name} on {cid}: worst |got - ref| / (1e-5 . S) = {worst:.3g}; fails elementwise {fails['elementwise']}, statistical "
          f"{fails['statistical']}, old bar 1e-3 . max {fails['legacy_1e3']}, old narrow rule {fails['narrow_rule']}")


def _elementwise_failures(cid, got):
    ref, S, _ = CC.reference(cid)
    bad = []
    for n in sorted(ref):
        try:
            BC.check_elementwise(got[n], ref[n], S[n], n)
        except AssertionError as e:
            assert "worst" in str(e), e
            bad.append(n)
    return bad


def test_control_a_eps_mode_0_formula_on_a_sqrt_eps_layer():
    """N-ln-sqrt-first: three log-uniform features per edge, so some rows have a deviation below sqrt(eps), where (x - mean) / (sigma + eps) and
    (x - mean) / sqrt(sigma^2 + eps) differ by a factor; the LayerNorm's inputs and the cotangents of the layer behind it are handed to the call, so
    S is the scale of one LayerNorm and one Dense"""
    cid = "N-ln-sqrt-first"
    base = narrow_restatement(cid)
    got = narrow_restatement(cid, mode0_everywhere=True)
    fails, worst = _verdicts(cid, got, base)
    _record("a", cid, fails, worst)
    assert _elementwise_failures(cid, got) == fails["elementwise"] and fails["elementwise"], "the eps-mode-0 formula on a sqrt-eps layer passed the elementwise bar"
    assert {"edge0.dW", "edge1.dW", "d_ef"} & set(fails["elementwise"])  # the LayerNorm's gamma gradient, the weight gradient behind it, its dx


def test_control_b_the_last_partial_chunk_left_out_of_one_dW():
    """N-w8: the rows 1024..1030 of the node level (its 17th chunk of 64 rows, 7 rows long) left out of the node function's weight gradient.  The old
    bars see this one as well: 7 rows of 1031 are 0.7 % of a sum that does not cancel, above 1e-3"""
    cid = "N-w8"
    base = narrow_restatement(cid)
    got = narrow_restatement(cid, drop={("node", 0): np.arange(1024, 1031)})
    assert not np.array_equal(got["node0.dW"], base["node0.dW"]) and all(np.array_equal(got[n], base[n]) for n in got if not n.startswith("node0"))
    fails, worst = _verdicts(cid, got, base)
    _record("b", cid, fails, worst)
    assert _elementwise_failures(cid, got) == fails["elementwise"] and "node0.dW" in fails["elementwise"] and worst > 100


def test_control_c_a_relative_error_of_1e3_in_the_rows_of_the_smallest_cotangent():
    """N-log_uniform_edge_cotangents: d_ef of the 64 edges whose cotangent row is smallest, off by 1e-3 of its value.  Both old bars pass it: the
    rows are many decades below the tensor's largest"""
    cid = "N-log_uniform_edge_cotangents"
    base = narrow_restatement(cid)
    cot = np.abs(CC.data(cid)["cot"][0][0]).max(axis=1)
    rows = np.argsort(cot)[:64]
    got = {n: np.array(v, dtype=np.float64) for n, v in base.items()}
    got["d_ef"][0, rows] *= 1 + 1e-3
    fails, worst = _verdicts(cid, got, base)
    _record("c", cid, fails, worst)
    assert _elementwise_failures(cid, got) == ["d_ef"] == fails["elementwise"]
    assert not fails["legacy_1e3"] and not fails["narrow_rule"], "both old bars were expected to pass this mutation"
