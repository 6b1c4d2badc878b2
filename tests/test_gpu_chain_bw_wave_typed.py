"""gnx_chain_block_backward_wave_typed: the wave-per-tile Chain pullback on bfloat16 features (csrc/gnx_chain_bw_wave_bf16.hip).  Inside the
rule the three input gradients are bit for bit to_bf16 of gnx_chain_block_backward_wave's on the widened tensors and every parameter gradient is
that call's bits; outside it every output is gnx_chain_block_backward_narrow_typed's bytes.  The cases, batches and tile kinds are those of
tests/test_gpu_chain_bw_wave.py; the calls go through tests/test_gpu_chain_bw_native.py's NCall with the library's narrow names mapped to the
wave ones (WaveLib: NCall.nrun / napplies / nquery then reach the new entry, TCall.brun(1, plain=True) the fp32 wave entry)."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests import arena as AR
from tests import test_gpu_chain_bw_native as NB
from tests import test_gpu_chain_bw_wave as BWW
from tests import test_gpu_chain_narrow as CN
from tests import test_gpu_chain_typed as TY
from tests import test_gpu_chain_wave as TW
from tests.chain_torch import _torch_chain_block
from tests.test_gpu_chain_narrow import _adjs, gn  # noqa: F401  (gn: the module's fixture)
from tests.test_gpu_memory_contract import _chain_params, _decl, _decl_chains, _decl_dense_grad, _dense_grad

pytestmark = pytest.mark.gpu
CASES = BWW.CASES
ODD = ((3, 1, 1), [5, 3], [3], [3], None, None)  # every width odd: with odd E and N every row and every replica starts on a 2-byte boundary
IDS = [str(c[:4]) for c in CASES]


def wave(c, f):
    """f() with the wave entries under the narrow entries' names"""
    lib, c.lib = c.lib, BWW.WaveLib(c.lib)
    try:
        return f()
    finally:
        c.lib = lib


def call(gn, adjs, case, R=1, seed=0):
    """an NCall on the parameters of tests/test_gpu_chain_bw_wave.py's draw of the case"""
    return NB.NCall(gn, adjs, BWW.make(gn, adjs, case, R, seed).p, R, seed)


def rounded(ref):
    import torch
    return {n: t.to(torch.bfloat16) if n.startswith("d_") else t for n, t in ref.items()}


def same(a, b):
    return sorted(a) == sorted(b) and all(TY._same(a[n], b[n]) for n in a)


def verify(c, inside, what, **kw):
    """`_applies`; NaN-filled outputs fully written; the same bytes on a 0x00 and a 0xA5 workspace; inside the rule to_bf16 of the fp32 wave
    entry's input gradients and its parameter gradients' bits, outside the narrow typed entry's bytes and workspace size"""
    import torch
    assert wave(c, c.napplies) == int(inside), what
    (a, na), (b, _) = wave(c, lambda: c.nrun(fill=0x00, **kw)), wave(c, lambda: c.nrun(fill=0xA5, **kw))
    assert all(not bool(torch.isnan(t.float()).any()) for t in a.values()), f"{what}: an output keeps NaN"
    assert same(a, b), f"{what}: the bytes depend on what the workspace held"
    if inside:
        ref, _ = wave(c, lambda: c.brun(1, plain=True, **{k: v for k, v in kw.items() if k in ("skip", "no_cot")}))
        assert c.napplies(c.L.ELEM_F32) == 0 and wave(c, lambda: c.napplies(c.L.ELEM_F32)) == 1
        assert same(a, rounded(ref)), f"{what}: {[n for n in a if not TY._same(a[n], rounded(ref)[n])]} differ from the fp32 wave pullback, rounded"
    else:
        ref, nr = c.nrun(**kw)
        assert na == nr and same(a, ref), f"{what}: outside the rule the call is not gnx_chain_block_backward_narrow_typed"
    return a


# ---- 1. bits ----
@pytest.mark.parametrize("graphs", [5, 1])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_bits(gn, i, graphs):
    rng = np.random.default_rng(100 + i)
    case = CASES[i]
    c = call(gn, _adjs(rng) if graphs == 5 else _adjs(rng, [40]), case, seed=i)
    verify(c, inside=graphs == 1 or not (TW.wide(case) or BWW.narrow8(case)), what=str(case[:4]))  # (the two inherited cuts: 32 or 8 on five graphs)


# ---- 2. against float64 ----
def f64(c):
    """float64 autograd on the widened bf16 inputs and cotangents (R = 1): ({name: gradient}, no relu pre-activation within 5e-6 of its kink)"""
    import torch
    csc = (*c.g.csc(), c.g.node_off, c.g.edge_off)
    T = lambda v: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True)
    W = {name: [(w, T(b), T(q)) if isinstance(w, str) else (T(w), T(b), q) for w, b, q in c.p[name]] for name in ("edge", "node", "graph")}
    xs = [None if t is None else t[0].double().cpu().requires_grad_(True) for t in c.xt]
    outs, pre = _torch_chain_block(csc, *xs, W)
    ok = not any(a == 1 and float(z.detach().abs().min()) < 5e-6 for z, a in pre if z.numel())
    sum((o * ct[0].double().cpu()).sum() for o, ct in zip(outs, c.cw) if o is not None).backward()
    g = lambda q: np.zeros(tuple(q.shape)) if q.grad is None else q.grad.numpy()
    ref = {n: g(x)[None] for n, x in zip(("d_ef", "d_nf", "d_gf"), xs) if x is not None}
    for name in ("edge", "node", "graph"):
        for k, (w, b, q) in enumerate(W[name]):
            ref[f"{name}{k}.dW"], ref[f"{name}{k}.db"] = (g(b), g(q)) if isinstance(w, str) else (g(w).T, g(b))
    return ref, ok


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_float64_autograd(gn, i):
    """max|got - ref| <= max(4 max|yardstick - ref|, 1e-5 max(1, max|ref|)) per tensor; the yardstick is gnx_chain_block_backward_typed(narrow = 1)
    on the same nine bf16 tensors"""
    adjs = _adjs(np.random.default_rng(100 + i), [40])
    for attempt in range(20):
        c = call(gn, adjs, CASES[i], seed=i + 1000 * attempt)
        ref, ok = f64(c)
        if ok:
            break
    assert ok, "no kink-free draw in 20 attempts"
    assert wave(c, c.napplies) == 1
    got, _ = wave(c, c.nrun)
    yard, _ = c.brun(1)
    for n, r in ref.items():
        if r.size:
            en = float(np.max(np.abs(got[n].float().cpu().numpy().astype(np.float64).reshape(r.shape) - r)))
            ey = float(np.max(np.abs(yard[n].float().cpu().numpy().astype(np.float64).reshape(r.shape) - r)))
            bound = max(4.0 * ey, 1e-5 * max(1.0, float(np.abs(r).max())))
            print(f"chain bw wave bf16 {CASES[i][:4]} {n}: err {en:.3e}, yardstick err {ey:.3e}, bound {bound:.3e}")
            assert np.isfinite(en) and en <= bound, (n, en, ey, bound)


# ---- 3. tiles ----
@pytest.mark.parametrize("kind", ["node-and-edge-cap", "empty-columns", "degree-cap", "degree-cap+1", "replicas-3"])
def test_tiles(gn, kind):
    rng = np.random.default_rng(200)
    adjs, R, inside = TW._tiles(kind, rng)
    c = call(gn, adjs, CASES[2] if len(adjs) == 1 else CASES[1], R, seed=20)  # (one graph: the 32-wide instantiation)
    if kind.startswith("degree-cap"):
        assert c.g.max_in_degree == TW.CAP + (not inside)
    if kind == "node-and-edge-cap":  # a tile of 64 one-in-edge nodes, tiles of two edge chunks with a partly live second one
        assert c.g.n_edges > 64 + TW.CAP
    verify(c, inside, kind)


def test_odd_widths_on_exact_buffers(gn):
    """every width odd at R = 3 on one graph of an odd number of nodes and edges: every buffer carved at its exact size from the sentinel arena,
    4-byte aligned only; nothing but the outputs and the workspace is written, the inputs are untouched, the bits are the heap call's"""
    import torch
    L, lib = gn._lib, gn._lib.load()
    _, adjs, R = TY._structural("odd-everything-replicas-3", np.random.default_rng(500))
    src = call(gn, adjs, ODD, R, seed=50)
    p, g, BF = src.p, src.g, L.ELEM_BF16
    assert R == 3 and g.n_edges % 2 == 1 and g.n_nodes % 2 == 1 and g.n_graphs == 1 and wave(src, src.napplies) == 1
    want = verify(src, True, "odd")
    a = AR.Arena("cuda", skew=lambda c: 0 if c.kind == AR.WORKSPACE else 4)
    _decl_chains(a, p)
    ins = [_decl(a, n, v) for n, v in zip(("ef", "nf", "gf"), src.xb)]
    gs = [_decl(a, n, v) for n, v in zip(("g_ef_out", "g_nf_out", "g_gf_out"), src.cb)]
    dx = [a.output(n, v.shape, torch.bfloat16) for n, v in zip(("d_ef", "d_nf", "d_gf"), src.xb)]
    for name in ("edge", "node", "graph"):
        for k, (w, b, c) in enumerate(p[name]):
            _decl_dense_grad(a, f"grad.{name}{k}", w, b)
    keep = []
    ws = a.workspace("ws", lambda: lib.gnx_chain_block_backward_wave_typed_workspace_bytes(g._h, C.byref(_chain_params(gn, a, p, keep)), R, BF))
    a.build(ws_fill=0xA5)
    assert a.nbytes(ws) == wave(src, src.nquery) > 0, lib.gnx_last_error()
    assert all((a.ptr(n) + 2 * v.shape[1] * v.shape[2]) % 4 == 2 for n, v in zip(ins + gs, src.xb + src.cb))  # replica 1 starts 2-byte aligned
    arrays = []
    for name in ("edge", "node", "graph"):
        arr = (L.DenseGrad * len(p[name]))(*[_dense_grad(gn, a, f"grad.{name}{k}") for k in range(len(p[name]))])
        arrays.append(arr)
    gr = L.ChainBlockGrads(*[C.cast(x_, C.POINTER(L.DenseGrad)) for x_ in arrays])
    P = a.ptr
    rc = lib.gnx_chain_block_backward_wave_typed(g._h, C.byref(_chain_params(gn, a, p, keep)), BF, *map(P, ins), *map(P, gs), R, *map(P, dx), C.byref(gr),
                                                 P(ws), a.nbytes(ws), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.gnx_last_error()
    a.check("wave typed pullback, odd widths")
    for n in dx:
        assert torch.equal(a.view(n).reshape(-1).view(torch.int16), want[n].view(torch.int16)), n


# ---- 4. NULLs ----
def test_null_outputs(gn):
    """d_nf and one layer's gradient pair not wanted, no upstream gradient of gf': the fp32 wave entry under the same NULLs, rounded"""
    c = call(gn, _adjs(np.random.default_rng(300)), CASES[1], seed=30)
    skip = {"d_nf", "edge1.dW", "edge1.db"}
    a = verify(c, True, "NULLs", skip=skip, no_cot=(2,))
    assert not skip & set(a) and "d_ef" in a and "edge0.dW" in a


# ---- 5. the wave form ran ----
def test_the_wave_form_ran(gn):
    c = call(gn, _adjs(np.random.default_rng(600)), CASES[1], seed=60)
    assert wave(c, c.napplies) == 1
    prof = CN._profiled(gn, lambda: wave(c, c.nrun))
    count = lambda name: prof[name]["kernels"] if name in prof else 0
    names = NB.PROFILE_NAMES | {"bw_chain_fw_g"}  # (the wave form's graph rows; every name has its case in tests/test_gpu_memory_contract.py)
    assert set(prof) <= names, sorted(set(prof) - names)
    assert count("k_bf16_widen") <= 1 and count("k_bf16_round") <= 1 and count("bw_chain_fw_n") == 0 and count("bw_delta_edge") == 1, prof
    up256 = lambda x: -(-x // 256) * 256
    fp32 = c.lib.gnx_chain_block_backward_wave_workspace_bytes(c.g._h, C.byref(c.cp), c.R)
    assert 0 < fp32 <= wave(c, c.nquery) <= fp32 + 2 * up256(4 * c.R * c.rows[2] * c.p["in_dims"][2]) + 256, (fp32, wave(c, c.nquery))


# ---- 6. capture ----
def test_a_captured_call_replays_the_eager_bits(gn):
    import torch
    c = call(gn, _adjs(np.random.default_rng(700)), CASES[1], seed=70)
    assert wave(c, c.napplies) == 1
    ws = torch.zeros((wave(c, c.nquery),), dtype=torch.uint8, device=c.g.device)  # (the query builds the tables the call reads, outside the capture)
    eager, _ = wave(c, lambda: c.nrun(ws=ws))
    graphed = c.grads(True)
    side = torch.cuda.Stream()
    cg = torch.cuda.CUDAGraph()
    gc.collect()  # nothing may free device memory while the capture is open
    gc.disable()
    try:
        with torch.cuda.stream(side):
            with torch.cuda.graph(cg, stream=side):
                wave(c, lambda: c.nrun(outs=graphed, ws=ws, stream=side.cuda_stream, sync=False))
    finally:
        gc.enable()
    for _ in range(3):
        for t in graphed.values():
            t.zero_()
        ws.fill_(0x5A)
        cg.replay()
        torch.cuda.synchronize()
        assert same(eager, graphed)


# ---- 7. Python ----
def test_python_switch(gn):
    """GNBlock(..., bf16_chain, bf16_backward, wave_chain_backward) under torch.autograd gives the entry's bytes; with the switch off, the bytes
    of the entry the other switches select"""
    import torch
    c = call(gn, _adjs(np.random.default_rng(400)), CASES[1], seed=40)
    blk = c.blk
    blk.bf16_chain = blk.bf16_backward = blk.native_chain_backward = blk.narrow_chain_backward = True
    leaves = [(l.weight.requires_grad_(True), l.bias.requires_grad_(True)) for ch in (blk.edgefn, blk.nodefn, blk.graphfn) for l in ch.layers]
    names = [f"{name}{i}" for name in ("edge", "node", "graph") for i in range(len(c.p[name]))]
    eq = lambda u, v: torch.equal(TY._bits(u).reshape(-1), TY._bits(v).reshape(-1))
    for on, (want, _) in ((True, wave(c, c.nrun)), (False, c.nrun())):
        blk.wave_chain_backward = on  # (wins over native_chain_backward and narrow_chain_backward)
        for w, b in leaves:
            w.grad = b.grad = None
        xt = [t.clone().requires_grad_(True) for t in c.xb]
        y = blk(TY._nt(gn, c, xt))
        sum((o.permute(2, 1, 0).float() * ct.float()).sum() for o, ct in zip((y.ef, y.nf, y.gf), c.cb)).backward()
        torch.cuda.synchronize()
        assert all(t.grad.dtype == torch.bfloat16 and eq(t.grad, want[n]) for n, t in zip(("d_ef", "d_nf", "d_gf"), xt)), on
        for n, (w, b) in zip(names, leaves):
            assert eq(w.grad if w.grad.dim() == 1 else w.grad.t(), want[n + ".dW"]) and eq(b.grad, want[n + ".db"]), (on, n)
