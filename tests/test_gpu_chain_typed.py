"""gnx_chain_block_forward_typed / gnx_chain_block_backward_typed: a GNBlock whose update functions are Chains on bfloat16 features.  Every
comparison is exact: the bf16 outputs are the bits of to_bf16(the mirrored fp32 entry on the exactly widened inputs) — on the native path (each
narrow update function in one kernel that reads and writes bf16 rows, csrc/gnx_chain_narrow_bf16.hip), on the staged paths and in the pullback;
GNX_ELEM_F32 is the fp32 entry itself.  Also: that the native form ran, the memory contract on exactly sized 4-byte-aligned buffers, stream
capture, the Python switch and a seeded sweep.  The batches, width cases and structural cases are those of tests/test_gpu_chain_narrow.py,
restated, plus the cases a 16-bit load can get wrong (odd widths and row counts under replicas; an odd dg on an odd number of graphs)."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

from oracle import gn_oracle as O
from tests import arena as AR
from tests import util as U
from tests import test_gpu_chain_narrow as CN
from tests.test_gpu_memory_contract import _chain_out_widths, _chain_params, _decl, _decl_chains, _decl_dense_grad, _decl_outputs, _dense_grad

pytestmark = pytest.mark.gpu
EXTRA = int(os.environ.get("GNX_FUZZ_EXTRA", "0"))
NAMES = ("k_rows_gemm_chain_e", "k_rows_gemm_chain_n", "k_rows_gemm_chain_g")

WIDTH_CASES = [
    ((10, 5, 0), [16, 3], [8, 4], [6, 5], None),                                         # gf nothing
    ((2, 2, 1), [8, 8, 1], [3], [2], None),                                              # all widths <= 8
    ((3, 2, 1), [9, 17, 4], [16, "ln", 5], ["ln", 9, 4, "ln"], (4, 3, 1)),               # gelu, sigmoid, relu; the 16 / 32 buckets by one
    ((8, 8, 8), [32, "ln", 32, 32, 7], ["ln", 32, 32, 9], [32, "ln", 17, 4], (1, 2, 0)),  # K_e = 32, layer widths up to 32
    ((0, 4, 2), [8, 5], [5], [], None),                                                  # ef nothing, no graph output
    ((6, 0, 0), [4, 3], [], [], None),                                                   # edge function only
    ((10, 5, 3), ["ln", 12, 7], [6], [4], None),                                         # LayerNorm as the edge function's first layer
    ((3, 2, 1), [8] * 8, [8, 8, 8], [8, 8], None),                                       # long chains
    ((4, 2, 3), [8, 3], [4], [5], None),                                                 # dg odd on G = 5 graphs: gf rows at 2-byte boundaries
]
ODD_CASE = ((3, 5, 1), [9, 3], [7, 5], [3], None)  # odd de, dn, oe, on: under replicas every bf16 tensor's replicas 1 and 2 start 2-byte aligned
STRUCTURAL = ["isolated-column", "graph-without-edges", "partial-workgroup", "edgeless-batch", "replicas-2", "replicas-3", "odd-everything-replicas-3"]


def _structural(kind, rng):
    """(case, adjacency matrices, R)"""
    if kind == "odd-everything-replicas-3":  # one graph with an odd number of nodes and of edges
        a = (rng.random((31, 31)) < 0.3).astype(np.int64)
        if int(a.sum()) % 2 == 0:
            a[0, 0] ^= 1
        assert a.shape[0] % 2 == 1 and int(a.sum()) % 2 == 1
        return ODD_CASE, [a], 3
    adjs, R = CN._structural(kind, rng)
    return WIDTH_CASES[3 if kind == "partial-workgroup" else 0], adjs, R


@pytest.fixture(scope="module")
def gn():
    import torch
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(u, v):
    import torch
    return u.dtype == v.dtype and u.shape == v.shape and torch.equal(_bits(u), _bits(v))


class TCall(CN.Call):
    """CN.Call on bfloat16 features: `xb` the bf16 inputs, `xt` (what CN.Call.run reads) their exact fp32 widening, bf16 cotangents `cb` and their
    widening `cw`; the typed entries on workspaces of exactly the queried size"""

    def __init__(self, gn, adjs, p, R=1, seed=0):
        import torch
        super().__init__(gn, adjs, p, R, seed)
        BF = torch.bfloat16
        self.xb = [None if t is None else t.to(BF) for t in self.xt]
        self.xt = [None if t is None else t.float() for t in self.xb]
        self.rows = (self.g.n_edges, self.g.n_nodes, self.g.n_graphs)
        gen = torch.Generator(device="cpu").manual_seed(4000 + seed)
        self.cb = [torch.randn((R, T, d), generator=gen).to(BF).to(self.g.device) if d > 0 else None for T, d in zip(self.rows, self.outw)]
        self.cw = [None if t is None else t.float() for t in self.cb]

    # ---- forward ----
    def native(self):
        return self.lib.gnx_chain_block_forward_typed_applies(self.g._h, C.byref(self.cp), self.R, self.L.ELEM_BF16, 1)

    def want_native(self):
        """every function with output and rows is in gnx_chain_block_forward_narrow_applies' mask"""
        m = self.mask()
        return int(all(m >> t & 1 for t in range(3) if self.outw[t] > 0 and self.rows[t] > 0))

    def tquery(self, narrow=1, elem=None):
        return self.lib.gnx_chain_block_forward_typed_workspace_bytes(self.g._h, C.byref(self.cp), self.R, self.L.ELEM_BF16 if elem is None else elem, narrow)

    def touts(self, dtype=None):
        import torch
        dtype = torch.bfloat16 if dtype is None else dtype
        return [torch.full((self.R, T, d), float("nan"), dtype=dtype, device=self.g.device) if d > 0 else None for T, d in zip(self.rows, self.outw)]

    def trun(self, narrow=1, elem=None, outs=None, ws=None, fill=0xA5, stream=None, nbytes=None):
        import torch
        elem = self.L.ELEM_BF16 if elem is None else elem
        bf16 = elem == self.L.ELEM_BF16
        nbytes = self.tquery(narrow, elem) if nbytes is None else nbytes
        assert nbytes > 0, self.lib.gnx_last_error()
        if ws is None:
            ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=self.g.device)
        outs = self.touts(None if bf16 else torch.float32) if outs is None else outs
        ptr = lambda t: None if t is None else t.data_ptr()
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        rc = self.lib.gnx_chain_block_forward_typed(self.g._h, C.byref(self.cp), elem, *map(ptr, self.xb if bf16 else self.xt), self.R, *map(ptr, outs),
                                                    ws.data_ptr(), nbytes, narrow, 0, s)
        assert rc == 0, self.lib.gnx_last_error()
        return outs

    def want(self, narrow=1):
        """to_bf16 of the mirrored fp32 entry on the widened inputs"""
        import torch
        ref = self.run(bool(narrow))
        torch.cuda.synchronize()
        return [None if t is None else t.to(torch.bfloat16) for t in ref]

    def check_forward(self, what, narrow=1):
        import torch
        got, want = self.trun(narrow), self.want(narrow)
        torch.cuda.synchronize()
        for n, u, v in zip(("ef", "nf", "gf"), got, want):
            assert (u is None) == (v is None), (what, n)
            if u is not None:
                assert not bool(torch.isnan(v.float()).any()), (what, n)
                bad = int((_bits(u) != _bits(v)).sum())
                assert bad == 0, f"{what} {n}: {bad} of {u.numel()} elements differ from to_bf16(fp32 entry)"

    # ---- backward ----
    def grad_names(self):
        """{name: element count} of every gradient the pullback can write"""
        out = {n: t.numel() for n, t in zip(("d_ef", "d_nf", "d_gf"), self.xt) if t is not None}
        for name in ("edge", "node", "graph"):
            for i, (w, b, c) in enumerate(self.p[name]):
                out[f"{name}{i}.dW"] = int(np.size(b) if isinstance(w, str) else np.size(w))
                out[f"{name}{i}.db"] = int(np.size(c) if isinstance(w, str) else np.size(b))
        return out

    def grads(self, bf16, skip=()):
        import torch
        mk = lambda n, k: torch.full((k,), float("nan"), dtype=torch.bfloat16 if bf16 and n.startswith("d_") else torch.float32, device=self.g.device)
        return {n: mk(n, k) for n, k in self.grad_names().items() if n not in skip}

    def bquery(self, narrow, elem):
        return self.lib.gnx_chain_block_backward_typed_workspace_bytes(self.g._h, C.byref(self.cp), self.R, elem, narrow)

    def brun(self, narrow, elem=None, plain=False, skip=(), no_cot=(), fill=0xA5):
        """the typed pullback — or (`plain`) the fp32 entry `narrow` selects — on the bf16 (elem BF16) or the widened tensors"""
        import torch
        L, lib = self.L, self.lib
        elem = L.ELEM_BF16 if elem is None else elem
        bf16 = elem == L.ELEM_BF16 and not plain
        if plain:
            q = lib.gnx_chain_block_backward_narrow_workspace_bytes if narrow else lib.gnx_chain_block_backward_workspace_bytes
            nbytes = q(self.g._h, C.byref(self.cp), self.R)
        else:
            nbytes = self.bquery(narrow, elem)
        assert nbytes > 0, lib.gnx_last_error()
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=self.g.device)
        outs = self.grads(bf16, skip)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        arrays = []
        for name in ("edge", "node", "graph"):
            arr = (L.DenseGrad * max(len(self.p[name]), 1))()
            for i in range(len(self.p[name])):
                arr[i] = L.DenseGrad(ptr(outs.get(f"{name}{i}.dW")), ptr(outs.get(f"{name}{i}.db")))
            arrays.append(arr)
        gr = L.ChainBlockGrads(*[C.cast(a, C.POINTER(L.DenseGrad)) for a in arrays])
        xin = [ptr(t) for t in (self.xb if bf16 else self.xt)]
        cot = [None if k in no_cot else ptr(t) for k, t in enumerate(self.cb if bf16 else self.cw)]
        dx = [ptr(outs.get(n)) for n in ("d_ef", "d_nf", "d_gf")]
        s = torch.cuda.current_stream().cuda_stream
        if plain:
            entry = lib.gnx_chain_block_backward_narrow if narrow else lib.gnx_chain_block_backward
            rc = entry(self.g._h, C.byref(self.cp), *xin, *cot, self.R, *dx, C.byref(gr), ws.data_ptr(), nbytes, s)
        else:
            rc = lib.gnx_chain_block_backward_typed(self.g._h, C.byref(self.cp), elem, *xin, *cot, self.R, *dx, C.byref(gr), ws.data_ptr(), nbytes, narrow, s)
        assert rc == 0, lib.gnx_last_error()
        torch.cuda.synchronize()
        return outs, nbytes

    def check_backward(self, what, narrow, skip=(), no_cot=()):
        import torch
        got, _ = self.brun(narrow, skip=skip, no_cot=no_cot)
        ref, _ = self.brun(narrow, plain=True, skip=skip, no_cot=no_cot)
        assert sorted(got) == sorted(ref) and not set(got) & set(skip)
        for n in got:
            if got[n].numel() == 0:
                continue
            assert not bool(torch.isnan(ref[n]).any()), (what, n)
            want = ref[n].to(torch.bfloat16) if n.startswith("d_") else ref[n]
            bad = int((_bits(got[n]) != _bits(want)).sum())
            assert bad == 0, f"{what} narrow={narrow} {n}: {bad} of {got[n].numel()} elements differ from the fp32 pullback's"


def _call(gn, i, R=1, cls=TCall):
    rng = np.random.default_rng(100 + i)
    return cls(gn, CN._adjs(rng), CN._params(rng, WIDTH_CASES[i]), R, seed=i)


# ---- 1. bit for bit, native ----
@pytest.mark.parametrize("i", range(len(WIDTH_CASES) + len(STRUCTURAL)), ids=[str(c[:4]) for c in WIDTH_CASES] + STRUCTURAL)
def test_native_bits(gn, i):
    import torch
    rng = np.random.default_rng(100 + i)
    if i < len(WIDTH_CASES):
        case, adjs, R, what = WIDTH_CASES[i], CN._adjs(rng), 1, str(WIDTH_CASES[i][:4])
    else:
        what = STRUCTURAL[i - len(WIDTH_CASES)]
        case, adjs, R = _structural(what, rng)
    c = TCall(gn, adjs, CN._params(rng, case), R, seed=i)
    want = (1 if case[1] and c.g.n_edges > 0 else 0) | (2 if case[2] else 0) | (4 if case[3] else 0)
    assert c.mask() == want, (what, c.mask(), want)
    assert c.native() == c.want_native() == 1, (what, c.native(), c.want_native())
    if R > 1:  # the replicas of an odd rows * d start on a 2-byte boundary
        odd = [t for t in c.xb if t is not None and (t.shape[1] * t.shape[2]) % 2 == 1]
        assert what != "odd-everything-replicas-3" or len(odd) == 3
        assert all((t.data_ptr() + 2 * t.shape[1] * t.shape[2]) % 4 == 2 for t in odd)
    c.check_forward(what)
    if what == "edgeless-batch":  # no edge launch; the node and graph functions still run
        prof = CN._profiled(gn, c.trun)
        assert sorted(prof) == sorted(NAMES[1:]), sorted(prof)
    torch.cuda.synchronize()


# ---- 2. the native form ran ----
def test_the_native_form_ran(gn):
    c = _call(gn, 0)
    assert c.mask() == 7 and c.native() == 1
    assert 0 < c.tquery(1) < c.tquery(0), (c.tquery(1), c.tquery(0))  # native < staged around gnx_chain_block_forward
    # ... and < what staging around the narrow entry would take: its workspace plus the six fp32 copies
    copies = sum(-(-4 * c.R * T * d // 256) * 256 for T, d in zip(c.rows * 2, list(c.p["in_dims"]) + list(c.outw)))
    assert c.tquery(1) < c.query(True) + copies
    c.trun()
    prof = CN._profiled(gn, c.trun)
    assert sorted(prof) == sorted(NAMES), f"other kernels than the three typed launches ran: {sorted(prof)}"
    for n in NAMES:
        assert prof[n]["launches"] == 1 and prof[n]["kernels"] == 1, (n, prof[n])
    # a graph input gf: additionally only its widening (G rows; the materialisation of the graph function's input rows has no name of its own)
    c = _call(gn, 6)
    assert c.mask() == 7 and c.native() == 1 and c.p["in_dims"][2] > 0
    c.trun()
    prof = CN._profiled(gn, c.trun)
    assert sorted(prof) == sorted(NAMES + ("k_bf16_widen",)), sorted(prof)
    assert all(prof[n]["kernels"] == 1 for n in prof), prof
    # staged (narrow = 0): the conversions run on every tensor
    old = CN._profiled(gn, lambda: c.trun(narrow=0))
    assert old["k_bf16_widen"]["kernels"] == 3 and old["k_bf16_round"]["kernels"] == 3, old


# ---- 3. staged paths ----
@pytest.mark.parametrize("i", (0, 2, 6), ids=lambda i: str(WIDTH_CASES[i][:4]))
def test_staged_around_the_generic_entry(gn, i):
    c = _call(gn, i)
    assert c.lib.gnx_chain_block_forward_typed_applies(c.g._h, C.byref(c.cp), c.R, c.L.ELEM_BF16, 0) == 0
    c.check_forward(f"narrow=0 {WIDTH_CASES[i][:4]}", narrow=0)


@pytest.mark.parametrize("widths,mask", ((([33, 3], [33, 4], [33, 5]), 0), (([33, 3], [8, 4], [40, 5]), 2), (([16, 3], [40, 4], [5]), 5)), ids=("mask0", "mask2", "mask5"))
def test_staged_outside_the_rule(gn, widths, mask):
    rng = np.random.default_rng(2)
    adjs = CN._adjs(rng)
    c = TCall(gn, adjs, O.make_chain_block_params(np.random.default_rng(20 + mask), (10, 5, 3), *widths), seed=mask)
    assert c.mask() == mask and c.native() == c.want_native() == 0
    c.check_forward(f"mask {mask}", narrow=1)


# ---- 4. GNX_ELEM_F32 is the fp32 entry ----
@pytest.mark.parametrize("narrow", (0, 1))
def test_elem_f32_is_the_fp32_entry(gn, narrow):
    import torch
    c = _call(gn, 2)
    F32 = c.L.ELEM_F32
    assert c.tquery(narrow, F32) == c.query(bool(narrow)) > 0
    assert c.lib.gnx_chain_block_forward_typed_applies(c.g._h, C.byref(c.cp), c.R, F32, narrow) == 0
    a, b = c.trun(narrow, elem=F32), c.run(bool(narrow))
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert _same(u, v)
    plain_q = c.lib.gnx_chain_block_backward_narrow_workspace_bytes if narrow else c.lib.gnx_chain_block_backward_workspace_bytes
    ga, na = c.brun(narrow, elem=F32)
    gb, nb = c.brun(narrow, plain=True)
    assert na == nb == plain_q(c.g._h, C.byref(c.cp), c.R) > 0
    assert sorted(ga) == sorted(gb)
    for n in ga:
        assert _same(ga[n], gb[n]), n


# ---- 5. memory contract ----
@pytest.mark.parametrize("mode", ("native", "staged", "backward"))
@pytest.mark.parametrize("i", (0, 2, 3, 6), ids=lambda i: str(WIDTH_CASES[i][:4]))
def test_memory_contract(gn, i, mode):
    """every buffer carved at its exact size, 4-byte aligned only (a skew of 4 bytes on every bf16 and fp32 carve), the workspace exactly the
    query's; nothing but the outputs and the workspace is written, the inputs are untouched; the bits depend neither on what the workspace held
    nor on the run; one byte less than the query is refused in the query's name with nothing written"""
    import torch
    L, lib = gn._lib, gn._lib.load()
    src = _call(gn, i)
    p, g, R = src.p, src.g, 1
    BF = L.ELEM_BF16
    narrow = 0 if mode == "staged" else 1
    a = AR.Arena("cuda", skew=lambda c: 0 if c.kind == AR.WORKSPACE else 4)
    _decl_chains(a, p)
    ins = [_decl(a, n, v) for n, v in zip(("ef", "nf", "gf"), src.xb)]
    keep = []
    P = a.ptr
    if mode == "backward":
        gs = [_decl(a, n, v) for n, v in zip(("g_ef_out", "g_nf_out", "g_gf_out"), src.cb)]
        dx = [a.output(n, v.shape, torch.bfloat16) if v is not None else None for n, v in zip(("d_ef", "d_nf", "d_gf"), src.xb)]
        for name in ("edge", "node", "graph"):
            for k, (w, b, c) in enumerate(p[name]):
                if isinstance(w, str):
                    a.output(f"grad.{name}{k}.dW", b.shape)
                    a.output(f"grad.{name}{k}.db", c.shape)
                else:
                    _decl_dense_grad(a, f"grad.{name}{k}", w, b)
        qname = b"gnx_chain_block_backward_typed_workspace_bytes()"
        ws = a.workspace("ws", lambda: lib.gnx_chain_block_backward_typed_workspace_bytes(g._h, C.byref(_chain_params(gn, a, p, keep)), R, BF, narrow))
        bf16_carves = ins + gs + dx

        def call(nbytes):
            arrays = []
            for name in ("edge", "node", "graph"):
                arr = (L.DenseGrad * max(len(p[name]), 1))()
                for k in range(len(p[name])):
                    arr[k] = _dense_grad(gn, a, f"grad.{name}{k}")
                arrays.append(arr)
            gr = L.ChainBlockGrads(*[C.cast(x_, C.POINTER(L.DenseGrad)) for x_ in arrays])
            rc = lib.gnx_chain_block_backward_typed(g._h, C.byref(_chain_params(gn, a, p, keep)), BF, *map(P, ins), *map(P, gs), R, *map(P, dx), C.byref(gr),
                                                    P(ws), nbytes, narrow, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return rc
    else:
        outs = _decl_outputs(a, "", R, src.rows, _chain_out_widths(p), torch.bfloat16)
        qname = b"gnx_chain_block_forward_typed_workspace_bytes()"
        ws = a.workspace("ws", lambda: lib.gnx_chain_block_forward_typed_workspace_bytes(g._h, C.byref(_chain_params(gn, a, p, keep)), R, BF, narrow))
        bf16_carves = ins + outs

        def call(nbytes):
            rc = lib.gnx_chain_block_forward_typed(g._h, C.byref(_chain_params(gn, a, p, keep)), BF, *map(P, ins), R, *map(P, outs), P(ws), nbytes, narrow, 0,
                                                   torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return rc
    a.build(ws_fill=0x00)
    assert a.nbytes(ws) > 0, lib.gnx_last_error()
    assert all(a.ptr(n) % 8 == 4 for n in bf16_carves if n is not None)
    assert lib.gnx_chain_block_forward_typed_applies(g._h, C.byref(_chain_params(gn, a, p, keep)), R, BF, narrow) == (1 if mode != "staged" else 0)
    bits = []
    for fill in (0x00, 0xFF, 0xFF):
        a.refill(fill)
        torch.cuda.synchronize()
        assert call(a.nbytes(ws)) == 0, lib.gnx_last_error()
        a.check(f"{mode} workspace {fill:#04x}")
        bits.append(a.output_bits())
    for k in bits[0]:
        assert torch.equal(bits[0][k], bits[1][k]), f"'{k}' depends on what the workspace held"
        assert torch.equal(bits[1][k], bits[2][k]), f"'{k}' differs between two calls"
    if mode == "native":  # the kernels read every parameter and feature element by element: the bits do not depend on the addresses either
        for n, w in zip(outs, src.want(1)):
            if n is not None:
                assert torch.equal(a.view(n).view(torch.int16), w.view(torch.int16)), n
    a.refill(0x00)
    torch.cuda.synchronize()
    before, ws_before = a.output_bits(), a.raw(ws).clone()
    assert call(a.nbytes(ws) - 1) == L.ERR_WORKSPACE and qname in lib.gnx_last_error()
    a.check("refused", unwritten=False)
    after = a.output_bits()
    assert all(torch.equal(before[k], after[k]) for k in before) and torch.equal(ws_before, a.raw(ws)), "a refused call wrote an output or the workspace"


# ---- 6. backward ----
@pytest.mark.parametrize("narrow", (0, 1))
@pytest.mark.parametrize("which", (0, 2, 6, "replicas-3"), ids=str)
def test_backward_bits(gn, which, narrow):
    if which == "replicas-3":
        rng = np.random.default_rng(150)
        case, adjs, R = _structural(which, rng)
        c = TCall(gn, adjs, CN._params(rng, case), R, seed=50)
    else:
        c = _call(gn, which)
    c.check_backward(str(which), narrow)
    # gradients that are not wanted and an upstream gradient that is NULL (= zero): as in the fp32 entry
    skip = {"d_nf", "edge0.dW", "node0.db", "graph0.dW", "graph0.db"}
    c.check_backward(f"{which} optional", narrow, skip=skip, no_cot=(1,))


# ---- 7. capture ----
def test_a_captured_native_forward_replays_the_eager_bits(gn):
    import torch
    c = _call(gn, 6)
    assert c.native() == 1
    nbytes = c.tquery(1)  # (builds the tables the call reads, outside the capture)
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device=c.g.device)
    eager = c.trun(ws=ws, nbytes=nbytes)
    torch.cuda.synchronize()
    graphed = c.touts()
    side = torch.cuda.Stream()
    cg = torch.cuda.CUDAGraph()
    gc.collect()  # nothing may free device memory while the capture is open
    gc.disable()
    try:
        with torch.cuda.stream(side):
            with torch.cuda.graph(cg, stream=side):
                c.trun(outs=graphed, ws=ws, stream=side.cuda_stream, nbytes=nbytes)
    finally:
        gc.enable()
    for t in graphed:
        t.zero_()
    cg.replay()
    torch.cuda.synchronize()
    for u, v in zip(eager, graphed):
        assert _same(u, v)


# ---- 8. Python ----
def _nt(gn, c, tensors):
    return gn.NT(c.g, *(None if t is None else t.permute(2, 1, 0) for t in tensors))


def test_python_no_grad_gives_the_entrys_bits(gn):
    import torch
    c = _call(gn, 2)
    blk = c.blk
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="bf16_chain"):  # off by default
            blk(_nt(gn, c, c.xb))
        blk.bf16_chain = True
        for narrow in (False, True):
            blk.narrow_chain = narrow
            want = c.trun(int(narrow))
            y = blk(_nt(gn, c, c.xb))
            prof = CN._profiled(gn, lambda: blk(_nt(gn, c, c.xb)))
            torch.cuda.synchronize()
            for got, w in zip((y.ef, y.nf, y.gf), want):
                assert got.dtype == torch.bfloat16 and _same(got.permute(2, 1, 0).contiguous(), w)
            if U.default_flags(gn) == 0:  # narrow_chain selects the mirrored entry: one launch per function and one widening (gf), or the generic launches
                if narrow:
                    assert sorted(prof) == sorted(NAMES + ("k_bf16_widen",)) and all(prof[n]["kernels"] == 1 for n in prof), prof
                else:
                    assert prof["k_bf16_round"]["kernels"] == 3 and prof["k_chain_layernorm"]["kernels"] == 3 and [prof[n]["kernels"] for n in NAMES] == [2, 2, 2], prof
        # a bf16 view that starts at an odd element is copied, not refused
        blk.narrow_chain = True
        base = torch.zeros(c.xb[0].numel() + 1, dtype=torch.bfloat16, device=c.g.device)
        base[1:] = c.xb[0].reshape(-1)
        odd = base[1:].view(c.xb[0].shape)
        assert odd.data_ptr() % 4 == 2
        y2 = blk(_nt(gn, c, [odd] + c.xb[1:]))
        torch.cuda.synchronize()
        assert _same(y2.ef, y.ef) and _same(y2.gf, y.gf)


@pytest.mark.parametrize("narrow_bw", (False, True))
def test_python_backward_through_the_switches(gn, narrow_bw):
    import torch
    c = _call(gn, 2)
    blk = c.blk
    blk.bf16_chain, blk.narrow_chain, blk.narrow_chain_backward = True, True, narrow_bw
    leaves = []
    for ch in (blk.edgefn, blk.nodefn, blk.graphfn):
        for l in ch.layers:
            l.weight.requires_grad_(True); l.bias.requires_grad_(True)
            leaves.append((l.weight, l.bias))
    xt = [None if t is None else t.clone().requires_grad_(True) for t in c.xb]
    with pytest.raises(NotImplementedError, match="bf16_backward"):
        blk(_nt(gn, c, xt))
    blk.bf16_backward = True
    want, _ = c.brun(int(narrow_bw))
    y = blk(_nt(gn, c, xt))
    assert all(o.dtype == torch.bfloat16 for o in (y.ef, y.nf, y.gf))
    loss = sum((o.permute(2, 1, 0).float() * ct.float()).sum() for o, ct in zip((y.ef, y.nf, y.gf), c.cb) if o is not None)
    prof = CN._profiled(gn, loss.backward)
    torch.cuda.synchronize()
    for n, t in zip(("d_ef", "d_nf", "d_gf"), xt):
        if t is not None:
            assert t.grad.dtype == torch.bfloat16 and torch.equal(_bits(t.grad).reshape(-1), _bits(want[n])), n
    k = 0
    for name in ("edge", "node", "graph"):
        for i in range(len(c.p[name])):
            w, b = leaves[k]; k += 1
            gw = w.grad if w.grad.dim() == 1 else w.grad.t()
            assert gw.dtype == torch.float32 and torch.equal(_bits(gw).reshape(-1), _bits(want[f"{name}{i}.dW"])), (name, i)
            assert torch.equal(_bits(b.grad).reshape(-1), _bits(want[f"{name}{i}.db"])), (name, i)
    if U.default_flags(gn) == 0:  # narrow_chain_backward selects the mirrored pullback: its launches and the nine conversions, nothing else
        assert prof.pop("k_bf16_widen")["kernels"] == 6 and prof.pop("k_bf16_round")["kernels"] == 3, prof
        kernels = lambda pr: {n: v["kernels"] for n, v in pr.items()}
        mirrored = CN._profiled(gn, lambda: c.brun(int(narrow_bw), plain=True))
        other = CN._profiled(gn, lambda: c.brun(int(not narrow_bw), plain=True))
        assert kernels(prof) == kernels(mirrored) != kernels(other), (kernels(prof), kernels(mirrored), kernels(other))


# ---- 9. seeded sweep ----
@pytest.mark.parametrize("seed", range(12 + EXTRA))
def test_seeded_sweep(gn, seed):
    rng = np.random.default_rng(7000 + seed)
    case = CN._random_block(rng)
    R = 1
    adjs = CN._adjs(rng)
    if seed % 6 == 5:
        adjs, R = CN._adjs(rng, [int(rng.integers(3, 40))]), int(rng.integers(2, 4))
    c = TCall(gn, adjs, CN._params(rng, case), R, seed=seed)
    assert c.mask() != 0, case
    assert c.native() == c.want_native(), case  # (a node / graph function behind a wide ef' may be outside the rule: then the call is staged)
    c.check_forward(f"sweep {seed} {case}")
