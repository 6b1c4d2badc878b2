"""gnx_block_backward_narrow on the GPU: the fused edge pullback at narrow width sets OUTSIDE the five ahead-of-time ones, its kernel specialised
at run time, and the five sets through the same entry.

Reference of the bits: gnx_block_backward (fp32) / gnx_block_backward_typed (bf16) on the same nine tensors — d_ef, d_nf, d_gf and the node /
graph parameter gradients must be their bits.  The edge function's weight / bias gradient, summed in the kernel's own fixed order, is compared
with torch float64 autograd at the bar of tests/test_gpu_bw_fused.py (max|got - ref| <= 2e-4 max(1, max|ref|)) in fp32, and in bf16 it must be
the bits of the fp32 narrow call on the exactly widened tensors.  Two runs on workspaces filled with different bytes give the same bits.

Width sets (de, dn, dg) => oe: (3,2,4)=>3 (36 weight-gradient pairs), (2,3,1)=>7 and (6,6,3)=>3 (70 and 66 pairs: two pair slots per lane),
(20,10,4)=>1 (44 weights in scalar registers, 47 KB of LDS), and one input entity alone: (1,0,0)=>1, (0,1,0)=>9, (0,0,1)=>5.  Graphs: the degree
graph of tests/test_gpu_bw_fused.py (a hub, isolated nodes, tiles of several 64-edge chunks, partial last chunks), its 40 small graphs, a
one-graph batch of ~20k edges whose wave-tile count is no multiple of four (the last workgroup has idle waves), a batch without edges.

Three tests start ONE child process each (GNX_JIT_ALL, GNX_JIT=0 and GNX_JIT_CACHE are read by the library once per process), every child
under its own time limit; an abnormal exit fails the test at once."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import util as U
from tests.arena import Arena, WORKSPACE
from tests.test_gpu_bw_fused import NAMES, SETS as AOT_SETS, _graph, _profiled, _ptr, _seed, _stream
from tests.test_gpu_bw_fused_bf16 import Case16, _at_the_bar, _rb, _same, _wide

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_SETS = (((3, 2, 4), 3), ((2, 3, 1), 7), ((6, 6, 3), 3), ((20, 10, 4), 1), ((1, 0, 0), 1), ((0, 1, 0), 9), ((0, 0, 1), 5))  # (de, dn, dg), oe
SETS = [pytest.param(s, id="%d%d%d-%d" % (*s[0], s[1])) for s in IN_SETS]
ACTS = ((0, 0, 0), (2, 3, 2), (3, 2, 3), (1, 2, 3))  # identity / tanh / sigmoid / relu on the edges (relu: kink-free draws)
S231 = ((2, 3, 1), (7, 4, 5))
S324 = ((3, 2, 4), (3, 4, 5))
NARROW, FUSED, TYPED = "narrow", "fused_typed", "typed"
ENTRY = {NARROW: ("gnx_block_backward_narrow_workspace_bytes", "gnx_block_backward_narrow"),
         FUSED: ("gnx_block_backward_fused_typed_workspace_bytes", "gnx_block_backward_fused_typed"),
         TYPED: ("gnx_block_backward_typed_workspace_bytes", "gnx_block_backward_typed")}
CHILD_TIMEOUT = 300  # seconds, each child process


@pytest.fixture(scope="module")
def gn():
    import torch
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


def n_wtiles(gn, g):
    n = C.c_int64(0)
    gn._lib.check(gn._lib.load().gnx_graphs_get_table(g._h, 7, None, 0, C.byref(n)))
    return n.value // 32  # (a Tile record is 32 bytes)


_own = {}


def graph(gn, name):
    """"e20k3": one graph of 2000 nodes and about 20 000 edges whose wave-tile count is no multiple of four; else the graphs of test_gpu_bw_fused"""
    if name != "e20k3":
        return _graph(gn, name)
    if name not in _own:
        for extra in range(8):
            colptr, rowval = U.er_csc(np.random.default_rng(31), 2000, 20000 + 37 * extra)
            g = gn.GNGraphBatch.from_csc([colptr], [rowval], [2000])
            if n_wtiles(gn, g) % 4 != 0:
                break
        else:
            pytest.fail("no 20k-edge batch whose wave-tile count is no multiple of four")
        _own[name] = g
    return _own[name]


def stats(gn):
    s = (C.c_int64 * 4)()
    gn._lib.check(gn._lib.load().gnx_jit_stats(s))
    return dict(compiled=s[0], disk_hits=s[1], failures=s[2], capture_misses=s[3])


class CaseN(Case16):
    """Case16 (the block, kink-free draw, fp32 and bf16 tensors of a backward call) with one runner for the three typed entry families"""

    def elem(self, bf16):
        return self.gn._lib.ELEM_BF16 if bf16 else self.gn._lib.ELEM_F32

    def tensors(self, bf16, cots=(True, True, True)):
        return self.nine16(cots) if bf16 else self.nine(cots)

    def applies_n(self, bf16):
        return int(self.gn._lib.load().gnx_block_backward_narrow_applies(self.g._h, C.byref(self.cp), self.R, self.elem(bf16)))

    def size(self, entry, bf16):
        return int(getattr(self.gn._lib.load(), ENTRY[entry][0])(self.g._h, C.byref(self.cp), self.R, self.elem(bf16)))

    def go(self, entry, bf16, nine, want_d=(True, True, True), want_g=(True,) * 6, grads_null=False, ws_fill=0xA5, out_bf16=None):
        """one call: [d_ef, d_nf, d_gf, dWe, dbe, dWn, dbn, dWg, dbg], None where not wanted; every output starts as NaN"""
        import torch
        g, R = self.g, self.R
        lib, L = self.gn._lib.load(), self.gn._lib
        dt = torch.bfloat16 if bf16 else torch.float32
        nan = lambda shape, dtype: torch.full(shape, float("nan"), dtype=dtype, device="cuda")
        d = [nan((R, T, w), dt) if (w > 0 and keep) else None for T, w, keep in zip(self.rows, self.in_dims, want_d)]
        flat = [s for pair in self.grad_shapes() for s in pair]
        gs = [nan(tuple(s), torch.float32) if keep and int(np.prod(s)) > 0 else None for s, keep in zip(flat, want_g)]
        grads = L.BlockGrads(*[L.DenseGrad(_ptr(gs[2 * i]), _ptr(gs[2 * i + 1])) for i in range(3)])
        nb = self.size(entry, bf16)
        assert nb > 0, lib.gnx_last_error()
        ws = torch.full((nb,), ws_fill, dtype=torch.uint8, device="cuda")
        rc = getattr(lib, ENTRY[entry][1])(g._h, C.byref(self.cp), self.elem(bf16), *map(_ptr, nine), R, *map(_ptr, d), None if grads_null else C.byref(grads),
                                           ws.data_ptr(), ws.numel(), _stream())
        assert rc == 0, lib.gnx_last_error()
        torch.cuda.synchronize()
        return d + (gs if not grads_null else [None] * 6)

    def check32(self, what, cots=(True, True, True), applies=1, **kw):
        """fp32: the generic call's bits everywhere but dWe / dbe, those at the bar against float64; two workspace fills, the same bits"""
        assert self.applies_n(False) == applies, what
        nine = self.nine(cots)
        ref = self.go(TYPED, False, nine, **kw)  # (GNX_ELEM_F32: gnx_block_backward)
        got = self.go(NARROW, False, nine, **kw)
        again = self.go(NARROW, False, nine, ws_fill=0x3C, **kw)
        f64 = None
        for i, (name, a, b, r) in enumerate(zip(NAMES, got, again, ref)):
            _same(a, b, f"{what} {name}: two runs, two workspace fills")
            if i in (3, 4) and applies and a is not None:
                f64 = f64 or self.edge_grads_f64(cots)
                _at_the_bar(a, f64[i - 3], f"{what} {name}")
            else:
                _same(a, r, f"{what} {name}: the generic call")
        if not applies:
            assert self.size(NARROW, False) == self.size(TYPED, False), what
        return got

    def check16(self, what, cots=(True, True, True), applies=1, **kw):
        """bf16: the typed call's bits everywhere but dWe / dbe, those the bits of the fp32 narrow call on the widened tensors"""
        assert self.applies_n(True) == applies, what
        nine = self.nine16(cots)
        typed = self.go(TYPED, True, nine, **kw)
        got = self.go(NARROW, True, nine, **kw)
        again = self.go(NARROW, True, nine, ws_fill=0x3C, **kw)
        wide = self.go(NARROW, False, _wide(nine), **kw) if applies else None
        for i, (name, a, b, t) in enumerate(zip(NAMES, got, again, typed)):
            _same(a, b, f"{what} {name}: two runs, two workspace fills")
            if i in (3, 4) and applies:
                _same(a, wide[i], f"{what} {name}: the fp32 narrow call on the widened tensors")
            else:
                _same(a, t, f"{what} {name}: the typed call")
                if applies:
                    _same(a, _rb(wide[i]) if i < 3 else wide[i], f"{what} {name}: the fp32 narrow call on the widened tensors")
        if not applies:
            assert self.size(NARROW, True) == self.size(TYPED, True), what
        return got


def digest_view(t):
    import torch
    return t.contiguous().view(-1).view(torch.uint8)


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(b"-" if t is None else digest_view(t).cpu().numpy().tobytes())
    return h.hexdigest()


# ---- 1. bits and edge gradients, fp32 ----
@pytest.mark.parametrize("dims", SETS)
@pytest.mark.parametrize("name", ["degrees", "small40", "e20k3", "edgeless"])
def test_bits_of_the_generic_backward_and_edge_gradients_at_the_bar(gn, name, dims):
    g = graph(gn, name)
    ins, oe = dims
    applies = 0 if name == "edgeless" else 1
    for act in ACTS:
        CaseN(gn, g, 1, ins, (oe, 4, 5), act, _seed("n32", dims, act, name)).check32(f"{name} {ins}=>{oe} act={act}", applies=applies)
    for out in ((oe, 0, 5), (oe, 4, 0), (oe, 0, 0)):  # on = 0, og = 0, both
        CaseN(gn, g, 1, ins, out, (2, 3, 2), _seed("n32", dims, out, name)).check32(f"{name} {ins}=>{out}", applies=applies)


# ---- 2. bf16 ----
@pytest.mark.parametrize("dims", SETS)
@pytest.mark.parametrize("name", ["degrees", "small40", "e20k3"])
def test_bf16_bits_of_the_typed_backward_and_of_the_fp32_narrow_call(gn, name, dims):
    g = graph(gn, name)
    ins, oe = dims
    for act in ((1, 2, 3), (2, 3, 0)):
        CaseN(gn, g, 1, ins, (oe, 4, 5), act, _seed("n16", dims, act, name)).check16(f"bf16 {name} {ins}=>{oe} act={act}")


# ---- 3. replicas ----
@pytest.mark.parametrize("name,R", [("degrees", 2), ("degrees", 3), ("e20k3", 2)], ids=["degrees-R2", "degrees-R3", "e20k3-R2"])
def test_replicas(gn, name, R):
    g = graph(gn, name)
    assert g.n_graphs == 1
    for dims in (S324, S231):
        c = CaseN(gn, g, R, *dims, (2, 3, 0), _seed("nrep", R, dims))
        c.check32(f"{name} R={R} {dims}")
        c.check16(f"bf16 {name} R={R} {dims}")


# ---- 4. optional arguments ----
@pytest.mark.parametrize("name", ["degrees", "small40"])
def test_optional_arguments(gn, name):
    c = CaseN(gn, graph(gn, name), 1, *S231, (1, 2, 3), 77)
    for check in (c.check32, c.check16):
        for k in range(3):
            check(f"{name} without cotangent {k}", cots=tuple(i != k for i in range(3)))
        check(f"{name} without any cotangent", cots=(False, False, False))
        for k in range(3):
            check(f"{name} without d[{k}]", want_d=tuple(i != k for i in range(3)))
        check(f"{name} no input gradient", want_d=(False, False, False))
        check(f"{name} grads NULL", grads_null=True)
        check(f"{name} dWe alone", want_g=(True, False, False, False, False, False))
        check(f"{name} dbe alone", want_g=(False, True, False, False, False, False))
        check(f"{name} no edge gradient", want_g=(False, False, True, True, True, True))


# ---- 5. the five ahead-of-time sets through the new entry ----
@pytest.mark.parametrize("dims", AOT_SETS)
def test_the_listed_sets_are_the_fused_typed_call(gn, dims):
    for name in ("degrees", "e20k3"):
        c = CaseN(gn, graph(gn, name), 1, *dims, (1, 2, 3), _seed("aot", dims, name))
        for bf16 in (False, True):
            assert c.applies_n(bf16) == 1
            assert c.size(NARROW, bf16) == c.size(FUSED, bf16)
            nine = c.tensors(bf16)
            for n, a, b in zip(NAMES, c.go(NARROW, bf16, nine), c.go(FUSED, bf16, nine, ws_fill=0x3C)):
                _same(a, b, f"{name} {dims} bf16={bf16} {n}: gnx_block_backward_fused_typed")


# ---- children ----
def child(mode, env):
    """one child process (python -m tests.bw_narrow_child MODE) under its own time limit; its last output line as JSON"""
    r = subprocess.run([sys.executable, "-m", "tests.bw_narrow_child", mode], env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, f"child {mode}: exit {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
    return json.loads(r.stdout.strip().splitlines()[-1])


# ---- 6. GNX_JIT_ALL: the hiprtc build of the kernel equals the ahead-of-time build ----
def test_jit_all_runs_the_run_time_kernel_at_the_listed_sets_with_the_same_bits(gn):
    out = child("jit_all", dict(GNX_JIT_ALL="1"))
    assert out["failures"] == 0 and out["compiled"] >= 10, out  # five sets, two element types
    assert out["cases"] == 10 and out["differing"] == [], out


# ---- 7. where it does not apply ----
def test_where_it_does_not_apply_it_is_the_typed_backward(gn):
    for name, dims, act in (("degrees", S231, (4, 0, 0)), ("degrees", ((10, 5, 3), (3, 4, 5)), (2, 2, 2)), ("degrees", ((23, 15, 10), (1, 4, 5)), (2, 2, 2)),
                            ("edgeless", S231, (2, 2, 2))):
        c = CaseN(gn, graph(gn, name), 1, *dims, act, 5)
        before = stats(gn)  # (behind the forward, which has run-time kernels of its own)
        c.check32(f"not applicable: {name} {dims} {act}", applies=0)
        c.check16(f"not applicable: {name} {dims} {act}", applies=0)
        c.check32(f"not applicable: {name} {dims} {act}, d_nf alone", applies=0, want_d=(False, True, False), want_g=(False,) * 6)
        assert stats(gn) == before  # (the backward did not reach the specialiser)
    # the same handle, the same widths, but a gelu NODE function: the edge level is still fused
    assert CaseN(gn, graph(gn, "degrees"), 1, *S231, (2, 4, 4), 6).applies_n(False) == 1


def test_without_run_time_specialisation_it_is_the_typed_backward(gn):
    out = child("nojit", dict(GNX_JIT="0"))
    assert out["applies"] == [0, 0] and out["sizes_equal"] == [True, True] and out["differing"] == [], out
    assert out["listed_applies"] == [1, 1], out  # (the ahead-of-time sets need no specialiser)
    assert out["stats"] == dict(compiled=0, disk_hits=0, failures=0, capture_misses=0), out


# ---- 8. first use inside a capture ----
def test_first_use_inside_a_capture_takes_the_generic_form_and_compiles_nothing(gn):
    import torch
    lib, L = gn._lib.load(), gn._lib
    dims = ((4, 1, 2), (5, 4, 5))  # (a width set no other test of this process uses)
    c = CaseN(gn, graph(gn, "e20k3"), 1, *dims, (1, 2, 3), 14)
    nine = c.nine()
    generic = c.go(TYPED, False, nine)  # (its query builds what the backward reads: outside the capture)

    def captured(nbytes):
        outs = [None if t is None else torch.zeros_like(t) for t in generic]
        grads = L.BlockGrads(*[L.DenseGrad(_ptr(outs[3 + 2 * i]), _ptr(outs[4 + 2 * i])) for i in range(3)])
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        graph_ = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph_, stream=s):
                rc = lib.gnx_block_backward_narrow(c.g._h, C.byref(c.cp), L.ELEM_F32, *map(_ptr, nine), 1, *map(_ptr, outs[:3]), C.byref(grads), ws.data_ptr(),
                                                   ws.numel(), s.cuda_stream)
        assert rc == 0, lib.gnx_last_error()
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(2):
            graph_.replay()
        torch.cuda.synchronize()
        return outs, (ws, grads)

    before = stats(gn)
    outs, _keep = captured(c.size(TYPED, False))
    after = stats(gn)
    assert after["capture_misses"] == before["capture_misses"] + 1 and after["compiled"] == before["compiled"] and after["failures"] == 0, (before, after)
    for name, x, y in zip(NAMES, outs, generic):
        _same(x, y, f"first use inside a capture, {name}: the generic call")
    assert c.applies_n(False) == 1  # the query, outside any capture, obtains the kernel
    assert stats(gn)["compiled"] == after["compiled"] + 1
    eager = c.go(NARROW, False, nine)
    assert c.size(NARROW, False) < c.size(TYPED, False)
    outs, _keep = captured(c.size(NARROW, False))
    assert stats(gn)["capture_misses"] == after["capture_misses"]
    for name, x, y in zip(NAMES, outs, eager):
        _same(x, y, f"captured after the query, {name}: the fused call")
    for i, (x, y) in enumerate(zip(outs, generic)):
        if i not in (3, 4):
            _same(x, y, f"captured after the query, {NAMES[i]}: the generic call")


# ---- 9. disk cache ----
def test_the_code_object_is_kept_on_disk_for_the_next_process(gn, tmp_path):
    dims = ((1, 2, 3), (4, 4, 5))  # (a width set no other test of this process uses; the child runs the same case)
    os.environ["GNX_JIT_CACHE"] = str(tmp_path)
    try:
        c = CaseN(gn, graph(gn, "degrees"), 1, *dims, (2, 3, 2), 15)  # (the forward's run-time kernels go to the same directory)
        before = stats(gn)
        here = [digest(c.go(NARROW, bf16, c.tensors(bf16))) for bf16 in (False, True)]
        after = stats(gn)
    finally:
        del os.environ["GNX_JIT_CACHE"]
    assert after["compiled"] == before["compiled"] + 2 and after["failures"] == 0
    files = sorted(f for f in os.listdir(tmp_path) if f.startswith("gnx_bw_edge_"))
    assert len(files) == 2 and files[0].startswith("gnx_bw_edge_1_2_3_4_bf16_") and files[1].startswith("gnx_bw_edge_1_2_3_4_f32_"), files
    out = child("cache", dict(GNX_JIT_CACHE=str(tmp_path)))
    assert out["stats"]["compiled"] == 0 and out["stats"]["disk_hits"] >= 2 and out["bw_disk_hits"] == 2 and out["stats"]["failures"] == 0, out
    assert out["applies"] == [1, 1] and out["digests"] == here, (out, here)


# ---- 10. launch structure ----
def test_launch_structure(gn):
    """against the generic call: no edge function-input launch, no edge dX launch, one kernel under bw_delta_edge, the final reduction alone for
    the edge weight gradient, no new profiler name"""
    if U.default_flags(gn) != 0:
        return  # (forms switched on for the whole process change which kernels run, not the bits)
    for name, R, bf16 in (("e20k3", 1, False), ("e20k3", 2, True), ("small40", 1, False)):
        c = CaseN(gn, graph(gn, name), R, *S231, (1, 2, 3), 9)
        assert c.applies_n(bf16) == 1
        nine = c.tensors(bf16)
        gen = _profiled(gn, lambda: c.go(TYPED, bf16, nine))
        new = _profiled(gn, lambda: c.go(NARROW, bf16, nine))
        assert set(new) <= set(gen), (sorted(new), sorted(gen))
        assert new["bw_fn_inputs"]["kernels"] == gen["bw_fn_inputs"]["kernels"] - 1, (new["bw_fn_inputs"], gen["bw_fn_inputs"])
        assert new["bw_dx_generic"]["launches"] == gen["bw_dx_generic"]["launches"] - 1, (new["bw_dx_generic"], gen["bw_dx_generic"])
        assert new["bw_delta_edge"]["kernels"] == gen["bw_delta_edge"]["kernels"] == 1
        assert new["bw_dw_generic"]["kernels"] == gen["bw_dw_generic"]["kernels"] - 1


# ---- 11. workspace ----
@pytest.mark.parametrize("dims", [S324, S231, ((20, 10, 4), (1, 4, 5))], ids=["324", "231", "20104"])
def test_workspace(gn, dims):
    import torch
    lib, L = gn._lib.load(), gn._lib
    c = CaseN(gn, graph(gn, "e20k3"), 1, *dims, (2, 2, 2), 12)
    ke = dims[0][0] + 2 * dims[0][1] + dims[0][2]
    for bf16 in (False, True):
        assert c.applies_n(bf16) == 1
        fused, generic = c.size(NARROW, bf16), c.size(TYPED, bf16)
        print(f"{dims} bf16={bf16}: narrow {fused} B, generic {generic} B, Xe {4 * c.g.n_edges * ke} B")
        assert fused <= generic - 4 * c.g.n_edges * ke, (fused, generic)
        nine = c.tensors(bf16)
        outs = [None if t is None else torch.full_like(t, float("nan")) for t in c.go(NARROW, bf16, nine)]
        grads = L.BlockGrads(*[L.DenseGrad(_ptr(outs[3 + 2 * i]), _ptr(outs[4 + 2 * i])) for i in range(3)])
        ws = torch.full((fused,), 0x5A, dtype=torch.uint8, device="cuda")
        call = lambda p, n: lib.gnx_block_backward_narrow(c.g._h, C.byref(c.cp), c.elem(bf16), *map(_ptr, nine), 1, *map(_ptr, outs[:3]), C.byref(grads), p, n, _stream())
        assert call(ws.data_ptr(), fused - 1) == L.ERR_WORKSPACE and b"gnx_block_backward_narrow_workspace_bytes" in lib.gnx_last_error()
        assert call(None, fused) == L.ERR_WORKSPACE
        torch.cuda.synchronize()
        assert bool((ws == 0x5A).all()) and all(bool(torch.isnan(t.float()).all()) for t in outs if t is not None)


# ---- 12. memory contract ----
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dims", [S231, ((1, 0, 0), (1, 4, 5))], ids=["231", "100"])
def test_arena_memory_contract_and_skewed_addresses(gn, dims, bf16):
    """Every buffer of the call at its exact byte size inside one sentinel arena, aligned and 4 / 8 / 12 bytes behind a 256-byte boundary (the
    workspace on it): nothing outside the outputs and the workspace is written, the inputs are untouched, every requested output element is
    written, the bits are those of the plain-tensor run and do not depend on the address or on what the workspace held."""
    import torch
    lib, L = gn._lib.load(), gn._lib
    g, R = graph(gn, "degrees"), 1
    c = CaseN(gn, g, R, *dims, (1, 2, 3), 13)
    assert c.applies_n(bf16) == 1
    a = Arena("cuda")
    names = ("ef", "nf", "gf", "ef_out", "nf_out", "gf_out", "g_ef_out", "g_nf_out", "g_gf_out")
    nine = [a.input(n, t) if t is not None else None for n, t in zip(names, c.tensors(bf16))]
    dt = torch.bfloat16 if bf16 else torch.float32
    dx = [a.output(n, t.shape, dt) if t is not None else None for n, t in zip(("d_ef", "d_nf", "d_gf"), c.ins)]
    gnames = []
    for fn, (sw, sb) in zip(("edgefn", "nodefn", "graphfn"), c.grad_shapes()):
        gnames += [a.output(f"grad.{fn}.dW", sw), a.output(f"grad.{fn}.db", sb)]
    ws = a.workspace("ws", c.size(NARROW, bf16))
    a.build(ws_fill=0x00)

    def run():
        keep = []
        cp = c.blk._c(keep)
        grads = L.BlockGrads(*[L.DenseGrad(a.ptr(gnames[2 * k]), a.ptr(gnames[2 * k + 1])) for k in range(3)])
        rc = lib.gnx_block_backward_narrow(g._h, C.byref(cp), c.elem(bf16), *map(a.ptr, nine), R, *map(a.ptr, dx), C.byref(grads), a.ptr(ws), a.nbytes(ws), _stream())
        torch.cuda.synchronize()
        return rc

    assert run() == 0, lib.gnx_last_error()
    a.check(f"{dims} aligned")
    base = a.output_bits()
    ref = c.go(NARROW, bf16, c.tensors(bf16))
    for n, t in zip(dx + gnames, ref):
        if n is not None:
            assert torch.equal(a.raw(n), t.contiguous().view(-1).view(torch.uint8)), n
    for k in (4, 8, 12):  # every buffer k bytes behind a 256-B boundary, the workspace on it
        a.relayout(lambda cv: 0 if cv.kind == WORKSPACE else k, ws_fill=0xFF)
        assert run() == 0, (k, lib.gnx_last_error())
        a.check(f"{dims} skew +{k}")
        got = a.output_bits()
        assert all(torch.equal(got[n], base[n]) for n in base), f"{dims}: other bits at +{k}"


# ---- 13. Python ----
def _py_grads(gn, narrow, bf16):
    import torch
    from oracle import gn_oracle as O
    rng = np.random.default_rng(21)
    colptr, rowval = U.er_csc(rng, 300, 2500)
    g = gn.GNGraphBatch.from_csc([colptr], [rowval], [300])
    blk = U.block_from_params(gn, O.make_block_params(rng, *S324, act=(2, 2, 0)))
    blk.narrow_backward, blk.bf16_backward = narrow, bf16
    params = [blk.edgefn.weight, blk.edgefn.bias, blk.nodefn.weight, blk.nodefn.bias, blk.graphfn.weight, blk.graphfn.bias]
    for t in params:
        t.requires_grad_(True)
    x = U.to_nt(gn, g, *U.packed_inputs(rng, 1, 2500, 300, 1, S324[0]))
    cot = [torch.from_numpy(rng.standard_normal((d, T, 1)).astype(np.float32)).to(g.device) for d, T in zip(S324[1], (2500, 300, 1))]
    cast = (lambda t: t.to(torch.bfloat16)) if bf16 else (lambda t: t)
    ins = [cast(t).detach().requires_grad_(True) for t in (x.ef, x.nf, x.gf)]
    y = blk(gn.NT(x.graphs, *ins))
    sum((t.float() * cast(c).float()).sum() for t, c in zip((y.ef, y.nf, y.gf), cot)).backward()
    return [t.grad for t in ins] + [t.grad for t in params]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_python_autograd_with_the_switch(gn, bf16):
    """GNBlock((3,2,4), (3,4,5), narrow_backward=True) under torch.autograd against the same block without the switch: the input gradients and the
    node / graph parameter gradients are its bits, the edge function's are within the bar"""
    assert gn.GNBlock(*S324, narrow_backward=True, bf16_backward=bf16).narrow_backward is True
    before = stats(gn)
    res = [_py_grads(gn, narrow, bf16) for narrow in (False, True)]
    assert stats(gn)["failures"] == before["failures"]
    for i, (name, a, b) in enumerate(zip(("x.ef", "x.nf", "x.gf", "We", "be", "Wn", "bn", "Wg", "bg"), *res)):
        if i in (3, 4):
            _at_the_bar(b, a.double().cpu().numpy(), f"python {name}")
        else:
            _same(a.contiguous(), b.contiguous(), f"grad {name}")
