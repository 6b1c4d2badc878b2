"""CPU-side checks of the bfloat16 loop over batches (gnx_block_forward_steps_typed): the entry is declared, exported and bound; its argument
errors come back before any GPU work, with nothing written; the step spans of the two-stream schedule's hazard rule count 2 bytes per bf16
feature (gnx_step_hazard.h compiled with g++); the chained bf16 kernels keep no register in scratch memory and no more registers than their
fp32 counterparts; BlockPlan's dtype checks run before any library call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphnets.jl_amd", "csrc")
NAME = "gnx_block_forward_steps_typed"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    return gn._lib.load()


def test_steps_typed_declared_exported_and_bound(lib):
    import graphnets_jl_amd as gn
    with open(os.path.join(ROOT, "include", "gnx.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"GNX_API [\w\s\*]+?\b" + NAME + r"\(([^;]*?)\);", text, flags=re.S)
    assert m, f"{NAME} is not declared in include/gnx.h"
    assert m.group(1).count(",") + 1 == 8
    assert hasattr(lib, NAME)
    assert NAME in gn._lib.SIGNATURES and len(gn._lib.SIGNATURES[NAME][1]) == 8
    assert lib.gnx_version() == 130


def _params(gn):
    p = gn._lib.BlockParams(3, 4, 5, 3, 4, 5)
    w = np.zeros(64, dtype=np.float32)  # (never read: every call below fails before any GPU work)
    p.edgefn.weight = p.nodefn.weight = p.graphfn.weight = w.ctypes.data
    return p, w


def _steps(gn, n, bufs, misalign_last=False):
    arr = (gn._lib.BlockStep * max(n, 1))()
    for i in range(n):
        b = [x.ctypes.data for x in bufs]
        if misalign_last and i == n - 1:
            b[4] += 2  # nf_out of the LAST step: 2-byte aligned only
        arr[i] = gn._lib.BlockStep(*b[:6], b[6], 4096)
    return arr


def test_arguments_refused_before_any_gpu_work(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    p, _keep = _params(gn)
    bufs = [np.zeros(512, dtype=np.uint16) for _ in range(7)]
    arr = _steps(gn, 3, bufs)
    for elem in (-1, 0, 1, 2, 4, 6, 99):
        assert lib.gnx_block_forward_steps_typed(None, C.byref(p), elem, arr, 3, 1, 0, None) == L.ERR_INVALID_ARG
        assert b"elem" in lib.gnx_last_error()
    assert lib.gnx_block_forward_steps_typed(None, C.byref(p), L.ELEM_BF16, arr, 3, 1, L.FLAG_DEFER_GRAPH_UPDATE, None) == L.ERR_INVALID_ARG
    assert b"graph update" in lib.gnx_last_error()
    assert lib.gnx_block_forward_steps_typed(None, C.byref(p), L.ELEM_BF16, arr, -1, 1, 0, None) == L.ERR_INVALID_ARG
    assert b"n_steps" in lib.gnx_last_error()
    assert lib.gnx_block_forward_steps_typed(None, C.byref(p), L.ELEM_BF16, None, 2, 1, 0, None) == L.ERR_INVALID_ARG
    assert b"NULL" in lib.gnx_last_error()
    # a misaligned buffer in the last step is found before the first step runs (which would report the NULL handle)
    assert lib.gnx_block_forward_steps_typed(None, C.byref(p), L.ELEM_BF16, _steps(gn, 3, bufs, True), 3, 1, 0, None) == L.ERR_INVALID_ARG
    assert b"aligned" in lib.gnx_last_error()
    # no step at all: nothing to do
    assert lib.gnx_block_forward_steps_typed(None, C.byref(p), L.ELEM_BF16, None, 0, 1, 0, None) == 0
    assert all(np.all(b == 0) for b in bufs)
    # GNX_ELEM_F32 is gnx_block_forward_steps, errors included
    for args in ((arr, 3, 1, 0), (arr, -1, 1, 0), (None, 2, 1, 0), (arr, 3, 1, L.FLAG_DEFER_GRAPH_UPDATE)):
        want = lib.gnx_block_forward_steps(None, C.byref(p), *args, None)
        msg = lib.gnx_last_error()
        assert want != 0
        assert lib.gnx_block_forward_steps_typed(None, C.byref(p), L.ELEM_F32, *args, None) == want
        assert lib.gnx_last_error() == msg
    assert all(np.all(b == 0) for b in bufs)


HAZARD_DRIVER = r"""
#include <cstdio>
#include "gnx_step_hazard.h"
using namespace gnx;
static char buf[1 << 20];
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
static const long long rows[3] = {1000, 300, 2};  // E, N, G
static const int in_w[3] = {3, 4, 5}, out_w[3] = {3, 4, 5};
// a step whose six feature buffers start at the given offsets (-1: width 0 <=> nothing), its workspace at ws
static StepSpans step(const long long off[6], long long ws, size_t elem, long long R = 1) {
  const void* in[3];
  const void* out[3];
  for (int t = 0; t < 3; ++t) {
    in[t] = off[t] < 0 ? nullptr : buf + off[t];
    out[t] = off[3 + t] < 0 ? nullptr : buf + off[3 + t];
  }
  return step_spans_of(in, out, buf + ws, 8192, rows, in_w, out_w, R, elem, 4096);
}
int main() {
  const long long a[6] = {0, 16384, 32768, 49152, 65536, 81920};
  for (long long R = 1; R <= 3; R += 2) {
    const StepSpans f = step(a, 131072, 4, R), h = step(a, 131072, 2, R);
    for (int t = 0; t < 3; ++t) {
      EXPECT(f.rd[t].lo == h.rd[t].lo && f.wr[t].lo == h.wr[t].lo);
      EXPECT(f.rd[t].hi - f.rd[t].lo == 2 * (h.rd[t].hi - h.rd[t].lo));
      EXPECT(f.wr[t].hi - f.wr[t].lo == 2 * (h.wr[t].hi - h.wr[t].lo));
      EXPECT(h.rd[t].hi - h.rd[t].lo == (uintptr_t)(2 * R * rows[t] * in_w[t]));
    }
    // the workspace: what the block's kernels use (the query's figure), whatever the element type
    EXPECT(f.wr[3].hi - f.wr[3].lo == 4096 && h.wr[3].hi - h.wr[3].lo == 4096);
  }
  // bf16 ef (1000 x 3 x 2 B = 6000 B): a second step's nf that starts one ELEMENT before its end conflicts, one that starts at its end does not
  const long long E_BYTES = 2 * 1000 * 3;
  const long long b1[6] = {200000, E_BYTES - 2, 220000, 240000, 260000, 280000};  // reads [E_BYTES - 2, ...): one element of a's ef... as a read
  const long long w1[6] = {200000, 210000, 220000, E_BYTES - 2, 260000, 280000};  // WRITES ef_out over a's last ef element
  const long long w0[6] = {200000, 210000, 220000, E_BYTES, 260000, 280000};      // writes right behind a's ef
  const StepSpans s0 = step(a, 131072, 2);
  EXPECT(!steps_conflict(s0, step(b1, 300000, 2)));  // reads only: never a conflict
  EXPECT(steps_conflict(s0, step(w1, 300000, 2)) && steps_conflict(step(w1, 300000, 2), s0));
  EXPECT(!steps_conflict(s0, step(w0, 300000, 2)) && !steps_conflict(step(w0, 300000, 2), s0));
  // the same offsets as fp32 would overlap (the fp32 ef is 12000 B): the bf16 spans are not fp32 spans
  EXPECT(steps_conflict(step(a, 131072, 4), step(w0, 300000, 4)));
  // an absent tensor never conflicts
  const long long n0[6] = {-1, 16384, -1, -1, 65536, -1};
  const long long n1[6] = {-1, 400000, -1, -1, 420000, -1};
  EXPECT(!steps_conflict(step(n0, 500000, 2), step(n1, 600000, 2)));
  if (fails) return 1;
  std::printf("bf16 spans ok\n");
  return 0;
}
"""


def test_bf16_step_spans_compiled_with_gxx(tmp_path):
    src = tmp_path / "drv.cpp"
    src.write_text(HAZARD_DRIVER)
    exe = tmp_path / "drv"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bf16 spans ok" in r.stdout


def test_chained_bf16_kernels_resource_audit():
    """k_block_wave<..., CHAIN, BF16> of every bf16 ahead-of-time width set (one graph and several graphs), compiled as build.py compiles
    gnx_narrow_bf16.hip: no scratch, at most the kernel's 80 scalar registers, no more vector registers than the fp32 chained kernel"""
    from tools.kernel_resources import HIPCC, remarks_many
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    res = dict(zip(("bf16", "f32"), remarks_many(["gnx_narrow_bf16.hip", "gnx_narrow.hip"])))  # (both compiles at once, as build.py compiles the files)
    chained = {n: v for n, v in res["bf16"].items() if re.match(r"_ZN3gnx12k_block_waveI(Li\d+E){6}(Lb[01]E){4}Lb1ELb1EEEv", n)}
    # two per NF_PLAIN set of the bf16 list in gnx_narrow_sets.h (one graph, several graphs); (10,5,0) => (3,4,5) and (3,4,5) => (3,4,5) at least
    assert len(chained) >= 4 and any("ILi3ELi4ELi5ELi3ELi4E" in n for n in chained), sorted(chained)
    for n, v in chained.items():
        f32 = res["f32"].get(n.replace("ELb1ELb1EEEv", "ELb1ELb0EEEv"))
        assert f32 is not None, f"no fp32 chained kernel for {n}"
        assert v["scratch"] == 0, (n, v)
        assert v["sgpr"] <= 80, (n, v)
        assert v["vgpr"] <= f32["vgpr"], (n, v, f32)


def test_blockplan_dtype_checks_before_any_library_call(monkeypatch):
    import torch
    import graphnets_jl_amd as gn

    def no_lib():
        raise AssertionError("the library was called")

    monkeypatch.setattr(gn._lib, "load", no_lib)
    blk = gn.GNBlock((3, 4, 5), (3, 4, 5), device="cpu")
    with pytest.raises(TypeError, match="dtype"):
        gn.BlockPlan(blk, object(), dtype=torch.float16)
    # a bf16 plan as __init__ leaves it, without the library (the checks below come first)
    plan = gn.BlockPlan.__new__(gn.BlockPlan)
    plan.block, plan.g, plan.R, plan.flags, plan.bf16, plan.lib, plan.ws = blk, None, 1, 0, True, None, None
    bf = lambda *s: torch.zeros(s, dtype=torch.bfloat16)
    ins = (bf(1, 6, 3), bf(1, 3, 4), bf(1, 1, 5))
    outs = (bf(1, 6, 3), bf(1, 3, 4), bf(1, 1, 5))
    ws = torch.zeros(256, dtype=torch.uint8)
    with pytest.raises(TypeError, match="bfloat16"):
        plan(*ins, *outs, defer_graph_update=True)
    with pytest.raises(TypeError, match="bfloat16"):
        plan(ins[0].float(), *ins[1:], *outs)
    with pytest.raises(TypeError, match="bfloat16"):
        plan(*ins, outs[0], outs[1].float(), outs[2])
    good = dict(ef=ins[0], nf=ins[1], gf=ins[2], out=outs, ws=ws)
    with pytest.raises(TypeError, match="bfloat16"):
        plan.steps([good, dict(good, gf=ins[2].float())])
    with pytest.raises(TypeError, match="bfloat16"):
        plan.steps([good, (*ins, outs[0], outs[1], outs[2].double(), ws)])
    for call in (lambda: plan.chained(*ins, *outs, ws), lambda: plan.flush(None), lambda: plan.graph_update(ins[2], outs[2])):
        with pytest.raises(TypeError, match="bfloat16"):
            call()
