"""Times the backward of one GNBlock at README widths (10,5,0) => (3,4,5) on the 1M-edge batch (BASELINE configs[1]) in three forms:

  (a) gnx_block_backward on fp32 tensors;
  (b) what a bf16 caller ran before gnx_block_backward_typed: torch .float() of the feature-shaped inputs, gnx_block_backward, torch
      .to(bfloat16) of the input gradients;
  (c) gnx_block_backward_typed(GNX_ELEM_BF16), native path.

The forms alternate window by window in one process; each window is timed with device events over >= --window seconds of device time after
warm-up; the medians and every window are recorded.  (c)'s outputs are checked bit for bit against (b)'s on the timed buffers.

With --parent-lib, form (a) is also timed against another build of the library (the parent commit's), `--ab-rounds` fresh child processes
of each, alternating, before this process opens the GPU: the fp32 instantiations are meant to be the same code.

  python tools/time_bf16_backward.py [--windows 7] [--window 0.2] [--parent-lib libgnx_parent.so] [--out profiles/bf16_backward_c2.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIMS, OUT = (10, 5, 0), (3, 4, 5)
TYPED = ("gnx_block_backward_typed_workspace_bytes", "gnx_block_backward_typed")


def timed_windows(torch, forms, windows, window_s):
    """forms: {key: callable}; returns {key: [ms per call of each window]} and the calls per window"""
    steps, ms = {}, {k: [] for k in forms}
    for key, f in forms.items():
        for _ in range(10):
            f()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            f()
        e1.record()
        torch.cuda.synchronize()
        steps[key] = max(20, int(window_s * 1e3 / (e0.elapsed_time(e1) / 20)) + 1)
    for _ in range(windows):
        for key, f in forms.items():  # alternate the forms window by window
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps[key]):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms[key].append(e0.elapsed_time(e1) / steps[key])
    return ms, steps


def summary(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), window_ms=[round(x, 5) for x in ms])


def run(a, fp32_only):
    import torch
    import graphnets_jl_amd as gn
    if fp32_only:  # (a build of the parent commit has no typed backward)
        for n in TYPED:
            gn._lib.SIGNATURES.pop(n, None)
    from oracle import gn_oracle as O
    from tests import util as U
    lib, L = gn._lib.load(), gn._lib
    torch.cuda.set_device(0)
    colptr, rowval = U.er_csc(np.random.default_rng(0), 100_000, 1_000_000)
    g = gn.GNGraphBatch.from_csc([colptr], [rowval], [100_000])
    rng = np.random.default_rng(0)
    blk = U.block_from_params(gn, O.make_block_params(rng, DIMS, OUT, act=(1, 2, 0)))
    keep = []
    p = blk._c(keep)
    s = torch.cuda.current_stream().cuda_stream
    rows = (g.n_edges, g.n_nodes, g.n_graphs)
    ptr = lambda t: None if t is None else t.data_ptr()
    rnd = lambda T, d: torch.from_numpy((rng.random((1, T, d), dtype=np.float32) * 4 - 2)).cuda()
    ins16 = [rnd(g.n_edges, 10).to(torch.bfloat16), rnd(g.n_nodes, 5).to(torch.bfloat16), None]
    cot16 = [torch.from_numpy(rng.standard_normal((1, T, d)).astype(np.float32)).cuda().to(torch.bfloat16) for T, d in zip(rows, OUT)]
    # forward outputs: bf16 from the typed forward; the fp32 form gets the fp32 forward of the same (widened) inputs
    ins32 = [None if t is None else t.float() for t in ins16]
    outs32 = [torch.empty((1, T, d), dtype=torch.float32, device="cuda") for T, d in zip(rows, OUT)]
    ws = torch.empty(int(lib.gnx_block_workspace_bytes(g._h, C.byref(p), 1)), dtype=torch.uint8, device="cuda")
    assert lib.gnx_block_forward(g._h, C.byref(p), *map(ptr, ins32), 1, *map(ptr, outs32), ws.data_ptr(), ws.numel(), 0, s) == 0, lib.gnx_last_error()
    torch.cuda.synchronize()
    outs16 = [t.to(torch.bfloat16) for t in outs32]  # (bit for bit what gnx_block_forward_typed stores: tests/test_gpu_bf16_block.py)
    cot32 = [t.float() for t in cot16]
    layers = (blk.edgefn, blk.nodefn, blk.graphfn)

    def outputs(dt):
        d = [torch.empty((1, T, w), dtype=dt, device="cuda") if w else None for T, w in zip(rows, DIMS)]
        gs = [t for l in layers for t in (torch.empty((l.weight.shape[1], l.weight.shape[0]), device="cuda"), torch.empty_like(l.bias))]
        return d, gs, L.BlockGrads(*[L.DenseGrad(gs[2 * i].data_ptr(), gs[2 * i + 1].data_ptr()) for i in range(3)])

    nb32 = int(lib.gnx_block_backward_workspace_bytes(g._h, C.byref(p), 1))
    ws32 = torch.empty(nb32, dtype=torch.uint8, device="cuda")
    d_a, g_a, gr_a = outputs(torch.float32)
    nine_a = ins32 + outs32 + cot32

    def form_a():
        assert lib.gnx_block_backward(g._h, C.byref(p), *map(ptr, nine_a), 1, *map(ptr, d_a), C.byref(gr_a), ws32.data_ptr(), nb32, s) == 0

    forms = {"a_fp32": form_a}
    if not fp32_only:
        d_b32, g_b, gr_b = outputs(torch.float32)
        nine_16 = ins16 + outs16 + cot16
        held = {}

        def form_b():
            wide = [None if t is None else t.float() for t in nine_16]
            assert lib.gnx_block_backward(g._h, C.byref(p), *map(ptr, wide), 1, *map(ptr, d_b32), C.byref(gr_b), ws32.data_ptr(), nb32, s) == 0
            held["d"] = [None if t is None else t.to(torch.bfloat16) for t in d_b32]

        nb16 = int(lib.gnx_block_backward_typed_workspace_bytes(g._h, C.byref(p), 1, L.ELEM_BF16))
        ws16 = torch.empty(nb16, dtype=torch.uint8, device="cuda")
        d_c, g_c, gr_c = outputs(torch.bfloat16)

        def form_c():
            assert lib.gnx_block_backward_typed(g._h, C.byref(p), L.ELEM_BF16, *map(ptr, nine_16), 1, *map(ptr, d_c), C.byref(gr_c), ws16.data_ptr(), nb16,
                                                s) == 0

        forms.update(b_torch_casts_around_fp32=form_b, c_typed_bf16=form_c)
    ms, steps = timed_windows(torch, forms, a.windows, a.window)
    res = dict(device=torch.cuda.get_device_name(0), library=os.path.basename(gn._lib.LIB_PATH), E=g.n_edges, N=g.n_nodes, G=g.n_graphs,
               dims="(10,5,0)=>(3,4,5)", act="relu/tanh/identity", windows=a.windows, calls_per_window=steps, forms={k: summary(v) for k, v in ms.items()})
    if not fp32_only:
        torch.cuda.synchronize()
        same = all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(held["d"], d_c) if x is not None)
        same = same and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(g_b, g_c))
        b, c = res["forms"]["b_torch_casts_around_fp32"], res["forms"]["c_typed_bf16"]
        feat = lambda nbytes: sum(t.numel() for t in nine_16 + d_c if t is not None) * nbytes
        res.update(c_bit_identical_to_b=bool(same), c_over_b=c["median_ms"] / b["median_ms"], c_over_a=c["median_ms"] / res["forms"]["a_fp32"]["median_ms"],
                   c_not_slower_than_b=bool(c["median_ms"] <= b["median_ms"]), workspace_bytes=dict(fp32=nb32, typed_bf16=nb16),
                   feature_tensor_bytes=dict(fp32=feat(4), bf16=feat(2)))
    return res


def ab_fp32(a):
    """form (a) in fresh child processes, the parent build and this build alternating"""
    rounds = []
    for r in range(a.ab_rounds):
        for tag, path in (("parent", os.path.abspath(a.parent_lib)), ("this", None)):
            env = dict(os.environ)
            env.pop("GNX_LIB_PATH", None)
            if path:
                env["GNX_LIB_PATH"] = path
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--fp32-only", "--windows", str(a.windows), "--window", str(a.window)],
                                 env=env, stdout=subprocess.PIPE, timeout=600, check=True).stdout.decode()
            f = json.loads(out.strip().splitlines()[-1])["forms"]["a_fp32"]
            rounds.append(dict(round=r, build=tag, median_ms=f["median_ms"], min_ms=f["min_ms"], max_ms=f["max_ms"]))
            print(f"A/B round {r} {tag}: {f['median_ms']:.4f} ms", flush=True)
    med = {t: [x["median_ms"] for x in rounds if x["build"] == t] for t in ("parent", "this")}
    spread = max(med["parent"]) - min(med["parent"])
    diff = float(np.median(med["this"]) - np.median(med["parent"]))
    return dict(runs=rounds, parent_median_ms=float(np.median(med["parent"])), this_median_ms=float(np.median(med["this"])),
                parent_spread_ms=spread, this_minus_parent_ms=diff, within_parent_spread=bool(abs(diff) <= spread))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of device time per window")
    ap.add_argument("--fp32-only", action="store_true", help="form (a) alone (also runs on a build without the typed backward)")
    ap.add_argument("--parent-lib", default=None, help="another build of libgnx.so to time form (a) against")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ab = ab_fp32(a) if a.parent_lib and not a.fp32_only else None  # (children first: this process has not opened the GPU yet)
    res = run(a, a.fp32_only)
    if ab is not None:
        res["fp32_parent_vs_this_build"] = ab
    if not a.fp32_only:
        f = res["forms"]
        print(f"(a) fp32 {f['a_fp32']['median_ms']:.4f} ms   (b) torch casts + fp32 {f['b_torch_casts_around_fp32']['median_ms']:.4f} ms   "
              f"(c) typed bf16 {f['c_typed_bf16']['median_ms']:.4f} ms   c/b {res['c_over_b']:.3f}   bit-identical {res['c_bit_identical_to_b']}")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    if not a.fp32_only and not (res["c_not_slower_than_b"] and res["c_bit_identical_to_b"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
