"""Times the backward of one GNBlock at README widths (10,5,0) => (3,4,5) on the 1M-edge batch (BASELINE configs[1]) in three forms:

  (a) gnx_block_backward on fp32 tensors;
  (b) what a bf16 caller ran before gnx_block_backward_typed: torch .float() of the feature-shaped inputs, gnx_block_backward, torch
      .to(bfloat16) of the input gradients;
  (c) gnx_block_backward_typed(GNX_ELEM_BF16), native path.

The forms alternate window by window in one process; each window is timed with device events over >= --window seconds of device time after
warm-up (tools/timing.py: timed_windows); the medians and every window are recorded.  (c)'s outputs are checked bit for bit against (b)'s on
the timed buffers.

With --parent-lib, form (a) is also timed against another build of the library (the parent commit's), `--ab-rounds` fresh child processes
of each, alternating, before this process opens the GPU (tools/timing.py: library_rounds): the fp32 instantiations are meant to be the same code.

  python tools/time_bf16_backward.py [--windows 7] [--window 0.2] [--parent-lib libgnx_parent.so] [--out profiles/bf16_backward_c2.json]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import calls, timing  # noqa: E402

DIMS, OUT = (10, 5, 0), (3, 4, 5)
TYPED = ("gnx_block_backward_typed_workspace_bytes", "gnx_block_backward_typed")
TIMING = dict(warmup=10, probe=20, min_calls=20)


def run(a, fp32_only, g=None):
    """the record; g: a GNGraphBatch in place of the 1M-edge one (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    if fp32_only:  # (a build of the parent commit has no typed backward)
        for n in TYPED:
            gn._lib.SIGNATURES.pop(n, None)
    L = gn._lib
    torch.cuda.set_device(0)
    g = timing.er_1m(gn) if g is None else g
    BF = torch.bfloat16
    case = calls.block_case(gn, g, DIMS, OUT, act=(1, 2, 0), dtype=BF)  # (the bf16 tensors are the drawn ones; the fp32 forms get them widened)
    widen = lambda ts: [None if t is None else t.float() for t in ts]
    x32, cot32 = widen(case.x), widen(case.cot)
    # forward outputs: bf16 from the typed forward; the fp32 form gets the fp32 forward of the same (widened) inputs
    fw = calls.build(gn, case, "block", "forward", L.ELEM_F32, "gnx_block_forward", x=x32)
    fw.f()
    torch.cuda.synchronize()
    outs16 = [t.to(BF) for t in fw.outs]  # (bit for bit what gnx_block_forward_typed stores: tests/test_gpu_bf16_block.py)
    form_a = calls.build(gn, case, "block", "backward", L.ELEM_F32, "gnx_block_backward", x=x32, cot=cot32, fwd=fw.outs)
    forms = {"a_fp32": form_a.f}
    if not fp32_only:
        b32 = calls.build(gn, case, "block", "backward", L.ELEM_F32, "gnx_block_backward", x=x32, cot=cot32, fwd=fw.outs, ws=form_a.ws)
        nine_16 = case.x + outs16 + case.cot
        held = {}

        def form_b():
            wide = widen(nine_16)
            b32.f(x=wide[:3], cot=wide[6:], fwd=wide[3:6])
            held["d"] = [None if t is None else t.to(BF) for t in b32.outs]

        form_c = calls.build(gn, case, "block", "backward", L.ELEM_BF16, "gnx_block_backward_typed", fwd=outs16)
        forms.update(b_torch_casts_around_fp32=form_b, c_typed_bf16=form_c.f)
    ms, steps = timing.timed_windows(torch, forms, a.windows, a.window, **TIMING)
    res = dict(device=torch.cuda.get_device_name(0), library=os.path.basename(gn._lib.LIB_PATH), E=g.n_edges, N=g.n_nodes, G=g.n_graphs,
               dims="(10,5,0)=>(3,4,5)", act="relu/tanh/identity", windows=a.windows, timing=timing.windows_timing(a, **TIMING), calls_per_window=steps,
               forms={k: timing.summary_windows(v) for k, v in ms.items()})
    if not fp32_only:
        torch.cuda.synchronize()
        same = all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(held["d"], form_c.outs) if x is not None)
        same = same and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(b32.grads, form_c.grads))
        b, c = res["forms"]["b_torch_casts_around_fp32"], res["forms"]["c_typed_bf16"]
        feat = lambda nbytes: sum(t.numel() for t in nine_16 + form_c.outs if t is not None) * nbytes
        res.update(c_bit_identical_to_b=bool(same), c_over_b=c["median_ms"] / b["median_ms"], c_over_a=c["median_ms"] / res["forms"]["a_fp32"]["median_ms"],
                   c_not_slower_than_b=bool(c["median_ms"] <= b["median_ms"]), workspace_bytes=dict(fp32=form_a.nbytes, typed_bf16=form_c.nbytes),
                   feature_tensor_bytes=dict(fp32=feat(4), bf16=feat(2)))
    return res


def ab_fp32(a):
    """form (a) in fresh child processes, the parent build and this build alternating"""
    rounds = []
    recs = timing.library_rounds(__file__, (a.parent_lib, None), a.ab_rounds, ["--fp32-only", "--windows", a.windows, "--window", a.window], 600)
    for i, (key, rec) in enumerate(recs):
        f, tag = rec["forms"]["a_fp32"], "parent" if key == "parent" else "this"
        rounds.append(dict(round=i // 2, build=tag, median_ms=f["median_ms"], min_ms=f["min_ms"], max_ms=f["max_ms"]))
        print(f"A/B round {i // 2} {tag}: {f['median_ms']:.4f} ms", flush=True)
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
    timing.print_record(res)
    timing.RecordWriter(a.out, **res).write()
    if not a.fp32_only and not (res["c_not_slower_than_b"] and res["c_bit_identical_to_b"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
