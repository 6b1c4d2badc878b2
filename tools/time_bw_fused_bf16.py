"""Times the fused narrow edge pullback on bfloat16 features, gnx_block_backward_fused_typed(GNX_ELEM_BF16), with every gradient requested,
against the two calls it joins:

  typed        gnx_block_backward_typed(GNX_ELEM_BF16) on the same bf16 tensors — what a block with both switches ran before
  fused_fp32   gnx_block_backward_fused on fp32 tensors (its own fp32 forward)

on

  c2        the 1M-edge graph (BASELINE configs[1]) at (10,5,0) => (3,4,5)
  c2_345    the 1M-edge graph at (3,4,5) => (3,4,5)
  c3        the 512-graph batch of 1M edges (BASELINE configs[2]) at (10,5,0) => (3,4,5)

The forms alternate window by window in one process (tools/timing.py's windows: device events over >= --window seconds of device time
after warm-up); the medians and every window are recorded, and whether the new call is faster than the typed call by more than the spread
(max - min over the windows) of the typed call.  Per case: the three workspace sizes, the per-kernel profiler breakdown of one call of each
form, and the contract of the new call on this data — d_ef / d_nf / d_gf and the node / graph parameter gradients are the typed call's bits,
dWe / dbe the bits of gnx_block_backward_fused on the widened tensors.  The compiler's resource remarks of the ten instantiations of the
kernel (VGPRs, LDS, waves per SIMD, scratch; fp32 and bf16 side by side) are read when hipcc is present.

--fp32-only runs the fused_fp32 leg alone and touches no entry point younger than gnx_block_backward_fused: the same file measures that leg
on an older build of the library (the fp32 kernel must not have moved).

--resources-json PATH keeps the resource remarks in a file: read from it when it exists, else written to it (the compiler then need not run
again next to the timing).

  python tools/time_bw_fused_bf16.py [--windows 7] [--window 0.2] [--fp32-only] [--resources-json PATH] [--out profiles/bw_fused_bf16_c2.json]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import calls, timing  # noqa: E402
from tools.kernel_resources import HIPCC  # noqa: E402

OUT = (3, 4, 5)
TIMING = dict(warmup=10, probe=20, min_calls=20)
CASES = (("C2", (10, 5, 0), "c2"), ("C2", (3, 4, 5), "c2_345"), ("hetero512", (10, 5, 0), "c3"))  # (graph, input widths, label)
CONTRACT = ("input_and_node_graph_gradients_bits_of_typed", "edge_gradients_bits_of_fused_fp32_on_widened", "input_gradients_are_rounded_fused_fp32_on_widened")


def resources():
    """{"(de, dn, dg, oe)": {"fp32": {...}, "bf16": {...}}} of k_bw_edge_wave / k_bw_edge_wave_bf16 in gnx_backward_narrow.hip, compiled as build.py
    compiles it (tools/kernel_resources.py)"""
    from tools.kernel_resources import pick, remarks
    return pick("bw_narrow", remarks("gnx_backward_narrow.hip"))


def one_case(a, gn, g, dims, label):
    import torch
    F32, BF = gn._lib.ELEM_F32, gn._lib.ELEM_BF16
    case = calls.block_case(gn, g, dims, OUT, act=(1, 2, 0))
    # fp32 leg: its own fp32 forward
    fw = calls.build(gn, case, "block", "forward", F32, "gnx_block_forward")
    fw.f()
    torch.cuda.synchronize()
    assert calls.applies(gn, case, "gnx_block_backward_fused_applies") == 1, label
    f32 = calls.build(gn, case, "block", "backward", F32, "gnx_block_backward_fused", fwd=fw.outs)
    built = {"fused_fp32": f32}
    if not a.fp32_only:
        x16 = [None if t is None else t.bfloat16() for t in case.x]
        cot16 = [t.bfloat16() for t in case.cot]
        fw16 = calls.build(gn, case, "block", "forward", BF, "gnx_block_forward_typed", x=x16)
        fw16.f()
        torch.cuda.synchronize()
        assert calls.applies(gn, case, "gnx_block_backward_fused_typed_applies", BF) == 1, label
        on16 = dict(x=x16, cot=cot16, fwd=fw16.outs)
        ws = [calls.workspace(gn, case, "block", "backward", BF, name) for name in ("gnx_block_backward_typed", "gnx_block_backward_fused_typed")]  # both first
        typ = calls.build(gn, case, "block", "backward", BF, "gnx_block_backward_typed", ws=ws[0], **on16)
        new = calls.build(gn, case, "block", "backward", BF, "gnx_block_backward_fused_typed", ws=ws[1], **on16)
        built = {"fused_bf16": new, "typed": typ, "fused_fp32": f32}
    forms = {k: c.f for k, c in built.items()}
    ms, steps = timing.timed_windows(torch, forms, a.windows, a.window, **TIMING)
    torch.cuda.synchronize()
    res = {k: timing.summary_windows(v) for k, v in ms.items()}
    out = dict(label=label, E=g.n_edges, N=g.n_nodes, G=g.n_graphs, dims=f"{tuple(dims)}=>{OUT}", act="relu/tanh/identity", calls_per_window=steps, forms=res,
               workspace_bytes={k: c.nbytes for k, c in built.items()}, profiler_one_call={k: timing.profiled_once(gn, torch, f) for k, f in forms.items()})
    if not a.fp32_only:
        bits = lambda x, y: x.dtype == y.dtype and torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                                                               y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32))
        same = all(bits(x, y) for x, y in zip(typ.outs, new.outs) if x is not None) and all(bits(x, y) for x, y in zip(typ.grads[2:], new.grads[2:]))
        # dWe / dbe: gnx_block_backward_fused on the exactly widened bf16 tensors
        widen = lambda ts: [None if t is None else t.float() for t in ts]
        wide = calls.build(gn, case, "block", "backward", F32, "gnx_block_backward_fused", x=widen(x16), cot=widen(cot16), fwd=widen(fw16.outs), ws=f32.ws)
        wide.f()
        torch.cuda.synchronize()
        edge = all(bits(x, y) for x, y in zip(wide.grads[:2], new.grads[:2]))
        rounded = all(bits(x.bfloat16(), y) for x, y in zip(wide.outs, new.outs) if x is not None)
        n_, t_, f_ = res["fused_bf16"], res["typed"], res["fused_fp32"]
        out.update(fused_bf16_over_typed=n_["median_ms"] / t_["median_ms"], fused_bf16_over_fused_fp32=n_["median_ms"] / f_["median_ms"],
                   saved_ms=t_["median_ms"] - n_["median_ms"],
                   faster_than_typed_by_more_than_the_typed_spread=bool(t_["median_ms"] - n_["median_ms"] > t_["spread_ms"]),
                   at_or_below_fused_fp32=bool(n_["median_ms"] <= f_["median_ms"]),
                   input_and_node_graph_gradients_bits_of_typed=bool(same), edge_gradients_bits_of_fused_fp32_on_widened=bool(edge),
                   input_gradients_are_rounded_fused_fp32_on_widened=bool(rounded))
    return out


def run(a, kres="not measured", graphs=None, limit=None):
    """the record; graphs: {key: GNGraphBatch} in place of the full-size ones, limit: the first cases only (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    out = timing.RecordWriter(a.out, device=torch.cuda.get_device_name(0), windows=a.windows, window_s=a.window, timing=timing.windows_timing(a, **TIMING),
                              fp32_only=a.fp32_only, kernel_resources=kres, cases=[])
    get = timing.OneGraph(gn, graphs)
    for key, dims, label in CASES[:limit]:
        out.add("cases", one_case(a, gn, get(key), dims, label))
    return out.res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of device time per window")
    ap.add_argument("--fp32-only", action="store_true", help="the gnx_block_backward_fused leg alone (also runs on a build without the typed fused call)")
    ap.add_argument("--resources-json", default=None, help="the kernels' resource remarks: read from this file if it exists, else written to it")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    try:  # (the compiler runs before this process opens the GPU)
        kres = timing.read_record(a.resources_json)
        if not kres:
            kres = resources() if os.path.exists(HIPCC) else "not measured (no hipcc)"
            if a.resources_json and isinstance(kres, dict):
                timing.RecordWriter(a.resources_json, **kres).write()
    except Exception as e:  # the timing stands without it
        kres = f"not measured ({type(e).__name__})"
    res = run(a, kres)
    for c in res["cases"]:
        print(f"{c['label']}: " + "   ".join(f"{k} {v['median_ms']:.4f} ms (spread {v['spread_ms']:.4f})" for k, v in c["forms"].items()))
    timing.print_record(res)
    if not a.fp32_only and not all(c[k] for c in res["cases"] for k in CONTRACT):
        sys.exit(1)


if __name__ == "__main__":
    main()
