"""Times gnx_block_backward (the generic edge level) against gnx_block_backward_fused (the edge level in k_bw_edge_wave) with every gradient
requested, on

  c2        the 1M-edge graph (BASELINE configs[1]) at (10,5,0) => (3,4,5)
  c3        the 512-graph batch of 1M edges (BASELINE configs[2]) at (10,5,0) => (3,4,5)
  c2_345    the 1M-edge graph at (3,4,5) => (3,4,5)

The two forms alternate window by window in one process; each window is timed with device events over >= --window seconds of device time after
warm-up; the medians and every window are recorded, and whether the fused call is faster by more than the spread (max - min over the windows) of
the generic call.  Per case: the per-kernel profiler breakdown of both forms (gnx_profile_*, one profiled call each after the timing), the two
workspace sizes, and a check that the fused input gradients and node / graph parameter gradients are the generic call's bits.  The compiler's
resource remarks of the five instantiations (registers, LDS, scratch) are read when hipcc is present (tools/kernel_resources.py).

  python tools/time_bw_fused.py [--windows 7] [--window 0.2] [--out profiles/bw_fused_c2.json]
"""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import calls, timing  # noqa: E402

OUT = (3, 4, 5)
TIMING = dict(warmup=10, probe=20, min_calls=20)
CASES = (("C2", (10, 5, 0), "c2"), ("C2", (3, 4, 5), "c2_345"), ("hetero512", (10, 5, 0), "c3"))  # (graph, input widths, label)


def kernel_resources():
    """{"(de, dn, dg, oe)": {sgpr, vgpr, scratch, lds, occupancy}} of the five k_bw_edge_wave instantiations of gnx_backward_narrow.hip"""
    from tools.kernel_resources import remarks
    res = {}
    for name, r in remarks("gnx_backward_narrow.hip").items():
        m = re.match(r"_ZN3gnx14k_bw_edge_waveILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEEv", name)
        if m:
            res[tuple(int(v) for v in m.groups())] = dict(sgpr=r["sgpr"], vgpr=r["vgpr"], scratch=r["scratch"], lds=r["lds"], occupancy=r["waves_per_simd"])
    return {str(k): v for k, v in sorted(res.items())}


def one_case(a, gn, g, dims, label):
    import torch
    F32 = gn._lib.ELEM_F32
    case = calls.block_case(gn, g, dims, OUT, act=(1, 2, 0))
    fw = calls.build(gn, case, "block", "forward", F32, "gnx_block_forward")
    fw.f()
    torch.cuda.synchronize()
    assert calls.applies(gn, case, "gnx_block_backward_fused_applies") == 1, label
    ws = [calls.workspace(gn, case, "block", "backward", F32, name) for name in ("gnx_block_backward", "gnx_block_backward_fused")]  # both first
    gen = calls.build(gn, case, "block", "backward", F32, "gnx_block_backward", fwd=fw.outs, ws=ws[0])
    fus = calls.build(gn, case, "block", "backward", F32, "gnx_block_backward_fused", fwd=fw.outs, ws=ws[1])
    forms = {"generic": gen.f, "fused": fus.f}
    ms, steps = timing.timed_windows(torch, forms, a.windows, a.window, **TIMING)
    torch.cuda.synchronize()
    bits = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))
    same = all(bits(x, y) for x, y in zip(gen.outs, fus.outs) if x is not None) and all(bits(x, y) for x, y in zip(gen.grads[2:], fus.grads[2:]))
    edge_err = [float((x.double() - y.double()).abs().max() / max(1.0, float(x.double().abs().max()))) for x, y in zip(gen.grads[:2], fus.grads[:2])]
    prof = {key: timing.profiled_once(gn, torch, f) for key, f in forms.items()}
    res = {k: timing.summary_windows(v) for k, v in ms.items()}
    g_, f_ = res["generic"], res["fused"]
    return dict(label=label, E=g.n_edges, N=g.n_nodes, G=g.n_graphs, dims=f"{tuple(dims)}=>{OUT}", act="relu/tanh/identity", calls_per_window=steps, forms=res,
                fused_over_generic=f_["median_ms"] / g_["median_ms"], saved_ms=g_["median_ms"] - f_["median_ms"],
                faster_by_more_than_the_generic_spread=bool(g_["median_ms"] - f_["median_ms"] > g_["spread_ms"]),
                input_and_node_graph_gradients_bit_identical=bool(same), edge_gradient_max_diff_over_scale=dict(dWe=edge_err[0], dbe=edge_err[1]),
                workspace_bytes=dict(generic=gen.nbytes, fused=fus.nbytes), profiler_one_call=prof)


def run(a, kres="not measured", graphs=None, limit=None):
    """the record; graphs: {key: GNGraphBatch} in place of the full-size ones, limit: the first cases only (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    out = timing.RecordWriter(a.out, device=torch.cuda.get_device_name(0), windows=a.windows, window_s=a.window, timing=timing.windows_timing(a, **TIMING),
                              kernel_resources=kres, cases=[])
    get = timing.OneGraph(gn, graphs)
    for key, dims, label in CASES[:limit]:
        out.add("cases", one_case(a, gn, get(key), dims, label))
    return out.res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of device time per window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    try:  # (the compiler runs before this process opens the GPU)
        from tools.kernel_resources import HIPCC
        kres = kernel_resources() if os.path.exists(HIPCC) else "not measured (no hipcc)"
    except Exception as e:  # the timing stands without it
        kres = f"not measured ({type(e).__name__})"
    res = run(a, kres)
    for c in res["cases"]:
        f = c["forms"]
        print(f"{c['label']}: generic {f['generic']['median_ms']:.4f} ms (spread {f['generic']['spread_ms']:.4f})   fused {f['fused']['median_ms']:.4f} ms   "
              f"ratio {c['fused_over_generic']:.3f}   bits {c['input_and_node_graph_gradients_bit_identical']}")
    timing.print_record(res)
    if not all(c["input_and_node_graph_gradients_bit_identical"] for c in res["cases"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
