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
import ctypes as C
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = (3, 4, 5)


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
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), spread_ms=float(max(ms) - min(ms)),
                window_ms=[round(x, 5) for x in ms])


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
    from oracle import gn_oracle as O
    from tests import util as U
    lib, L = gn._lib.load(), gn._lib
    rng = np.random.default_rng(0)
    blk = U.block_from_params(gn, O.make_block_params(rng, dims, OUT, act=(1, 2, 0)))
    keep = []
    p = blk._c(keep)
    s = torch.cuda.current_stream().cuda_stream
    rows = (g.n_edges, g.n_nodes, g.n_graphs)
    ptr = lambda t: None if t is None else t.data_ptr()
    rnd = lambda T, d: torch.from_numpy((rng.random((1, T, d), dtype=np.float32) * 4 - 2)).cuda() if d else None
    ins = [rnd(T, d) for T, d in zip(rows, dims)]
    cot = [torch.from_numpy(rng.standard_normal((1, T, d)).astype(np.float32)).cuda() for T, d in zip(rows, OUT)]
    outs = [torch.empty((1, T, d), dtype=torch.float32, device="cuda") for T, d in zip(rows, OUT)]
    ws = torch.empty(int(lib.gnx_block_workspace_bytes(g._h, C.byref(p), 1)), dtype=torch.uint8, device="cuda")
    assert lib.gnx_block_forward(g._h, C.byref(p), *map(ptr, ins), 1, *map(ptr, outs), ws.data_ptr(), ws.numel(), 0, s) == 0, lib.gnx_last_error()
    torch.cuda.synchronize()
    nine = ins + outs + cot
    layers = (blk.edgefn, blk.nodefn, blk.graphfn)

    def outputs():
        d = [torch.empty((1, T, w), dtype=torch.float32, device="cuda") if w else None for T, w in zip(rows, dims)]
        gs = [t for l in layers for t in (torch.empty((l.weight.shape[1], l.weight.shape[0]), device="cuda"), torch.empty_like(l.bias))]
        return d, gs, L.BlockGrads(*[L.DenseGrad(gs[2 * i].data_ptr(), gs[2 * i + 1].data_ptr()) for i in range(3)])

    assert lib.gnx_block_backward_fused_applies(g._h, C.byref(p), 1) == 1, label
    nb_g = int(lib.gnx_block_backward_workspace_bytes(g._h, C.byref(p), 1))
    nb_f = int(lib.gnx_block_backward_fused_workspace_bytes(g._h, C.byref(p), 1))
    ws_g, ws_f = torch.empty(nb_g, dtype=torch.uint8, device="cuda"), torch.empty(nb_f, dtype=torch.uint8, device="cuda")
    d_g, g_g, gr_g = outputs()
    d_f, g_f, gr_f = outputs()

    def generic():
        assert lib.gnx_block_backward(g._h, C.byref(p), *map(ptr, nine), 1, *map(ptr, d_g), C.byref(gr_g), ws_g.data_ptr(), nb_g, s) == 0

    def fused():
        assert lib.gnx_block_backward_fused(g._h, C.byref(p), *map(ptr, nine), 1, *map(ptr, d_f), C.byref(gr_f), ws_f.data_ptr(), nb_f, s) == 0

    ms, steps = timed_windows(torch, {"generic": generic, "fused": fused}, a.windows, a.window)
    torch.cuda.synchronize()
    bits = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))
    same = all(bits(x, y) for x, y in zip(d_g, d_f) if x is not None) and all(bits(x, y) for x, y in zip(g_g[2:], g_f[2:]))
    edge_err = [float((x.double() - y.double()).abs().max() / max(1.0, float(x.double().abs().max()))) for x, y in zip(g_g[:2], g_f[:2])]
    prof = {}
    for key, f in (("generic", generic), ("fused", fused)):
        gn.profile_reset(); gn.profile_enable(True)
        try:
            f()
            torch.cuda.synchronize()
        finally:
            gn.profile_enable(False)
        prof[key] = {n: dict(kernels=v["kernels"], total_ms=round(v["total_ms"], 5)) for n, v in sorted(gn.profile_read().items())}
        gn.profile_reset()
    res = {k: summary(v) for k, v in ms.items()}
    gen, fus = res["generic"], res["fused"]
    return dict(label=label, E=g.n_edges, N=g.n_nodes, G=g.n_graphs, dims=f"{tuple(dims)}=>{OUT}", act="relu/tanh/identity", calls_per_window=steps, forms=res,
                fused_over_generic=fus["median_ms"] / gen["median_ms"], saved_ms=gen["median_ms"] - fus["median_ms"],
                faster_by_more_than_the_generic_spread=bool(gen["median_ms"] - fus["median_ms"] > gen["spread_ms"]),
                input_and_node_graph_gradients_bit_identical=bool(same), edge_gradient_max_diff_over_scale=dict(dWe=edge_err[0], dbe=edge_err[1]),
                workspace_bytes=dict(generic=nb_g, fused=nb_f), profiler_one_call=prof)


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
    import torch
    import bench
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), windows=a.windows, window_s=a.window, kernel_resources=kres, cases=[])
    c2 = gn.GNGraphBatch.from_csc(*bench.make_c2())
    res["cases"].append(one_case(a, gn, c2, (10, 5, 0), "c2"))
    res["cases"].append(one_case(a, gn, c2, (3, 4, 5), "c2_345"))
    del c2
    c3 = gn.GNGraphBatch.from_csc(*bench.make_hetero(3))
    res["cases"].append(one_case(a, gn, c3, (10, 5, 0), "c3"))
    for c in res["cases"]:
        f = c["forms"]
        print(f"{c['label']}: generic {f['generic']['median_ms']:.4f} ms (spread {f['generic']['spread_ms']:.4f})   fused {f['fused']['median_ms']:.4f} ms   "
              f"ratio {c['fused_over_generic']:.3f}   bits {c['input_and_node_graph_gradients_bit_identical']}")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    if not all(c["input_and_node_graph_gradients_bit_identical"] for c in res["cases"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
