"""Times the fused narrow edge pullback on bfloat16 features, gnx_block_backward_fused_typed(GNX_ELEM_BF16), with every gradient requested,
against the two calls it joins:

  typed        gnx_block_backward_typed(GNX_ELEM_BF16) on the same bf16 tensors — what a block with both switches ran before
  fused_fp32   gnx_block_backward_fused on fp32 tensors (its own fp32 forward)

on

  c2        the 1M-edge graph (BASELINE configs[1]) at (10,5,0) => (3,4,5)
  c2_345    the 1M-edge graph at (3,4,5) => (3,4,5)
  c3        the 512-graph batch of 1M edges (BASELINE configs[2]) at (10,5,0) => (3,4,5)

The forms alternate window by window in one process (tools/time_bw_fused.py's windows: device events over >= --window seconds of device time
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
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.kernel_resources import HIPCC  # noqa: E402
from tools.time_bw_fused import summary, timed_windows  # noqa: E402

OUT = (3, 4, 5)


def resources():
    """{"(de, dn, dg, oe)": {"fp32": {...}, "bf16": {...}}} of k_bw_edge_wave / k_bw_edge_wave_bf16 in gnx_backward_narrow.hip, compiled as build.py
    compiles it (tools/kernel_resources.py)"""
    from tools.kernel_resources import pick, remarks
    return pick("bw_narrow", remarks("gnx_backward_narrow.hip"))


def profiled(gn, torch, f):
    gn.profile_reset(); gn.profile_enable(True)
    try:
        f()
        torch.cuda.synchronize()
    finally:
        gn.profile_enable(False)
    out = {n: dict(kernels=v["kernels"], total_ms=round(v["total_ms"], 5)) for n, v in sorted(gn.profile_read().items())}
    gn.profile_reset()
    return out


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
    layers = (blk.edgefn, blk.nodefn, blk.graphfn)

    def outputs(dtype):
        d = [torch.empty((1, T, w), dtype=dtype, device="cuda") if w else None for T, w in zip(rows, dims)]
        gs = [t for l in layers for t in (torch.empty((l.weight.shape[1], l.weight.shape[0]), device="cuda"), torch.empty_like(l.bias))]
        return d, gs, L.BlockGrads(*[L.DenseGrad(gs[2 * i].data_ptr(), gs[2 * i + 1].data_ptr()) for i in range(3)])

    # fp32 leg: its own fp32 forward
    outs = [torch.empty((1, T, d), dtype=torch.float32, device="cuda") for T, d in zip(rows, OUT)]
    ws = torch.empty(int(lib.gnx_block_workspace_bytes(g._h, C.byref(p), 1)), dtype=torch.uint8, device="cuda")
    assert lib.gnx_block_forward(g._h, C.byref(p), *map(ptr, ins), 1, *map(ptr, outs), ws.data_ptr(), ws.numel(), 0, s) == 0, lib.gnx_last_error()
    torch.cuda.synchronize()
    nine = ins + outs + cot
    assert lib.gnx_block_backward_fused_applies(g._h, C.byref(p), 1) == 1, label
    nb_f = int(lib.gnx_block_backward_fused_workspace_bytes(g._h, C.byref(p), 1))
    ws_f = torch.empty(nb_f, dtype=torch.uint8, device="cuda")
    d_f, g_f, gr_f = outputs(torch.float32)

    def fused_fp32():
        assert lib.gnx_block_backward_fused(g._h, C.byref(p), *map(ptr, nine), 1, *map(ptr, d_f), C.byref(gr_f), ws_f.data_ptr(), nb_f, s) == 0

    forms = {"fused_fp32": fused_fp32}
    nbytes = dict(fused_fp32=nb_f)
    if not a.fp32_only:
        BF = L.ELEM_BF16
        ins16 = [None if t is None else t.bfloat16() for t in ins]
        cot16 = [t.bfloat16() for t in cot]
        outs16 = [torch.empty((1, T, d), dtype=torch.bfloat16, device="cuda") for T, d in zip(rows, OUT)]
        ws = torch.empty(int(lib.gnx_block_typed_workspace_bytes(g._h, C.byref(p), 1, BF, 0)), dtype=torch.uint8, device="cuda")
        assert lib.gnx_block_forward_typed(g._h, C.byref(p), BF, *map(ptr, ins16), 1, *map(ptr, outs16), ws.data_ptr(), ws.numel(), 0, s) == 0, lib.gnx_last_error()
        torch.cuda.synchronize()
        nine16 = ins16 + outs16 + cot16
        assert lib.gnx_block_backward_fused_typed_applies(g._h, C.byref(p), 1, BF) == 1, label
        nb_t = int(lib.gnx_block_backward_typed_workspace_bytes(g._h, C.byref(p), 1, BF))
        nb_n = int(lib.gnx_block_backward_fused_typed_workspace_bytes(g._h, C.byref(p), 1, BF))
        ws_t, ws_n = torch.empty(nb_t, dtype=torch.uint8, device="cuda"), torch.empty(nb_n, dtype=torch.uint8, device="cuda")
        d_t, g_t, gr_t = outputs(torch.bfloat16)
        d_n, g_n, gr_n = outputs(torch.bfloat16)

        def typed():
            assert lib.gnx_block_backward_typed(g._h, C.byref(p), BF, *map(ptr, nine16), 1, *map(ptr, d_t), C.byref(gr_t), ws_t.data_ptr(), nb_t, s) == 0

        def fused_bf16():
            assert lib.gnx_block_backward_fused_typed(g._h, C.byref(p), BF, *map(ptr, nine16), 1, *map(ptr, d_n), C.byref(gr_n), ws_n.data_ptr(), nb_n, s) == 0

        forms = {"fused_bf16": fused_bf16, "typed": typed, "fused_fp32": fused_fp32}
        nbytes = dict(fused_bf16=nb_n, typed=nb_t, fused_fp32=nb_f)
    ms, steps = timed_windows(torch, forms, a.windows, a.window)
    torch.cuda.synchronize()
    res = {k: summary(v) for k, v in ms.items()}
    out = dict(label=label, E=g.n_edges, N=g.n_nodes, G=g.n_graphs, dims=f"{tuple(dims)}=>{OUT}", act="relu/tanh/identity", calls_per_window=steps, forms=res,
               workspace_bytes=nbytes, profiler_one_call={k: profiled(gn, torch, f) for k, f in forms.items()})
    if not a.fp32_only:
        bits = lambda x, y: x.dtype == y.dtype and torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                                                               y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32))
        same = all(bits(x, y) for x, y in zip(d_t, d_n) if x is not None) and all(bits(x, y) for x, y in zip(g_t[2:], g_n[2:]))
        # dWe / dbe: gnx_block_backward_fused on the exactly widened bf16 tensors
        d_w, g_w, gr_w = outputs(torch.float32)
        wide = [None if t is None else t.float() for t in nine16]
        assert lib.gnx_block_backward_fused(g._h, C.byref(p), *map(ptr, wide), 1, *map(ptr, d_w), C.byref(gr_w), ws_f.data_ptr(), nb_f, s) == 0
        torch.cuda.synchronize()
        edge = all(bits(x, y) for x, y in zip(g_w[:2], g_n[:2]))
        rounded = all(bits(x.bfloat16(), y) for x, y in zip(d_w, d_n) if x is not None)
        new, typ, f32 = res["fused_bf16"], res["typed"], res["fused_fp32"]
        out.update(fused_bf16_over_typed=new["median_ms"] / typ["median_ms"], fused_bf16_over_fused_fp32=new["median_ms"] / f32["median_ms"],
                   saved_ms=typ["median_ms"] - new["median_ms"],
                   faster_than_typed_by_more_than_the_typed_spread=bool(typ["median_ms"] - new["median_ms"] > typ["spread_ms"]),
                   at_or_below_fused_fp32=bool(new["median_ms"] <= f32["median_ms"]),
                   input_and_node_graph_gradients_bits_of_typed=bool(same), edge_gradients_bits_of_fused_fp32_on_widened=bool(edge),
                   input_gradients_are_rounded_fused_fp32_on_widened=bool(rounded))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of device time per window")
    ap.add_argument("--fp32-only", action="store_true", help="the gnx_block_backward_fused leg alone (also runs on a build without the typed fused call)")
    ap.add_argument("--resources-json", default=None, help="the kernels' resource remarks: read from this file if it exists, else written to it")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    try:  # (the compiler runs before this process opens the GPU)
        if a.resources_json and os.path.exists(a.resources_json):
            with open(a.resources_json) as fh:
                kres = json.load(fh)
        else:
            kres = resources() if os.path.exists(HIPCC) else "not measured (no hipcc)"
            if a.resources_json and isinstance(kres, dict):
                with open(a.resources_json, "w") as fh:
                    json.dump(kres, fh, indent=1)
    except Exception as e:  # the timing stands without it
        kres = f"not measured ({type(e).__name__})"
    import torch
    import bench
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), windows=a.windows, window_s=a.window, fp32_only=a.fp32_only, kernel_resources=kres, cases=[])
    c2 = gn.GNGraphBatch.from_csc(*bench.make_c2())
    res["cases"].append(one_case(a, gn, c2, (10, 5, 0), "c2"))
    res["cases"].append(one_case(a, gn, c2, (3, 4, 5), "c2_345"))
    del c2
    c3 = gn.GNGraphBatch.from_csc(*bench.make_hetero(3))
    res["cases"].append(one_case(a, gn, c3, (10, 5, 0), "c3"))
    for c in res["cases"]:
        print(f"{c['label']}: " + "   ".join(f"{k} {v['median_ms']:.4f} ms (spread {v['spread_ms']:.4f})" for k, v in c["forms"].items()))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    keys = ("input_and_node_graph_gradients_bits_of_typed", "edge_gradients_bits_of_fused_fp32_on_widened", "input_gradients_are_rounded_fused_fp32_on_widened")
    if not a.fp32_only and not all(c[k] for c in res["cases"] for k in keys):
        sys.exit(1)


if __name__ == "__main__":
    main()
