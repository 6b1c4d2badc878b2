"""Times gnx_block_backward_narrow at width sets OUTSIDE the five ahead-of-time ones — the fused edge level in the run-time specialised
k_bw_edge_wave — against what those sets ran before the entry existed: gnx_block_backward (fp32) / gnx_block_backward_typed (bf16), the generic
edge level.  Every gradient is requested, on the 1M-edge graph (BASELINE configs[1], "C2").  Width sets (de, dn, dg) => (oe, 4, 5):

  (3,2,4)=>3     36 weight-gradient pairs, one slot per lane
  (6,6,3)=>3     66 pairs and (2,3,1)=>7: 70 pairs — two slots per lane
  (20,10,4)=>1   oe = 1 with Ke = 44: the LDS-heavy pair loop (47 KB of LDS, three waves per SIMD)
  (20,16,10)=>1  Ke = 62: the widest eligible rows (64 KB of LDS, two waves per SIMD; fp32 only — at on = 4 the bf16 call's node level is on the
                 matrix cores, the typed call stages and the narrow call does not apply)

in fp32 and bf16.  The two forms alternate window by window in one process (tools/time_bw_fused.py: timed_windows); medians, every window, the
workspace sizes, the profiler's per-kernel breakdown of one call of each form, and a check that the input gradients and the node / graph
parameter gradients of the two forms are the same bits are recorded.  `not_slower_beyond_spread`: narrow median <= generic median + the
generic form's spread (max - min over its windows) — the rule a class of width sets has to meet to stay eligible.

  python tools/time_bw_narrow.py [--windows 7] [--window 0.2] [--out profiles/bw_narrow_c2.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.time_bw_fused import summary, timed_windows  # noqa: E402

SETS = (((3, 2, 4), 3), ((6, 6, 3), 3), ((2, 3, 1), 7), ((20, 10, 4), 1), ((20, 16, 10), 1))


def one_case(a, gn, g, dims, oe, bf16):
    import torch
    from oracle import gn_oracle as O
    from tests import util as U
    lib, L = gn._lib.load(), gn._lib
    elem = L.ELEM_BF16 if bf16 else L.ELEM_F32
    dt = torch.bfloat16 if bf16 else torch.float32
    out = (oe, 4, 5)
    rng = np.random.default_rng(0)
    blk = U.block_from_params(gn, O.make_block_params(rng, dims, out, act=(1, 2, 0)))
    keep = []
    p = blk._c(keep)
    s = torch.cuda.current_stream().cuda_stream
    rows = (g.n_edges, g.n_nodes, g.n_graphs)
    ptr = lambda t: None if t is None else t.data_ptr()
    rnd = lambda T, d: torch.from_numpy((rng.random((1, T, d), dtype=np.float32) * 4 - 2)).cuda().to(dt) if d else None
    ins = [rnd(T, d) for T, d in zip(rows, dims)]
    cot = [torch.from_numpy(rng.standard_normal((1, T, d)).astype(np.float32)).cuda().to(dt) for T, d in zip(rows, out)]
    outs = [torch.empty((1, T, d), dtype=dt, device="cuda") for T, d in zip(rows, out)]
    ws = torch.empty(int(lib.gnx_block_typed_workspace_bytes(g._h, C.byref(p), 1, elem, 0)), dtype=torch.uint8, device="cuda")
    assert lib.gnx_block_forward_typed(g._h, C.byref(p), elem, *map(ptr, ins), 1, *map(ptr, outs), ws.data_ptr(), ws.numel(), 0, s) == 0, lib.gnx_last_error()
    torch.cuda.synchronize()
    nine = ins + outs + cot
    layers = (blk.edgefn, blk.nodefn, blk.graphfn)

    def outputs():
        d = [torch.empty((1, T, w), dtype=dt, device="cuda") if w else None for T, w in zip(rows, dims)]
        gs = [t for l in layers for t in (torch.empty((l.weight.shape[1], l.weight.shape[0]), device="cuda"), torch.empty_like(l.bias))]
        return d, gs, L.BlockGrads(*[L.DenseGrad(gs[2 * i].data_ptr(), gs[2 * i + 1].data_ptr()) for i in range(3)])

    label = f"{tuple(dims)}=>{out} {'bf16' if bf16 else 'fp32'}"
    if lib.gnx_block_backward_narrow_applies(g._h, C.byref(p), 1, elem) != 1:  # (bf16 with the node level on the matrix cores: the typed call stages)
        return dict(label=label, applies=False)
    nb_g = int(lib.gnx_block_backward_typed_workspace_bytes(g._h, C.byref(p), 1, elem))
    nb_n = int(lib.gnx_block_backward_narrow_workspace_bytes(g._h, C.byref(p), 1, elem))
    ws_g, ws_n = torch.empty(nb_g, dtype=torch.uint8, device="cuda"), torch.empty(nb_n, dtype=torch.uint8, device="cuda")
    d_g, g_g, gr_g = outputs()
    d_n, g_n, gr_n = outputs()

    def generic():
        assert lib.gnx_block_backward_typed(g._h, C.byref(p), elem, *map(ptr, nine), 1, *map(ptr, d_g), C.byref(gr_g), ws_g.data_ptr(), nb_g, s) == 0

    def narrow():
        assert lib.gnx_block_backward_narrow(g._h, C.byref(p), elem, *map(ptr, nine), 1, *map(ptr, d_n), C.byref(gr_n), ws_n.data_ptr(), nb_n, s) == 0

    ms, steps = timed_windows(torch, {"generic": generic, "narrow": narrow}, a.windows, a.window)
    torch.cuda.synchronize()
    raw = lambda x: x.contiguous().view(-1).view(torch.uint8)
    same = all(torch.equal(raw(x), raw(y)) for x, y in zip(d_g, d_n) if x is not None) and all(torch.equal(raw(x), raw(y)) for x, y in zip(g_g[2:], g_n[2:]))
    edge_err = [float((x.double() - y.double()).abs().max() / max(1.0, float(x.double().abs().max()))) for x, y in zip(g_g[:2], g_n[:2])]
    prof = {}
    for key, f in (("generic", generic), ("narrow", narrow)):
        gn.profile_reset(); gn.profile_enable(True)
        try:
            f()
            torch.cuda.synchronize()
        finally:
            gn.profile_enable(False)
        prof[key] = {n: dict(kernels=v["kernels"], total_ms=round(v["total_ms"], 5)) for n, v in sorted(gn.profile_read().items())}
        gn.profile_reset()
    res = {k: summary(v) for k, v in ms.items()}
    gen, nar = res["generic"], res["narrow"]
    return dict(label=label, E=g.n_edges, N=g.n_nodes, G=g.n_graphs, elem="bf16" if bf16 else "fp32", dims=f"{tuple(dims)}=>{out}", act="relu/tanh/identity",
                calls_per_window=steps, forms=res, narrow_over_generic=nar["median_ms"] / gen["median_ms"], saved_ms=gen["median_ms"] - nar["median_ms"],
                not_slower_beyond_spread=bool(nar["median_ms"] <= gen["median_ms"] + gen["spread_ms"]),
                input_and_node_graph_gradients_bit_identical=bool(same), edge_gradient_max_diff_over_scale=dict(dWe=edge_err[0], dbe=edge_err[1]),
                workspace_bytes=dict(generic=nb_g, narrow=nb_n), profiler_one_call=prof)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of device time per window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), windows=a.windows, window_s=a.window, cases=[])
    c2 = gn.GNGraphBatch.from_csc(*bench.make_c2())
    for dims, oe in SETS:
        for bf16 in (False, True):
            c = one_case(a, gn, c2, dims, oe, bf16)
            res["cases"].append(c)
            if not c.get("applies", True):
                print(f"{c['label']}: the narrow call does not apply", flush=True)
                continue
            f = c["forms"]
            print(f"{c['label']}: generic {f['generic']['median_ms']:.4f} ms (spread {f['generic']['spread_ms']:.4f})   narrow {f['narrow']['median_ms']:.4f} ms   "
                  f"ratio {c['narrow_over_generic']:.3f}   ws {c['workspace_bytes']['narrow'] / 2**20:.0f} / {c['workspace_bytes']['generic'] / 2**20:.0f} MiB   "
                  f"bits {c['input_and_node_graph_gradients_bit_identical']}", flush=True)
            if a.out:  # (after every case: a run cut short leaves what it measured)
                with open(a.out, "w") as fh:
                    json.dump(res, fh, indent=1)
    if not all(c.get("input_and_node_graph_gradients_bit_identical", True) for c in res["cases"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
