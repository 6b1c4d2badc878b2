"""Times the block forward on fp32 features (gnx_block_forward) against bfloat16 features (gnx_block_forward_typed, GNX_ELEM_BF16) at
README dims (10,5,0) => (3,4,5), on the 1M-edge batch (BASELINE configs[1]) and on a batch of small graphs that takes the one-launch
pack form.  The two forms alternate in one process; each window is timed with device events over >= --window seconds after warm-up;
the median ms/step of the windows is printed with the algorithmic bytes of a step (feature rows in and out, source indices, colptr).

  python tools/time_bf16_block.py [--windows 7] [--window 0.2] [--out result.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def algorithmic_bytes(E, N, G, dims, out, elem_bytes):
    de, dn, dg = dims
    oe, on, og = out
    return E * ((de + oe) * elem_bytes + 4) + N * ((dn + on) * elem_bytes + 4) + G * (dg + og) * elem_bytes


def run_config(gn, torch, name, g, windows, window_s):
    from oracle import gn_oracle as O
    from tests import util as U
    lib, L = gn._lib.load(), gn._lib
    dims, out = (10, 5, 0), (3, 4, 5)
    rng = np.random.default_rng(0)
    blk = U.block_from_params(gn, O.make_block_params(rng, dims, out))
    keep = []
    p = blk._c(keep)
    ef32 = torch.from_numpy(rng.random((1, g.n_edges, 10), dtype=np.float32)).cuda()
    nf32 = torch.from_numpy(rng.random((1, g.n_nodes, 5), dtype=np.float32)).cuda()
    ef16, nf16 = ef32.to(torch.bfloat16), nf32.to(torch.bfloat16)
    s = torch.cuda.current_stream().cuda_stream
    forms = {}
    for key, dt, e, n in (("fp32", torch.float32, ef32, nf32), ("bf16", torch.bfloat16, ef16, nf16)):
        outs = [torch.empty((1, T, d), dtype=dt, device="cuda") for T, d in zip((g.n_edges, g.n_nodes, g.n_graphs), out)]
        if key == "fp32":
            ws = torch.empty(int(lib.gnx_block_workspace_bytes(g._h, C.byref(p), 1)), dtype=torch.uint8, device="cuda")
            call = (lambda e=e, n=n, outs=outs, ws=ws: lib.gnx_block_forward(g._h, C.byref(p), e.data_ptr(), n.data_ptr(), None, 1,
                                                                           *(o.data_ptr() for o in outs), ws.data_ptr(), ws.numel(), 0, s))
        else:
            ws = torch.empty(int(lib.gnx_block_typed_workspace_bytes(g._h, C.byref(p), 1, L.ELEM_BF16, 0)), dtype=torch.uint8, device="cuda")
            call = (lambda e=e, n=n, outs=outs, ws=ws: lib.gnx_block_forward_typed(g._h, C.byref(p), L.ELEM_BF16, e.data_ptr(), n.data_ptr(), None, 1,
                                                                                 *(o.data_ptr() for o in outs), ws.data_ptr(), ws.numel(), 0, s))
        forms[key] = dict(call=call, outs=outs, ws_bytes=ws.numel(), keep=(ws,), ms=[],
                          bytes=algorithmic_bytes(g.n_edges, g.n_nodes, g.n_graphs, dims, out, 4 if key == "fp32" else 2))
    # warm-up, and the per-window step count (>= window_s of device time)
    steps = {}
    for key, f in forms.items():
        for _ in range(20):
            assert f["call"]() == 0, lib.gnx_last_error()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            f["call"]()
        e1.record()
        torch.cuda.synchronize()
        steps[key] = max(50, int(window_s * 1e3 / (e0.elapsed_time(e1) / 50)) + 1)
    for _ in range(windows):
        for key, f in forms.items():  # alternate the forms window by window
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps[key]):
                f["call"]()
            e1.record()
            torch.cuda.synchronize()
            f["ms"].append(e0.elapsed_time(e1) / steps[key])
    # the bf16 outputs are the rounded fp32 outputs of the widened inputs: checked here too, on the timed buffers
    ref = [o for o in forms["fp32"]["outs"]]
    ew, nw = ef16.float(), nf16.float()  # (held until the call has run)
    assert lib.gnx_block_forward(g._h, C.byref(p), ew.data_ptr(), nw.data_ptr(), None, 1, *(o.data_ptr() for o in ref),
                                 forms["fp32"]["keep"][0].data_ptr(), forms["fp32"]["ws_bytes"], 0, s) == 0
    torch.cuda.synchronize()
    differ = {k: int((a.to(torch.bfloat16).view(torch.int16) != b.view(torch.int16)).sum()) for k, a, b in zip(("ef", "nf", "gf"), ref, forms["bf16"]["outs"])}
    res = dict(config=name, E=g.n_edges, N=g.n_nodes, G=g.n_graphs, dims="(10,5,0)=>(3,4,5)", windows=windows, steps_per_window=steps,
               bit_identical=not any(differ.values()), values_differing=differ)
    for key, f in forms.items():
        med = float(np.median(f["ms"]))
        res[key] = dict(median_ms_per_step=med, window_ms=[round(x, 5) for x in f["ms"]], algorithmic_bytes=f["bytes"],
                        algorithmic_GB_per_s=f["bytes"] / (med * 1e-3) / 1e9)
    res["time_ratio_bf16_over_fp32"] = res["bf16"]["median_ms_per_step"] / res["fp32"]["median_ms_per_step"]
    res["byte_ratio_bf16_over_fp32"] = res["bf16"]["algorithmic_bytes"] / res["fp32"]["algorithmic_bytes"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of device time per window (>= 0.2)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import graphnets_jl_amd as gn
    from tests import util as U
    torch.cuda.set_device(0)
    colptr, rowval = U.er_csc(np.random.default_rng(0), 100_000, 1_000_000)
    c2 = gn.GNGraphBatch.from_csc([colptr], [rowval], [100_000])
    # 512 graphs of 32..256 nodes with ~3 in-edges per node: every graph <= 8 wave tiles, so the batch takes the pack form
    rng = np.random.default_rng(1)
    cps, rvs, ns = [], [], []
    for n in rng.integers(32, 257, 512):
        cp, rv = U.er_csc(rng, int(n), int(3 * n))
        cps.append(cp); rvs.append(rv); ns.append(int(n))
    small = gn.GNGraphBatch.from_csc(cps, rvs, ns)
    out = dict(device=torch.cuda.get_device_name(0), results=[run_config(gn, torch, "C2 (1M edges, one graph)", c2, a.windows, a.window),
                                                             run_config(gn, torch, "512 small graphs (pack form)", small, a.windows, a.window)])
    for r in out["results"]:
        print(f"{r['config']}: fp32 {r['fp32']['median_ms_per_step'] * 1e3:.2f} us/step ({r['fp32']['algorithmic_bytes'] / 1e6:.1f} MB), "
              f"bf16 {r['bf16']['median_ms_per_step'] * 1e3:.2f} us/step ({r['bf16']['algorithmic_bytes'] / 1e6:.1f} MB), "
              f"time ratio {r['time_ratio_bf16_over_fp32']:.3f}, byte ratio {r['byte_ratio_bf16_over_fp32']:.3f}, bit-identical {r['bit_identical']}")
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
