"""Times the block forward on fp32 features (gnx_block_forward) against bfloat16 features (gnx_block_forward_typed, GNX_ELEM_BF16) at
README dims (10,5,0) => (3,4,5), on the 1M-edge batch (BASELINE configs[1]) and on a batch of small graphs that takes the one-launch
pack form.  The two forms alternate in one process; each window is timed with device events over >= --window seconds after warm-up
(tools/timing.py: timed_windows); the median ms/step of the windows is printed with the algorithmic bytes of a step (feature rows in and
out, source indices, colptr).

  python tools/time_bf16_block.py [--windows 7] [--window 0.2] [--out result.json]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import calls, timing  # noqa: E402

DIMS, OUT = (10, 5, 0), (3, 4, 5)
TIMING = dict(warmup=20, probe=50, min_calls=50)
CONFIGS = (("C2 (1M edges, one graph)", timing.er_1m), ("512 small graphs (pack form)", timing.pack512))


def algorithmic_bytes(E, N, G, dims, out, elem_bytes):
    de, dn, dg = dims
    oe, on, og = out
    return E * ((de + oe) * elem_bytes + 4) + N * ((dn + on) * elem_bytes + 4) + G * (dg + og) * elem_bytes


def run_config(gn, torch, name, g, a):
    L = gn._lib
    case = calls.block_case(gn, g, DIMS, OUT, features="unit", cot=False)
    x16 = [None if t is None else t.to(torch.bfloat16) for t in case.x]
    built = dict(fp32=calls.build(gn, case, "block", "forward", L.ELEM_F32, "gnx_block_forward"),
                 bf16=calls.build(gn, case, "block", "forward", L.ELEM_BF16, "gnx_block_forward_typed", x=x16))
    ms, steps = timing.timed_windows(torch, {k: c.f for k, c in built.items()}, a.windows, a.window, **TIMING)
    # the bf16 outputs are the rounded fp32 outputs of the widened inputs: checked here too, on the timed buffers
    built["fp32"].f(x=[None if t is None else t.float() for t in x16])
    torch.cuda.synchronize()
    differ = {k: int((u.to(torch.bfloat16).view(torch.int16) != v.view(torch.int16)).sum()) for k, u, v in zip(("ef", "nf", "gf"), built["fp32"].outs, built["bf16"].outs)}
    res = dict(config=name, E=g.n_edges, N=g.n_nodes, G=g.n_graphs, dims="(10,5,0)=>(3,4,5)", windows=a.windows, steps_per_window=steps,
               bit_identical=not any(differ.values()), values_differing=differ)
    for key, nbytes in (("fp32", 4), ("bf16", 2)):
        s, moved = timing.summary_windows(ms[key]), algorithmic_bytes(g.n_edges, g.n_nodes, g.n_graphs, DIMS, OUT, nbytes)
        res[key] = dict(median_ms_per_step=s["median_ms"], window_ms=s["window_ms"], algorithmic_bytes=moved, algorithmic_GB_per_s=moved / (s["median_ms"] * 1e-3) / 1e9)
    res["time_ratio_bf16_over_fp32"] = res["bf16"]["median_ms_per_step"] / res["fp32"]["median_ms_per_step"]
    res["byte_ratio_bf16_over_fp32"] = res["bf16"]["algorithmic_bytes"] / res["fp32"]["algorithmic_bytes"]
    return res


def run(a, graphs=None):
    """the record; graphs: one GNGraphBatch per config in place of the full-size ones (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    out = timing.RecordWriter(a.out, device=torch.cuda.get_device_name(0), timing=timing.windows_timing(a, **TIMING), results=[])
    for i, (name, make) in enumerate(CONFIGS):
        out.add("results", run_config(gn, torch, name, make(gn) if graphs is None else graphs[i], a))
    return out.res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of device time per window (>= 0.2)")
    ap.add_argument("--out", default=None)
    res = run(ap.parse_args())
    for r in res["results"]:
        print(f"{r['config']}: fp32 {r['fp32']['median_ms_per_step'] * 1e3:.2f} us/step ({r['fp32']['algorithmic_bytes'] / 1e6:.1f} MB), "
              f"bf16 {r['bf16']['median_ms_per_step'] * 1e3:.2f} us/step ({r['bf16']['algorithmic_bytes'] / 1e6:.1f} MB), "
              f"time ratio {r['time_ratio_bf16_over_fp32']:.3f}, byte ratio {r['byte_ratio_bf16_over_fp32']:.3f}, bit-identical {r['bit_identical']}")
    timing.print_record(res)


if __name__ == "__main__":
    main()
