"""Times the loop over batches at README dims (10,5,0) => (3,4,5) in three forms, alternating window by window in one process:
fp32 gnx_block_forward_steps, bf16 gnx_block_forward_steps_typed, and K separate gnx_block_forward_typed calls (what a bf16 caller ran
before the typed loop existed).  K steps per call (--steps, >= 20) over 8 rotating buffer sets; each window is timed with device events
over >= --window seconds after warm-up (tools/timing.py: timed_windows); the median ms/step of the windows is printed.  Configs: the
1M-edge batch (BASELINE configs[1]) and a batch of 512 small graphs that takes the one-launch pack form.  The bf16 loop's outputs are
checked bit for bit against the separate calls on the timed buffers.  --graph: each form is captured once into a hipGraph and the windows
replay it (no host cost per step).

  python tools/time_bf16_steps.py [--steps 20] [--windows 7] [--window 0.2] [--graph] [--only c2|all] [--out result.json]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import calls, timing  # noqa: E402

NSETS = 8
TIMING = dict(warmup=5, probe=10, min_calls=10)
CONFIGS = (("C2 (1M edges, one graph)", timing.er_1m), ("512 small graphs (pack form)", timing.pack512))


def run_config(gn, torch, name, g, K, a):
    from oracle import gn_oracle as O
    from tests import util as U
    dims, out = (10, 5, 0), (3, 4, 5)
    rng = np.random.default_rng(0)
    blk = U.block_from_params(gn, O.make_block_params(rng, dims, out))
    plan32 = gn.BlockPlan(blk, g)
    plan16 = gn.BlockPlan(blk, g, dtype=torch.bfloat16)
    ins = [(calls.draw(rng, "unit", (1, g.n_edges, 10)), calls.draw(rng, "unit", (1, g.n_nodes, 5))) for _ in range(NSETS)]
    sets32 = [dict(ef=e, nf=n, gf=None, out=plan32.outputs(), ws=plan32.new_workspace()) for e, n in ins]
    sets16 = [dict(ef=e.to(torch.bfloat16), nf=n.to(torch.bfloat16), gf=None, out=plan16.outputs(), ws=plan16.new_workspace()) for e, n in ins]
    sep16 = [dict(b, out=plan16.outputs()) for b in sets16]  # the separate calls write buffers of their own (compared below)
    seq32 = [sets32[i % NSETS] for i in range(K)]
    seq16 = [sets16[i % NSETS] for i in range(K)]
    sepq = [sep16[i % NSETS] for i in range(K)]

    def separate():
        for b in sepq:
            plan16(b["ef"], b["nf"], b["gf"], *b["out"], ws=b["ws"])

    forms = {"fp32_steps": lambda: plan32.steps(seq32), "bf16_steps": lambda: plan16.steps(seq16), "bf16_separate_typed": separate}
    graphs = []
    if a.graph:
        for key, f in list(forms.items()):
            f()
            torch.cuda.synchronize()
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg, capture_error_mode="thread_local"):
                f()
            graphs.append(cg)
            forms[key] = cg.replay
    ms, per_window = timing.timed_windows(torch, forms, a.windows, a.window, **TIMING)
    differ = {k: sum(int((u[t].view(torch.int16) != v[t].view(torch.int16)).sum()) for u, v in zip([s["out"] for s in sets16], [s["out"] for s in sep16]))
              for t, k in enumerate(("ef", "nf", "gf"))}
    res = dict(config=name, replayed_from_captured_graph=a.graph, E=g.n_edges, N=g.n_nodes, G=g.n_graphs, dims="(10,5,0)=>(3,4,5)", steps_per_call=K,
               buffer_sets=NSETS, windows=a.windows, calls_per_window=per_window, bf16_steps_bit_identical_to_separate_calls=not any(differ.values()),
               values_differing=differ)
    for key in forms:  # (a call is K steps)
        res[key] = dict(median_ms_per_step=float(np.median(ms[key])) / K, window_ms_per_step=[round(x / K, 6) for x in ms[key]])
    res["bf16_steps_over_separate"] = res["bf16_steps"]["median_ms_per_step"] / res["bf16_separate_typed"]["median_ms_per_step"]
    res["bf16_steps_over_fp32_steps"] = res["bf16_steps"]["median_ms_per_step"] / res["fp32_steps"]["median_ms_per_step"]
    return res


def run(a, graphs=None):
    """the record; graphs: one GNGraphBatch per config in place of the full-size ones (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    out = timing.RecordWriter(a.out, device=torch.cuda.get_device_name(0), replayed_from_captured_graph=a.graph, timing=timing.windows_timing(a, **TIMING), results=[])
    for i, (name, make) in enumerate(CONFIGS[:1 if a.only == "c2" else None]):
        out.add("results", run_config(gn, torch, name, make(gn) if graphs is None else graphs[i], a.steps, a))
    return out.res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of device time per window")
    ap.add_argument("--only", choices=("c2", "all"), default="all", help="c2: the 1M-edge batch alone (a profiler run)")
    ap.add_argument("--graph", action="store_true", help="replay each form from a captured graph")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps must be >= 20")
    res = run(a)
    for r in res["results"]:
        print(f"{r['config']}: fp32 steps {r['fp32_steps']['median_ms_per_step'] * 1e3:.2f} us/step, bf16 steps "
              f"{r['bf16_steps']['median_ms_per_step'] * 1e3:.2f} us/step, {r['steps_per_call']} separate typed calls "
              f"{r['bf16_separate_typed']['median_ms_per_step'] * 1e3:.2f} us/step; bf16 loop bit-identical to the separate calls: "
              f"{r['bf16_steps_bit_identical_to_separate_calls']}")
    timing.print_record(res)


if __name__ == "__main__":
    main()
