"""Times gnx_block_backward_narrow at width sets OUTSIDE the five ahead-of-time ones — the fused edge level in the run-time specialised
k_bw_edge_wave — against what those sets ran before the entry existed: gnx_block_backward (fp32) / gnx_block_backward_typed (bf16), the generic
edge level.  Every gradient is requested, on the 1M-edge graph (BASELINE configs[1], "C2").  Width sets (de, dn, dg) => (oe, 4, 5):

  (3,2,4)=>3     36 weight-gradient pairs, one slot per lane
  (6,6,3)=>3     66 pairs and (2,3,1)=>7: 70 pairs — two slots per lane
  (20,10,4)=>1   oe = 1 with Ke = 44: the LDS-heavy pair loop (47 KB of LDS, three waves per SIMD)
  (20,16,10)=>1  Ke = 62: the widest eligible rows (64 KB of LDS, two waves per SIMD; fp32 only — at on = 4 the bf16 call's node level is on the
                 matrix cores, the typed call stages and the narrow call does not apply)

in fp32 and bf16.  The two forms alternate window by window in one process (tools/timing.py: timed_windows); medians, every window, the
workspace sizes, the profiler's per-kernel breakdown of one call of each form, and a check that the input gradients and the node / graph
parameter gradients of the two forms are the same bits are recorded.  `not_slower_beyond_spread`: narrow median <= generic median + the
generic form's spread (max - min over its windows) — the rule a class of width sets has to meet to stay eligible.

  python tools/time_bw_narrow.py [--windows 7] [--window 0.2] [--out profiles/bw_narrow_c2.json]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import calls, timing  # noqa: E402

SETS = (((3, 2, 4), 3), ((6, 6, 3), 3), ((2, 3, 1), 7), ((20, 10, 4), 1), ((20, 16, 10), 1))
TIMING = dict(warmup=10, probe=20, min_calls=20)


def one_case(a, gn, g, dims, oe, bf16):
    import torch
    L = gn._lib
    elem = L.ELEM_BF16 if bf16 else L.ELEM_F32
    out = (oe, 4, 5)
    case = calls.block_case(gn, g, dims, out, act=(1, 2, 0), dtype=calls.elem_dtype(gn, elem))
    fw = calls.build(gn, case, "block", "forward", elem, "gnx_block_forward_typed")
    fw.f()
    torch.cuda.synchronize()
    label = f"{tuple(dims)}=>{out} {'bf16' if bf16 else 'fp32'}"
    if calls.applies(gn, case, "gnx_block_backward_narrow_applies", elem) != 1:  # (bf16 with the node level on the matrix cores: the typed call stages)
        return dict(label=label, applies=False)
    ws = [calls.workspace(gn, case, "block", "backward", elem, name) for name in ("gnx_block_backward_typed", "gnx_block_backward_narrow")]  # both first
    gen = calls.build(gn, case, "block", "backward", elem, "gnx_block_backward_typed", fwd=fw.outs, ws=ws[0])
    nar = calls.build(gn, case, "block", "backward", elem, "gnx_block_backward_narrow", fwd=fw.outs, ws=ws[1])
    forms = {"generic": gen.f, "narrow": nar.f}
    ms, steps = timing.timed_windows(torch, forms, a.windows, a.window, **TIMING)
    torch.cuda.synchronize()
    raw = lambda x: x.contiguous().view(-1).view(torch.uint8)
    same = all(torch.equal(raw(x), raw(y)) for x, y in zip(gen.outs, nar.outs) if x is not None) and \
        all(torch.equal(raw(x), raw(y)) for x, y in zip(gen.grads[2:], nar.grads[2:]))
    edge_err = [float((x.double() - y.double()).abs().max() / max(1.0, float(x.double().abs().max()))) for x, y in zip(gen.grads[:2], nar.grads[:2])]
    prof = {key: timing.profiled_once(gn, torch, f) for key, f in forms.items()}
    res = {k: timing.summary_windows(v) for k, v in ms.items()}
    g_, n_ = res["generic"], res["narrow"]
    return dict(label=label, E=g.n_edges, N=g.n_nodes, G=g.n_graphs, elem="bf16" if bf16 else "fp32", dims=f"{tuple(dims)}=>{out}", act="relu/tanh/identity",
                calls_per_window=steps, forms=res, narrow_over_generic=n_["median_ms"] / g_["median_ms"], saved_ms=g_["median_ms"] - n_["median_ms"],
                not_slower_beyond_spread=bool(n_["median_ms"] <= g_["median_ms"] + g_["spread_ms"]),
                input_and_node_graph_gradients_bit_identical=bool(same), edge_gradient_max_diff_over_scale=dict(dWe=edge_err[0], dbe=edge_err[1]),
                workspace_bytes=dict(generic=gen.nbytes, narrow=nar.nbytes), profiler_one_call=prof)


def run(a, graphs=None, limit=None):
    """the record; graphs: {key: GNGraphBatch} in place of the full-size ones, limit: the first cases only (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    out = timing.RecordWriter(a.out, device=torch.cuda.get_device_name(0), windows=a.windows, window_s=a.window, timing=timing.windows_timing(a, **TIMING), cases=[])
    c2 = timing.graph(gn, "C2", graphs)
    for dims, oe, bf16 in [(dims, oe, bf16) for dims, oe in SETS for bf16 in (False, True)][:limit]:
        c = one_case(a, gn, c2, dims, oe, bf16)
        out.add("cases", c)  # (after every case: a run cut short leaves what it measured)
        if not c.get("applies", True):
            print(f"{c['label']}: the narrow call does not apply", flush=True)
            continue
        f = c["forms"]
        print(f"{c['label']}: generic {f['generic']['median_ms']:.4f} ms (spread {f['generic']['spread_ms']:.4f})   narrow {f['narrow']['median_ms']:.4f} ms   "
              f"ratio {c['narrow_over_generic']:.3f}   ws {c['workspace_bytes']['narrow'] / 2**20:.0f} / {c['workspace_bytes']['generic'] / 2**20:.0f} MiB   "
              f"bits {c['input_and_node_graph_gradients_bit_identical']}", flush=True)
    return out.res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of device time per window")
    ap.add_argument("--out", default=None)
    res = run(ap.parse_args())
    if not all(c.get("input_and_node_graph_gradients_bit_identical", True) for c in res["cases"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
