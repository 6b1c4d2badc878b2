"""Times gnx_core_backward_narrow — the pullback of each FeedForward of a narrow GNCore in one kernel (csrc/gnx_core_bw_narrow.hip) — against the
calls it stands in for: gnx_core_backward (fp32) and gnx_core_backward_typed (bf16), every gradient requested, on the 1M-edge Erdős–Rényi graph
(BASELINE configs[1], "C2").  Widths: (10,5,3) README ex.3, (16,16,16) examples/train_sort.py's default, (3,4,5) and (1,1,1).

The two forms alternate window by window in one process (tools/timing.py: timed_windows); medians of the windows, every window, the two
workspace sizes and the profiler's per-scope times of one call of each form (gnx_profile_*) are recorded, and the largest difference of any output
of the two forms over max(1, max|reference|), with the tensor it is in and the number of edge rows whose input gradient differs by more than 1e-4
of the scale.  (The inputs here are not kink-free: where the existing call recomputes the hidden layer on the matrix cores, a pre-activation
within rounding of zero falls on the other side of the relu kink in a few of the 1M rows, and those rows' gradients differ by whole terms — the
tests compare bits under GNX_BW_GENERIC and against float64 on kink-free draws.)
`--parent-root DIR`: a checkout of the PARENT commit with its library built; gnx_core_backward is timed there first, in a process of its own
(this script with --root DIR --baseline-only), once per width — `narrow_over_parent` is taken against that figure, and this build's own time
for the untouched call stands next to it to show the two overlap.  `not_slower_beyond_spread`: narrow median <= parent median + the parent's
spread (max - min over its windows) — what a width has to meet to stay in the eligibility rule.

  python tools/time_core_bw_narrow.py [--windows 7] [--window 0.2] [--parent-root DIR] [--out profiles/core_bw_narrow.json]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools import calls, timing  # noqa: E402

WIDTHS = ((10, 5, 3), (16, 16, 16), (3, 4, 5), (1, 1, 1))
TIMING = dict(warmup=5, probe=10, min_calls=5)
FF_SCOPES = ("bw_fw_dense_generic", "bw_ff1_recompute", "bw_dx_ff2", "bw_dx_ff1", "bw_dx_generic", "bw_delta", "bw_dw_generic", "k_dw_gemm", "bw_colsum_all")


def one_case(a, gn, g, dims, bf16, baseline_only):
    import torch
    L = gn._lib
    elem = L.ELEM_BF16 if bf16 else L.ELEM_F32
    case = calls.core_case(gn, g, dims, dtype=calls.elem_dtype(gn, elem))
    label = f"{tuple(dims)} {'bf16' if bf16 else 'fp32'}"
    old = calls.build(gn, case, "core", "backward", elem, "gnx_core_backward_typed" if bf16 else "gnx_core_backward",
                      query=("gnx_core_backward_typed_workspace_bytes", (elem,)))  # (the typed query sizes both, as in every record of this tool)
    built = {"existing": old}
    if not baseline_only:
        assert calls.applies(gn, case, "gnx_core_backward_narrow_applies", elem) == 1, label
        built["narrow"] = new = calls.build(gn, case, "core", "backward", elem, "gnx_core_backward_narrow")
    forms = {k: c.f for k, c in built.items()}
    ms, steps = timing.timed_windows(torch, forms, a.windows, a.window, **TIMING)
    torch.cuda.synchronize()
    res = {k: timing.summary_windows(v) for k, v in ms.items()}
    rec = dict(label=label, E=g.n_edges, N=g.n_nodes, G=g.n_graphs, elem="bf16" if bf16 else "fp32", dims=list(dims), calls_per_window=steps, forms=res)
    if baseline_only:
        return rec
    prof = {key: timing.profiled_once(gn, torch, f) for key, f in forms.items()}
    names = ["d_ef", "d_nf", "d_gf"] + [f"param[{i}]" for i in range(len(old.grads))]
    err, worst = max((float((x.double() - y.double()).abs().max() / max(1.0, float(x.double().abs().max()))), n)
                     for n, x, y in zip(names, old.outs + old.grads, new.outs + new.grads) if x.numel())
    d_g, d_n = old.outs[0], new.outs[0]
    far = (d_g.double() - d_n.double()).abs().amax(dim=-1) > 1e-4 * max(1.0, float(d_g.double().abs().max()))  # edge rows whose gradient differs visibly
    rec.update(narrow_over_existing=res["narrow"]["median_ms"] / res["existing"]["median_ms"], workspace_bytes=dict(existing=old.nbytes, narrow=new.nbytes),
               max_output_diff_over_scale=err, max_output_diff_at=worst, edge_rows_differing_beyond_1e4_of_scale=int(far.sum()), profiler_one_call=prof,
               feedforward_scopes_ms={k: round(sum(v["total_ms"] for n, v in prof[k].items() if n in FF_SCOPES), 5) for k in prof})
    return rec


def run(a, parent=None, graphs=None, limit=None):
    """the record; parent: {dims: the parent's case}; graphs: {key: GNGraphBatch} in place of C2, limit: the first cases only
    (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    out = timing.RecordWriter(None if a.baseline_only else a.out, device=torch.cuda.get_device_name(0), windows=a.windows, window_s=a.window,
                              timing=timing.windows_timing(a, **TIMING), cases=[])
    c2 = timing.graph(gn, "C2", graphs)
    for dims, bf16 in [(dims, bf16) for dims in WIDTHS for bf16 in ((False,) if a.baseline_only else (False, True))][:limit]:
        c = one_case(a, gn, c2, dims, bf16, a.baseline_only)
        if a.baseline_only:
            out.add("cases", c)
            continue
        f = c["forms"]
        line = f"{c['label']}: existing {f['existing']['median_ms']:.4f} ms (spread {f['existing']['spread_ms']:.4f})   narrow {f['narrow']['median_ms']:.4f} ms   " \
               f"ratio {c['narrow_over_existing']:.3f}   ws {c['workspace_bytes']['narrow'] / 2**20:.0f} / {c['workspace_bytes']['existing'] / 2**20:.0f} MiB   " \
               f"FeedForward scopes {c['feedforward_scopes_ms']['narrow']:.3f} / {c['feedforward_scopes_ms']['existing']:.3f} ms"
        if parent and not bf16:
            pf = parent[tuple(dims)]["forms"]["existing"]
            c["parent_gnx_core_backward"] = pf
            c["narrow_over_parent"] = f["narrow"]["median_ms"] / pf["median_ms"]
            c["not_slower_beyond_spread"] = bool(f["narrow"]["median_ms"] <= pf["median_ms"] + pf["spread_ms"])
            line += f"   parent {pf['median_ms']:.4f} ms (spread {pf['spread_ms']:.4f})   narrow / parent {c['narrow_over_parent']:.3f}"
        print(line, flush=True)
        out.add("cases", c)  # (after every case: a run cut short leaves what it measured)
    return out.res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of device time per window")
    ap.add_argument("--root", default=HERE, help="the checkout whose package and library are timed")
    ap.add_argument("--baseline-only", action="store_true", help="time gnx_core_backward (fp32) only and print one JSON line")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit, its library built")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parent = None
    if a.parent_root:  # first, and in a process of its own: one library per process
        parent = {tuple(c["dims"]): c for c in timing.parent_baseline(__file__, a.parent_root, ["--windows", a.windows, "--window", a.window], 900)["cases"]}
    timing.child_root(a.root)
    res = run(a, parent)
    if a.baseline_only:
        timing.print_record(res)


if __name__ == "__main__":
    main()
