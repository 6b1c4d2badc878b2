"""Times gnx_core_backward_narrow — the pullback of each FeedForward of a narrow GNCore in one kernel (csrc/gnx_core_bw_narrow.hip) — against the
calls it stands in for: gnx_core_backward (fp32) and gnx_core_backward_typed (bf16), every gradient requested, on the 1M-edge Erdős–Rényi graph
(BASELINE configs[1], "C2").  Widths: (10,5,3) README ex.3, (16,16,16) examples/train_sort.py's default, (3,4,5) and (1,1,1).

The two forms alternate window by window in one process (tools/time_bw_fused.py: timed_windows); medians of the windows, every window, the two
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
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = ((10, 5, 3), (16, 16, 16), (3, 4, 5), (1, 1, 1))


def timed_windows(torch, forms, windows, window_s):
    """forms: {key: callable}; {key: [ms per call of each window]} and the calls per window (tools/time_bw_fused.py's, restated so that this
    file also runs inside a checkout of the parent commit)"""
    steps, ms = {}, {k: [] for k in forms}
    for key, f in forms.items():
        for _ in range(5):
            f()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            f()
        e1.record()
        torch.cuda.synchronize()
        steps[key] = max(5, int(window_s * 1e3 / (e0.elapsed_time(e1) / 10)) + 1)
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


def one_case(a, gn, g, dims, bf16, baseline_only):
    import torch
    from oracle import gn_oracle as O
    from tests import util as U
    lib, L = gn._lib.load(), gn._lib
    elem = L.ELEM_BF16 if bf16 else L.ELEM_F32
    dt = torch.bfloat16 if bf16 else torch.float32
    rng = np.random.default_rng(0)
    core = U.core_from_params(gn, O.make_core_params(rng, dims))
    keep = []
    p = core._c(keep)
    params = core.parameters()
    s = torch.cuda.current_stream().cuda_stream
    rows = (g.n_edges, g.n_nodes, g.n_graphs)
    six = [torch.from_numpy((rng.random((1, T, d), dtype=np.float32) * 4 - 2)).cuda().to(dt) for T, d in zip(rows, dims)]
    six += [torch.from_numpy(rng.standard_normal((1, T, d)).astype(np.float32)).cuda().to(dt) for T, d in zip(rows, dims)]

    def outputs():
        d = [torch.empty_like(t) for t in six[:3]]
        gs = [torch.empty((q.shape[1], q.shape[0]), dtype=torch.float32, device="cuda").t() if q.dim() == 2 else torch.empty_like(q) for q in params]
        return d, gs, gn.api._core_grads(core, gs)

    label = f"{tuple(dims)} {'bf16' if bf16 else 'fp32'}"
    ptrs = [t.data_ptr() for t in six]
    nb_g = int(lib.gnx_core_backward_typed_workspace_bytes(g._h, C.byref(p), 1, elem))
    ws_g = torch.empty(nb_g, dtype=torch.uint8, device="cuda")
    d_g, g_g, gr_g = outputs()

    def existing():
        if bf16:
            rc = lib.gnx_core_backward_typed(g._h, C.byref(p), elem, *ptrs, 1, *(t.data_ptr() for t in d_g), C.byref(gr_g), ws_g.data_ptr(), nb_g, s)
        else:
            rc = lib.gnx_core_backward(g._h, C.byref(p), *ptrs, 1, *(t.data_ptr() for t in d_g), C.byref(gr_g), ws_g.data_ptr(), nb_g, s)
        assert rc == 0, lib.gnx_last_error()

    forms = {"existing": existing}
    if not baseline_only:
        assert lib.gnx_core_backward_narrow_applies(g._h, C.byref(p), 1, elem) == 1, label
        nb_n = int(lib.gnx_core_backward_narrow_workspace_bytes(g._h, C.byref(p), 1, elem))
        ws_n = torch.empty(nb_n, dtype=torch.uint8, device="cuda")
        d_n, g_n, gr_n = outputs()

        def narrow():
            assert lib.gnx_core_backward_narrow(g._h, C.byref(p), elem, None, *ptrs, 1, *(t.data_ptr() for t in d_n), C.byref(gr_n), ws_n.data_ptr(), nb_n, s) == 0, \
                lib.gnx_last_error()

        forms["narrow"] = narrow
    ms, steps = timed_windows(torch, forms, a.windows, a.window)
    torch.cuda.synchronize()
    res = {k: summary(v) for k, v in ms.items()}
    rec = dict(label=label, E=g.n_edges, N=g.n_nodes, G=g.n_graphs, elem="bf16" if bf16 else "fp32", dims=list(dims), calls_per_window=steps, forms=res)
    if baseline_only:
        return rec
    prof = {}
    for key, f in forms.items():
        gn.profile_reset(); gn.profile_enable(True)
        try:
            f()
            torch.cuda.synchronize()
        finally:
            gn.profile_enable(False)
        prof[key] = {n: dict(kernels=v["kernels"], total_ms=round(v["total_ms"], 5)) for n, v in sorted(gn.profile_read().items())}
        gn.profile_reset()
    ff_scopes = ("bw_fw_dense_generic", "bw_ff1_recompute", "bw_dx_ff2", "bw_dx_ff1", "bw_dx_generic", "bw_delta", "bw_dw_generic", "k_dw_gemm", "bw_colsum_all")
    names = ["d_ef", "d_nf", "d_gf"] + [f"param[{i}]" for i in range(len(params))]
    err, worst = max((float((x.double() - y.double()).abs().max() / max(1.0, float(x.double().abs().max()))), n) for n, x, y in zip(names, d_g + g_g, d_n + g_n) if x.numel())
    far = (d_g[0].double() - d_n[0].double()).abs().amax(dim=-1) > 1e-4 * max(1.0, float(d_g[0].double().abs().max()))  # edge rows whose gradient differs visibly
    rec.update(narrow_over_existing=res["narrow"]["median_ms"] / res["existing"]["median_ms"], workspace_bytes=dict(existing=nb_g, narrow=nb_n),
               max_output_diff_over_scale=err, max_output_diff_at=worst, edge_rows_differing_beyond_1e4_of_scale=int(far.sum()), profiler_one_call=prof,
               feedforward_scopes_ms={k: round(sum(v["total_ms"] for n, v in prof[k].items() if n in ff_scopes), 5) for k in prof})
    return rec


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
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", os.path.abspath(a.parent_root), "--baseline-only", "--windows", str(a.windows),
                            "--window", str(a.window)], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        parent = {tuple(c["dims"]): c for c in json.loads(r.stdout.strip().splitlines()[-1])["cases"]}
    sys.path.insert(0, a.root)
    os.chdir(a.root)
    import torch
    import bench
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), windows=a.windows, window_s=a.window, cases=[])
    c2 = gn.GNGraphBatch.from_csc(*bench.make_c2())
    for dims in WIDTHS:
        for bf16 in ((False,) if a.baseline_only else (False, True)):
            c = one_case(a, gn, c2, dims, bf16, a.baseline_only)
            res["cases"].append(c)
            if a.baseline_only:
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
            if a.out:  # (after every case: a run cut short leaves what it measured)
                with open(a.out, "w") as fh:
                    json.dump(res, fh, indent=1)
                    fh.write("\n")
    if a.baseline_only:
        print(json.dumps(res))


if __name__ == "__main__":
    main()
