"""Times the backward of one GNCore on the 1M-edge graph (100k nodes, one graph), all 3 input gradients and all 30 parameter gradients wanted, at
README ex.3's widths (10,5,3) and at (128,64,32), in three forms:

  (i)   gnx_core_backward_typed(GNX_ELEM_BF16) on six bf16 tensors;
  (ii)  what a bf16 caller ran before it: torch .float() of the six tensors, gnx_core_backward, torch .to(bfloat16) of the three input gradients;
  (iii) gnx_core_backward on fp32 tensors.

Every form walks a ring of --sets buffer sets (inputs, cotangents, input gradients), so that a call finds none of its rows in the caches the
previous call filled; the workspace is one per form (it is hundreds of megabytes, several times the 256 MB last-level cache).  The forms
alternate window by window in one process; a window is timed with device events over >= --window seconds of device time after warm-up (the
clocks have settled by then), and the whole measurement is repeated --repeats times: the spread of (ii)'s medians over the repeats is what
(i) - (ii) is judged against.  (i)'s outputs are checked bit for bit against (ii)'s on the timed buffers.
Bytes: what autograd keeps alive between forward and backward (the three saved inputs) plus the workspace, and the peak that one backward call
allocates on top of its inputs (torch.cuda.max_memory_allocated: outputs, casts, workspace).

--resources (needs hipcc, no GPU): compiles gnx_generic.hip and gnx_backward.hip as build.py does and records registers, scratch, LDS and waves
per SIMD of the four LayerNorm kernels that take the element type, fp32 beside bf16 (kept in --out across runs; `parent_fp32` entries that a
previous run stored are kept too).

  python tools/time_bf16_core_backward.py [--windows 5] [--window 0.3] [--sets 3] [--repeats 3] [--resources] [--out profiles/bf16_core_backward.json]
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WIDTHS = ((10, 5, 3), (128, 64, 32))


def kernel_resources():
    """{kernel<...>: {vgpr, sgpr, scratch, lds, waves_per_simd}} of k_layernorm2, k_layernorm2_v4, k_ln_backward, k_ln_backward_v4"""
    from tools.kernel_resources import remarks_many
    out = {}
    for res in remarks_many(("gnx_generic.hip", "gnx_backward.hip")):
        for name, r in res.items():
            if not re.search(r"k_layernorm2|k_ln_backward", name):
                continue
            demangled = subprocess.run(["c++filt", name], stdout=subprocess.PIPE, text=True).stdout.strip() or name
            out[re.sub(r"\(.*$", "", demangled).replace("void gnx::", "").replace("gnx::", "")] = dict(
                vgpr=r["vgpr"], sgpr=r["sgpr"], scratch_bytes_per_lane=r["scratch"], lds_bytes=r["lds"], waves_per_simd=r["waves_per_simd"])
    assert out and all(v["scratch_bytes_per_lane"] == 0 for v in out.values()), "an instantiation uses scratch"
    return dict(sorted(out.items()))


def timed_windows(torch, forms, windows, window_s):
    """forms: {key: callable}; returns {key: [ms per call of each window]} and the calls per window"""
    steps, ms = {}, {k: [] for k in forms}
    for key, f in forms.items():
        for _ in range(6):
            f()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(6):
            f()
        e1.record()
        torch.cuda.synchronize()
        steps[key] = max(6, int(window_s * 1e3 / (e0.elapsed_time(e1) / 6)) + 1)
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


def run_widths(a, torch, gn, g, dims):
    from oracle import gn_oracle as O
    from tests import util as U
    lib, L = gn._lib.load(), gn._lib
    rng = np.random.default_rng(0)
    core = U.core_from_params(gn, O.make_core_params(rng, dims))
    keep = []
    p = core._c(keep)
    s = torch.cuda.current_stream().cuda_stream
    rows = (g.n_edges, g.n_nodes, g.n_graphs)
    ptr = lambda t: t.data_ptr()
    nb32 = int(lib.gnx_core_backward_workspace_bytes(g._h, C.byref(p), 1))
    nb16 = int(lib.gnx_core_backward_typed_workspace_bytes(g._h, C.byref(p), 1, L.ELEM_BF16))
    assert 0 < nb32 <= nb16
    plist = core.parameters()
    gs = [torch.empty((q.shape[1], q.shape[0]), dtype=torch.float32, device="cuda").t() if q.dim() == 2 else torch.empty_like(q) for q in plist]
    gr = gn.api._core_grads(core, gs)
    mk16 = lambda f: [torch.from_numpy(f((1, T, d))).cuda().to(torch.bfloat16) for T, d in zip(rows, dims)]
    x16 = mk16(lambda sh: rng.random(sh, dtype=np.float32) * 4 - 2)
    c16 = mk16(lambda sh: rng.standard_normal(sh).astype(np.float32))
    K = a.sets
    new = lambda dt: [torch.empty((1, T, d), dtype=dt, device="cuda") for T, d in zip(rows, dims)]
    sets = [dict(x16=[t.clone() for t in x16], c16=[t.clone() for t in c16], x32=[t.float() for t in x16], c32=[t.float() for t in c16],
                 d16=new(torch.bfloat16), d16b=None, d32=new(torch.float32)) for _ in range(K)]
    ws16 = torch.empty(nb16, dtype=torch.uint8, device="cuda")
    ws32 = torch.empty(nb32, dtype=torch.uint8, device="cuda")
    turn = {"i": 0, "ii": 0, "iii": 0}

    def nxt(k):
        turn[k] = (turn[k] + 1) % K
        return sets[turn[k]]

    def typed(x, c, d, ws):
        assert lib.gnx_core_backward_typed(g._h, C.byref(p), L.ELEM_BF16, *map(ptr, x), *map(ptr, c), 1, *map(ptr, d), C.byref(gr), ws.data_ptr(), ws.numel(), s) == 0

    def plain(x, c, d, ws):
        assert lib.gnx_core_backward(g._h, C.byref(p), *map(ptr, x), *map(ptr, c), 1, *map(ptr, d), C.byref(gr), ws.data_ptr(), ws.numel(), s) == 0

    def form_i():
        b = nxt("i")
        typed(b["x16"], b["c16"], b["d16"], ws16)

    def form_ii():
        b = nxt("ii")
        plain([t.float() for t in b["x16"]], [t.float() for t in b["c16"]], b["d32"], ws32)
        b["d16b"] = [t.to(torch.bfloat16) for t in b["d32"]]

    def form_iii():
        b = nxt("iii")
        plain(b["x32"], b["c32"], b["d32"], ws32)

    forms = {"i_typed_bf16": form_i, "ii_torch_casts_around_fp32": form_ii, "iii_fp32": form_iii}
    repeats, steps = [], None
    for _ in range(a.repeats):
        ms, steps = timed_windows(torch, forms, a.windows, a.window)
        repeats.append({k: dict(median_ms=float(np.median(v)), window_ms=[round(x, 4) for x in v]) for k, v in ms.items()})
    torch.cuda.synchronize()
    same = all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for b in sets for x, y in zip(b["d16"], b["d16b"]))
    med = {k: [r[k]["median_ms"] for r in repeats] for k in forms}
    mid = {k: float(np.median(v)) for k, v in med.items()}
    spread_ii = max(med["ii_torch_casts_around_fp32"]) - min(med["ii_torch_casts_around_fp32"])
    # bytes: what stays alive between forward and backward, and the peak one backward call allocates on top of its inputs
    del sets[1:], ws16, ws32
    b = sets[0]
    b["d16"] = b["d16b"] = b["d32"] = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()

    def peak(call):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        call()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    def once_i():
        typed(b["x16"], b["c16"], new(torch.bfloat16), torch.empty(nb16, dtype=torch.uint8, device="cuda"))

    def once_ii():
        d = new(torch.float32)
        plain([t.float() for t in b["x16"]], [t.float() for t in b["c16"]], d, torch.empty(nb32, dtype=torch.uint8, device="cuda"))
        return [t.to(torch.bfloat16) for t in d]

    def once_iii():
        plain(b["x32"], b["c32"], new(torch.float32), torch.empty(nb32, dtype=torch.uint8, device="cuda"))

    feat = lambda nbytes: sum(T * d for T, d in zip(rows, dims)) * nbytes
    # (ii) as the issue describes it: the caller widened BEFORE the core, so autograd saved the fp32 copies
    nbytes = {"i_typed_bf16": dict(saved_inputs=feat(2), workspace=nb16, call_peak=peak(once_i)),
              "ii_torch_casts_around_fp32": dict(saved_inputs=feat(4), workspace=nb32, call_peak=peak(once_ii)),
              "iii_fp32": dict(saved_inputs=feat(4), workspace=nb32, call_peak=peak(once_iii))}
    for v in nbytes.values():
        v["saved_plus_workspace"] = v["saved_inputs"] + v["workspace"]
    return dict(dims=str(dims), calls_per_window=steps, repeats=repeats, median_of_medians_ms=mid, medians_ms=med,
                ii_spread_of_medians_ms=spread_ii, i_minus_ii_ms=mid["i_typed_bf16"] - mid["ii_torch_casts_around_fp32"],
                i_not_slower_than_ii=bool(mid["i_typed_bf16"] <= mid["ii_torch_casts_around_fp32"] + spread_ii),
                i_over_ii=mid["i_typed_bf16"] / mid["ii_torch_casts_around_fp32"], i_over_iii=mid["i_typed_bf16"] / mid["iii_fp32"],
                i_bit_identical_to_ii=bool(same), bytes=nbytes)


def run(a):
    import torch
    import graphnets_jl_amd as gn
    from tests import util as U
    torch.cuda.set_device(0)
    colptr, rowval = U.er_csc(np.random.default_rng(0), 100_000, 1_000_000)
    g = gn.GNGraphBatch.from_csc([colptr], [rowval], [100_000])
    res = dict(device=torch.cuda.get_device_name(0), E=g.n_edges, N=g.n_nodes, G=g.n_graphs, buffer_sets=a.sets, windows=a.windows, repeats=a.repeats,
               widths={})
    for dims in WIDTHS:
        r = run_widths(a, torch, gn, g, dims)
        res["widths"][r["dims"]] = r
        m = r["median_of_medians_ms"]
        print(f"{r['dims']}: (i) typed bf16 {m['i_typed_bf16']:.4f} ms   (ii) torch casts + fp32 {m['ii_torch_casts_around_fp32']:.4f} ms "
              f"(spread of its medians {r['ii_spread_of_medians_ms']:.4f})   (iii) fp32 {m['iii_fp32']:.4f} ms   i/ii {r['i_over_ii']:.3f}   "
              f"bit-identical {r['i_bit_identical_to_ii']}   saved + workspace bytes (i) {r['bytes']['i_typed_bf16']['saved_plus_workspace']} "
              f"(ii) {r['bytes']['ii_torch_casts_around_fp32']['saved_plus_workspace']}", flush=True)
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of device time per window")
    ap.add_argument("--sets", type=int, default=3, help="buffer sets in the ring")
    ap.add_argument("--repeats", type=int, default=3, help="repetitions of the whole measurement (medians of medians)")
    ap.add_argument("--resources", action="store_true", help="only compile and record the kernels' register figures (no GPU)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    old = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as fh:
            old = json.load(fh)
    if a.resources:
        res = dict(old, kernel_resources=dict(old.get("kernel_resources", {}), this_change=kernel_resources()))
    else:
        res = dict(old, timing=run(a))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    if not a.resources and not all(r["i_bit_identical_to_ii"] for r in res["timing"]["widths"].values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
