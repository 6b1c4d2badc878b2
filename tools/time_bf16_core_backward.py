"""Times the backward of one GNCore on the 1M-edge graph (100k nodes, one graph), all 3 input gradients and all 30 parameter gradients wanted, at
README ex.3's widths (10,5,3) and at (128,64,32), in three forms:

  (i)   gnx_core_backward_typed(GNX_ELEM_BF16) on six bf16 tensors;
  (ii)  what a bf16 caller ran before it: torch .float() of the six tensors, gnx_core_backward, torch .to(bfloat16) of the three input gradients;
  (iii) gnx_core_backward on fp32 tensors.

Every form walks a ring of --sets buffer sets (inputs, cotangents, input gradients), so that a call finds none of its rows in the caches the
previous call filled; the workspace is one per form (it is hundreds of megabytes, several times the 256 MB last-level cache).  The forms
alternate window by window in one process; a window is timed with device events over >= --window seconds of device time after warm-up (the
clocks have settled by then; tools/timing.py: timed_windows), and the whole measurement is repeated --repeats times: the spread of (ii)'s
medians over the repeats is what (i) - (ii) is judged against.  (i)'s outputs are checked bit for bit against (ii)'s on the timed buffers.
Bytes: what autograd keeps alive between forward and backward (the three saved inputs) plus the workspace, and the peak that one backward call
allocates on top of its inputs (torch.cuda.max_memory_allocated: outputs, casts, workspace).

--resources (needs hipcc, no GPU): compiles gnx_generic.hip and gnx_backward.hip as build.py does and records registers, scratch, LDS and waves
per SIMD of the four LayerNorm kernels that take the element type, fp32 beside bf16 (kept in --out across runs; `parent_fp32` entries that a
previous run stored are kept too).

  python tools/time_bf16_core_backward.py [--windows 5] [--window 0.3] [--sets 3] [--repeats 3] [--resources] [--out profiles/bf16_core_backward.json]
"""
import argparse
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import calls, timing  # noqa: E402

WIDTHS = ((10, 5, 3), (128, 64, 32))
TIMING = dict(warmup=6, probe=6, min_calls=6)


def kernel_resources():
    """{kernel<...>: {vgpr, sgpr, scratch, lds, waves_per_simd}} of k_layernorm2, k_layernorm2_v4, k_ln_backward, k_ln_backward_v4"""
    from tools.kernel_resources import demangle, remarks_many
    out = {}
    for res in remarks_many(("gnx_generic.hip", "gnx_backward.hip")):
        for name, r in res.items():
            if re.search(r"k_layernorm2|k_ln_backward", name):
                out[re.sub(r"\(.*$", "", demangle(name)).replace("void gnx::", "").replace("gnx::", "")] = dict(
                    vgpr=r["vgpr"], sgpr=r["sgpr"], scratch_bytes_per_lane=r["scratch"], lds_bytes=r["lds"], waves_per_simd=r["waves_per_simd"])
    assert out and all(v["scratch_bytes_per_lane"] == 0 for v in out.values()), "an instantiation uses scratch"
    return dict(sorted(out.items()))


def run_widths(a, torch, gn, g, dims):
    L = gn._lib
    BF = torch.bfloat16
    case = calls.core_case(gn, g, dims, dtype=BF)
    rows = calls.rows(g)
    x16, c16 = case.x, case.cot
    K = a.sets
    new = lambda dt: [torch.empty((1, T, d), dtype=dt, device="cuda") for T, d in zip(rows, dims)]
    sets = [dict(x16=[t.clone() for t in x16], c16=[t.clone() for t in c16], x32=[t.float() for t in x16], c32=[t.float() for t in c16],
                 d16=new(BF), d16b=None, d32=new(torch.float32)) for _ in range(K)]
    # one workspace per form
    typed = calls.build(gn, case, "core", "backward", L.ELEM_BF16, "gnx_core_backward_typed", outs=sets[0]["d16"])
    plain = calls.build(gn, case, "core", "backward", L.ELEM_F32, "gnx_core_backward", x=sets[0]["x32"], cot=sets[0]["c32"], outs=sets[0]["d32"])
    nb16, nb32 = typed.nbytes, plain.nbytes
    assert 0 < nb32 <= nb16
    turn = {"i": 0, "ii": 0, "iii": 0}

    def nxt(k):
        turn[k] = (turn[k] + 1) % K
        return sets[turn[k]]

    def form_i():
        b = nxt("i")
        typed.f(x=b["x16"], cot=b["c16"], outs=b["d16"])

    def form_ii():
        b = nxt("ii")
        plain.f(x=[t.float() for t in b["x16"]], cot=[t.float() for t in b["c16"]], outs=b["d32"])
        b["d16b"] = [t.to(BF) for t in b["d32"]]

    def form_iii():
        b = nxt("iii")
        plain.f(x=b["x32"], cot=b["c32"], outs=b["d32"])

    forms = {"i_typed_bf16": form_i, "ii_torch_casts_around_fp32": form_ii, "iii_fp32": form_iii}
    repeats, steps = [], None
    for _ in range(a.repeats):
        ms, steps = timing.timed_windows(torch, forms, a.windows, a.window, **TIMING)
        repeats.append({k: dict(median_ms=float(np.median(v)), window_ms=[round(x, 4) for x in v]) for k, v in ms.items()})
    torch.cuda.synchronize()
    same = all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for b in sets for x, y in zip(b["d16"], b["d16b"]))
    med = {k: [r[k]["median_ms"] for r in repeats] for k in forms}
    mid = {k: float(np.median(v)) for k, v in med.items()}
    spread_ii = max(med["ii_torch_casts_around_fp32"]) - min(med["ii_torch_casts_around_fp32"])
    # bytes: what stays alive between forward and backward, and the peak one backward call allocates on top of its inputs
    # (call_peak is a difference to what is allocated when the call starts: the timed workspaces and set 0 may stay)
    b = sets[0]
    del sets[1:]
    b["d16b"] = None
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
        typed.f(x=b["x16"], cot=b["c16"], outs=new(BF), ws=torch.empty(nb16, dtype=torch.uint8, device="cuda"))

    def once_ii():
        d = new(torch.float32)
        plain.f(x=[t.float() for t in b["x16"]], cot=[t.float() for t in b["c16"]], outs=d, ws=torch.empty(nb32, dtype=torch.uint8, device="cuda"))
        return [t.to(BF) for t in d]

    def once_iii():
        plain.f(x=b["x32"], cot=b["c32"], outs=new(torch.float32), ws=torch.empty(nb32, dtype=torch.uint8, device="cuda"))

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


def run(a, g=None, widths=WIDTHS):
    """the record; g: a GNGraphBatch in place of the 1M-edge one, widths: the first only (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    g = timing.er_1m(gn) if g is None else g
    res = dict(device=torch.cuda.get_device_name(0), E=g.n_edges, N=g.n_nodes, G=g.n_graphs, buffer_sets=a.sets, windows=a.windows, repeats=a.repeats,
               timing=timing.windows_timing(a, **TIMING), widths={})
    for dims in widths:
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
    old = timing.read_record(a.out)
    if a.resources:
        res = dict(old, kernel_resources=dict(old.get("kernel_resources", {}), this_change=kernel_resources()))
    else:
        res = dict(old, timing=run(a))
    timing.print_record(res)
    timing.RecordWriter(a.out, **res).write()
    if not a.resources and not all(r["i_bit_identical_to_ii"] for r in res["timing"]["widths"].values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
