"""Times the forward of one GNCore at README ex.3's widths (10,5,3) on the 1M-edge graph (100k nodes, one graph) in three forms:

  (i)   gnx_core_forward_typed(GNX_ELEM_BF16), native path;
  (ii)  what a bf16 caller ran before it: torch .float() of the three inputs, gnx_core_forward, torch .to(bfloat16) of the three outputs;
  (iii) gnx_core_forward on fp32 tensors.

Every form walks a ring of --sets buffer sets (inputs, outputs, workspace), so that a call finds none of its rows in the caches the previous
call filled (4 sets of fp32 tensors are ~0.7 GB against the 256 MB last-level cache).  The forms alternate window by window in one process;
a window is timed with device events over >= --window seconds of device time after warm-up (tools/timing.py: timed_windows); the medians
and every window are recorded.  (i)'s outputs are checked bit for bit against (ii)'s on the timed buffers.  A last pass, with the per-kernel
profiler on and not timed from outside, records each form's kernels (gnx_profile_*).

--resources (needs hipcc, no GPU): compiles gnx_narrow_bf16.hip, gnx_narrow.hip and gnx_core_narrow.hip as build.py does and records the
vector / scalar registers, scratch and waves per SIMD of the core's kernels at these widths, bf16 beside fp32 (kept in --out across runs).

  python tools/time_bf16_core.py [--windows 7] [--window 0.3] [--sets 4] [--resources] [--out profiles/bf16_core_c4narrow.json]
"""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import calls, timing  # noqa: E402

DIMS = (10, 5, 3)
TIMING = dict(warmup=12, probe=24, min_calls=24)
PROFILED_CALLS = 20


def kernel_resources():
    """{file: {kernel: {vgpr, sgpr, scratch, waves_per_simd, lds}}} of the core's kernels at (10,5,3), from tools/kernel_resources.py's remarks"""
    from tools.kernel_resources import demangle, remarks_many
    files = ("gnx_narrow_bf16.hip", "gnx_narrow.hip", "gnx_core_narrow.hip")
    want = re.compile(r"k_block_wave(_ffe)?ILi10ELi5ELi3ELi10ELi5ELi2ELb1|k_core_post3ILi10ELi5ELi3E|k_graph_tILi15E")  # (LN = 1: the core's block)
    out = {}
    for f, res in zip(files, remarks_many(files)):
        for name, r in res.items():
            if want.search(name):
                out.setdefault(f, {})[re.sub(r"\(.*$", "", demangle(name)).replace("void gnx::", "")] = dict(
                    vgpr=r["vgpr"], sgpr=r["sgpr"], scratch_bytes_per_lane=r["scratch"], waves_per_simd=r["waves_per_simd"], lds_bytes=r["lds"])
    return out


def run(a, g=None):
    """the record; g: a GNGraphBatch in place of the 1M-edge one (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    L = gn._lib
    torch.cuda.set_device(0)
    g = timing.er_1m(gn) if g is None else g
    BF = torch.bfloat16
    case = calls.core_case(gn, g, DIMS, dtype=BF, cot=False)
    rows = calls.rows(g)
    typed = calls.build(gn, case, "core", "forward", L.ELEM_BF16, "gnx_core_forward_typed")
    plain = calls.build(gn, case, "core", "forward", L.ELEM_F32, "gnx_core_forward", x=[t.float() for t in case.x], ws=typed.ws)
    assert typed.nbytes == plain.nbytes, "the native path needs no more than the fp32 core's workspace"
    K = a.sets
    new = lambda dt: [torch.empty((1, T, d), dtype=dt, device="cuda") for T, d in zip(rows, DIMS)]
    sets = [dict(x16=[t.clone() for t in case.x], x32=[t.float() for t in case.x], o16=new(BF), o16b=None, o32=new(torch.float32),
                 ws=torch.empty(plain.nbytes, dtype=torch.uint8, device="cuda")) for _ in range(K)]
    turn = {"i": 0, "ii": 0, "iii": 0}

    def nxt(k):
        turn[k] = (turn[k] + 1) % K
        return sets[turn[k]]

    def form_i():
        b = nxt("i")
        typed.f(x=b["x16"], outs=b["o16"], ws=b["ws"])

    def form_ii():
        b = nxt("ii")
        plain.f(x=[t.float() for t in b["x16"]], outs=b["o32"], ws=b["ws"])
        b["o16b"] = [t.to(BF) for t in b["o32"]]

    def form_iii():
        b = nxt("iii")
        plain.f(x=b["x32"], outs=b["o32"], ws=b["ws"])

    forms = {"i_typed_bf16_native": form_i, "ii_torch_casts_around_fp32": form_ii, "iii_fp32": form_iii}
    ms, steps = timing.timed_windows(torch, forms, a.windows, a.window, **TIMING)
    torch.cuda.synchronize()
    same = all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for b in sets for x, y in zip(b["o16"], b["o16b"]))
    # per-kernel times: the profiler's own pass (it synchronises around every launch; not comparable with the windows above)
    kernels = {key: {k: dict(launches_per_call=v["launches"] / PROFILED_CALLS, ms_per_call=v["total_ms"] / PROFILED_CALLS)
                     for k, v in timing.profiled(gn, torch, f, PROFILED_CALLS).items()} for key, f in forms.items()}
    f = {k: timing.summary_windows(v) for k, v in ms.items()}
    i, ii, iii = (f[k]["median_ms"] for k in forms)
    feat = lambda nbytes: 2 * sum(T * d for T, d in zip(rows, DIMS)) * nbytes
    return dict(device=torch.cuda.get_device_name(0), E=g.n_edges, N=g.n_nodes, G=g.n_graphs, dims=str(DIMS), buffer_sets=K, windows=a.windows,
                timing=timing.windows_timing(a, **TIMING), calls_per_window=steps, forms=f, i_bit_identical_to_ii=bool(same), i_over_ii=i / ii, i_over_iii=i / iii,
                i_faster_than_iii=bool(i < iii), workspace_bytes=dict(fp32=plain.nbytes, typed_bf16=typed.nbytes),
                feature_tensor_bytes_in_plus_out=dict(fp32=feat(4), bf16=feat(2)), kernels_profiled=kernels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of device time per window")
    ap.add_argument("--sets", type=int, default=4, help="buffer sets in the ring")
    ap.add_argument("--resources", action="store_true", help="only compile and record the kernels' register figures (no GPU)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    old = timing.read_record(a.out)
    if a.resources:
        res = dict(old, kernel_resources=kernel_resources())
    else:
        res = run(a)
        if "kernel_resources" in old:
            res["kernel_resources"] = old["kernel_resources"]
        f = res["forms"]
        print(f"(i) typed bf16 {f['i_typed_bf16_native']['median_ms']:.4f} ms   (ii) torch casts + fp32 {f['ii_torch_casts_around_fp32']['median_ms']:.4f} ms   "
              f"(iii) fp32 {f['iii_fp32']['median_ms']:.4f} ms   i/ii {res['i_over_ii']:.3f}   i/iii {res['i_over_iii']:.3f}   "
              f"bit-identical {res['i_bit_identical_to_ii']}")
    timing.print_record(res)
    timing.RecordWriter(a.out, **res).write()
    if not a.resources and not res["i_bit_identical_to_ii"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
