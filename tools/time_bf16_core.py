"""Times the forward of one GNCore at README ex.3's widths (10,5,3) on the 1M-edge graph (100k nodes, one graph) in three forms:

  (i)   gnx_core_forward_typed(GNX_ELEM_BF16), native path;
  (ii)  what a bf16 caller ran before it: torch .float() of the three inputs, gnx_core_forward, torch .to(bfloat16) of the three outputs;
  (iii) gnx_core_forward on fp32 tensors.

Every form walks a ring of --sets buffer sets (inputs, outputs, workspace), so that a call finds none of its rows in the caches the previous
call filled (4 sets of fp32 tensors are ~0.7 GB against the 256 MB last-level cache).  The forms alternate window by window in one process;
a window is timed with device events over >= --window seconds of device time after warm-up; the medians and every window are recorded.
(i)'s outputs are checked bit for bit against (ii)'s on the timed buffers.  A last pass, with the per-kernel profiler on and not timed from
outside, records each form's kernels (gnx_profile_*).

--resources (needs hipcc, no GPU): compiles gnx_narrow_bf16.hip, gnx_narrow.hip and gnx_core_narrow.hip as build.py does and records the
vector / scalar registers, scratch and waves per SIMD of the core's kernels at these widths, bf16 beside fp32 (kept in --out across runs).

  python tools/time_bf16_core.py [--windows 7] [--window 0.3] [--sets 4] [--resources] [--out profiles/bf16_core_c4narrow.json]
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
DIMS = (10, 5, 3)


def kernel_resources():
    """{file: {kernel: {vgpr, sgpr, scratch, waves_per_simd, lds}}} of the core's kernels at (10,5,3), from tools/kernel_resources.py's remarks"""
    from tools.kernel_resources import remarks_many
    files = ("gnx_narrow_bf16.hip", "gnx_narrow.hip", "gnx_core_narrow.hip")
    want = re.compile(r"k_block_wave(_ffe)?ILi10ELi5ELi3ELi10ELi5ELi2ELb1|k_core_post3ILi10ELi5ELi3E|k_graph_tILi15E")  # (LN = 1: the core's block)
    out = {}
    for f, res in zip(files, remarks_many(files)):
        for name, r in res.items():
            if not want.search(name):
                continue
            demangled = subprocess.run(["c++filt", name], stdout=subprocess.PIPE, text=True).stdout.strip() or name
            out.setdefault(f, {})[re.sub(r"\(.*$", "", demangled).replace("void gnx::", "")] = dict(
                vgpr=r["vgpr"], sgpr=r["sgpr"], scratch_bytes_per_lane=r["scratch"], waves_per_simd=r["waves_per_simd"], lds_bytes=r["lds"])
    return out


def timed_windows(torch, forms, windows, window_s):
    """forms: {key: callable}; returns {key: [ms per call of each window]} and the calls per window"""
    steps, ms = {}, {k: [] for k in forms}
    for key, f in forms.items():
        for _ in range(12):
            f()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(24):
            f()
        e1.record()
        torch.cuda.synchronize()
        steps[key] = max(24, int(window_s * 1e3 / (e0.elapsed_time(e1) / 24)) + 1)
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
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), window_ms=[round(x, 5) for x in ms])


def run(a):
    import torch
    import graphnets_jl_amd as gn
    from oracle import gn_oracle as O
    from tests import util as U
    lib, L = gn._lib.load(), gn._lib
    torch.cuda.set_device(0)
    colptr, rowval = U.er_csc(np.random.default_rng(0), 100_000, 1_000_000)
    g = gn.GNGraphBatch.from_csc([colptr], [rowval], [100_000])
    rng = np.random.default_rng(0)
    core = U.core_from_params(gn, O.make_core_params(rng, DIMS))
    keep = []
    p = core._c(keep)
    s = torch.cuda.current_stream().cuda_stream
    rows = (g.n_edges, g.n_nodes, g.n_graphs)
    ptr = lambda t: t.data_ptr()
    nb32 = int(lib.gnx_core_workspace_bytes(g._h, C.byref(p), 1))
    nb16 = int(lib.gnx_core_typed_workspace_bytes(g._h, C.byref(p), 1, L.ELEM_BF16, 0))
    assert nb16 == nb32, "the native path needs no more than the fp32 core's workspace"
    x16 = [torch.from_numpy(rng.random((1, T, d), dtype=np.float32) * 4 - 2).cuda().to(torch.bfloat16) for T, d in zip(rows, DIMS)]
    K = a.sets
    new = lambda dt: [torch.empty((1, T, d), dtype=dt, device="cuda") for T, d in zip(rows, DIMS)]
    sets = [dict(x16=[t.clone() for t in x16], x32=[t.float() for t in x16], o16=new(torch.bfloat16), o16b=None, o32=new(torch.float32),
                 ws=torch.empty(nb32, dtype=torch.uint8, device="cuda")) for _ in range(K)]
    turn = {"i": 0, "ii": 0, "iii": 0}

    def nxt(k):
        turn[k] = (turn[k] + 1) % K
        return sets[turn[k]]

    def form_i():
        b = nxt("i")
        assert lib.gnx_core_forward_typed(g._h, C.byref(p), L.ELEM_BF16, *map(ptr, b["x16"]), 1, *map(ptr, b["o16"]), b["ws"].data_ptr(), nb16, 0, s) == 0

    def form_ii():
        b = nxt("ii")
        wide = [t.float() for t in b["x16"]]
        assert lib.gnx_core_forward(g._h, C.byref(p), *map(ptr, wide), 1, *map(ptr, b["o32"]), b["ws"].data_ptr(), nb32, 0, s) == 0
        b["o16b"] = [t.to(torch.bfloat16) for t in b["o32"]]

    def form_iii():
        b = nxt("iii")
        assert lib.gnx_core_forward(g._h, C.byref(p), *map(ptr, b["x32"]), 1, *map(ptr, b["o32"]), b["ws"].data_ptr(), nb32, 0, s) == 0

    forms = {"i_typed_bf16_native": form_i, "ii_torch_casts_around_fp32": form_ii, "iii_fp32": form_iii}
    ms, steps = timed_windows(torch, forms, a.windows, a.window)
    torch.cuda.synchronize()
    same = all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for b in sets for x, y in zip(b["o16"], b["o16b"]))
    # per-kernel times: the profiler's own pass (it synchronises around every launch; not comparable with the windows above)
    kernels = {}
    for key, f in forms.items():
        L.profile_reset()
        L.profile_enable(True)
        for _ in range(20):
            f()
        torch.cuda.synchronize()
        L.profile_enable(False)
        kernels[key] = {k: dict(launches_per_call=v["launches"] / 20, ms_per_call=v["total_ms"] / 20) for k, v in sorted(L.profile_read().items())}
        L.profile_reset()
    f = {k: summary(v) for k, v in ms.items()}
    i, ii, iii = (f[k]["median_ms"] for k in forms)
    feat = lambda nbytes: 2 * sum(T * d for T, d in zip(rows, DIMS)) * nbytes
    return dict(device=torch.cuda.get_device_name(0), E=g.n_edges, N=g.n_nodes, G=g.n_graphs, dims=str(DIMS), buffer_sets=K, windows=a.windows,
                calls_per_window=steps, forms=f, i_bit_identical_to_ii=bool(same), i_over_ii=i / ii, i_over_iii=i / iii,
                i_faster_than_iii=bool(i < iii), workspace_bytes=dict(fp32=nb32, typed_bf16=nb16),
                feature_tensor_bytes_in_plus_out=dict(fp32=feat(4), bf16=feat(2)), kernels_profiled=kernels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of device time per window")
    ap.add_argument("--sets", type=int, default=4, help="buffer sets in the ring")
    ap.add_argument("--resources", action="store_true", help="only compile and record the kernels' register figures (no GPU)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    old = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as fh:
            old = json.load(fh)
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
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    if not a.resources and not res["i_bit_identical_to_ii"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
