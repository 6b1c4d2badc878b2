"""Did a change of the Chain block's HOST code move the time of a whole call?  Times three calls on tests/chain_bw_cases.py's N-w16-32 (131 graphs,
1031 nodes, 4099 edges: almost pure host and launch time) against another build of libgnx.so (the parent commit's), never against another form of
the code under test:

  a  gnx_chain_block_forward_narrow, fp32: three kernels
  b  gnx_chain_block_backward_narrow, fp32: the recompute, three pullback kernels and their finishers
  c  gnx_chain_block_forward_typed, bf16, narrow = 1: the native path

  python tools/time_chain_plan.py --libs graphnets.jl_amd/libgnx_parent.so graphnets.jl_amd/libgnx.so [--rounds 2] [--windows 4] [--out profiles/chain_plan_ab.json]

One child process per library and round (GNX_LIB_PATH), each under its own time limit, in the order parent, new, parent, new; a child that fails
ends the run.  Windows as tools/time_bw_fused.py: timed_windows; rounds x windows >= 7 per library.  `not_slower_beyond_spread` (as
tools/time_bw_plan.py): new median <= parent median + the parent's spread (max - min over its windows).  `--run` is the child.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.ab_chain_bits import chain_params, out_widths, ptr  # noqa: E402
from tools.time_bw_fused import summary, timed_windows  # noqa: E402

CASE = "N-w16-32"


def calls(gn, g, d):
    import numpy as np
    import torch
    lib, L = gn._lib.load(), gn._lib
    keep = []
    q, gshapes = chain_params(gn, d["p"], keep)
    p, R = C.byref(q), d["R"]
    s = torch.cuda.current_stream().cuda_stream
    rows, ow = (g.n_edges, g.n_nodes, g.n_graphs), out_widths(d["p"])
    to = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(dt)
    x, cot = [to(v, torch.float32) for v in d["x"]], [to(v, torch.float32) for v in d["cot"]]
    xb = [to(v, torch.bfloat16) for v in d["x"]]
    outs = [torch.empty((R, T, w), device="cuda") for T, w in zip(rows, ow)]
    outs_b = [torch.empty((R, T, w), dtype=torch.bfloat16, device="cuda") for T, w in zip(rows, ow)]
    dx = [torch.empty_like(v) for v in x]
    gts = [[(torch.empty(a, device="cuda"), torch.empty(b, device="cuda")) for a, b in fn] for fn in gshapes]
    arrays = []
    for fn in gts:
        arr = (L.DenseGrad * len(fn))(*[L.DenseGrad(ptr(a), ptr(b)) for a, b in fn])
        arrays.append(arr)
    gr = L.ChainBlockGrads(*[C.cast(a, C.POINTER(L.DenseGrad)) for a in arrays])
    assert lib.gnx_chain_block_forward_narrow_applies(g._h, p, R) == 7 and lib.gnx_chain_block_backward_narrow_applies(g._h, p, R) == 7
    assert lib.gnx_chain_block_forward_typed_applies(g._h, p, R, L.ELEM_BF16, 1) == 1
    sizes = [int(lib.gnx_chain_block_forward_narrow_workspace_bytes(g._h, p, R)), int(lib.gnx_chain_block_backward_narrow_workspace_bytes(g._h, p, R)),
             int(lib.gnx_chain_block_forward_typed_workspace_bytes(g._h, p, R, L.ELEM_BF16, 1))]
    ws = [torch.empty(n, dtype=torch.uint8, device="cuda") for n in sizes]
    X, G, O_, OB, XB, DX = ([ptr(t) for t in v] for v in (x, cot, outs, outs_b, xb, dx))
    keep += [x, cot, xb, outs, outs_b, dx, gts, arrays, gr, ws, q]

    def forward():
        assert lib.gnx_chain_block_forward_narrow(g._h, p, *X, R, *O_, ws[0].data_ptr(), sizes[0], 0, s) == 0

    def backward():
        assert lib.gnx_chain_block_backward_narrow(g._h, p, *X, *G, R, *DX, C.byref(gr), ws[1].data_ptr(), sizes[1], s) == 0

    def native():
        assert lib.gnx_chain_block_forward_typed(g._h, p, L.ELEM_BF16, *XB, R, *OB, ws[2].data_ptr(), sizes[2], 1, 0, s) == 0

    return {"a gnx_chain_block_forward_narrow fp32": forward, "b gnx_chain_block_backward_narrow fp32": backward,
            "c gnx_chain_block_forward_typed bf16 native": native}, keep


def run(a):
    import torch
    import graphnets_jl_amd as gn
    from tests import chain_bw_cases as CC
    from tests import test_gpu_memory_contract as MC
    torch.cuda.set_device(0)
    g = MC._from_csc(gn, list(CC.batch_parts()))[0]
    cs, _keep = calls(gn, g, CC.data(CASE))
    res = {}
    for name, call in cs.items():
        ms, steps = timed_windows(torch, {"call": call}, a.windows, a.window)
        res[name] = dict(window_ms=ms["call"], calls_per_window=steps["call"])
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), cases=res)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true", help="the child: the windows of the library this process loads")
    ap.add_argument("--libs", nargs=2, metavar=("PARENT", "NEW"))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--windows", type=int, default=4, help="windows per child")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of device time per window")
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.run:
        return run(a)
    assert a.rounds * a.windows >= 7
    windows, device, steps = {"parent": {}, "new": {}}, None, {}
    for _ in range(a.rounds):
        for key, lib in zip(("parent", "new"), a.libs):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--run", "--windows", str(a.windows), "--window", str(a.window)],
                                   env=dict(os.environ, GNX_LIB_PATH=os.path.abspath(lib)), capture_output=True, text=True, timeout=a.timeout, cwd=ROOT)
            except subprocess.TimeoutExpired:
                print(f"{lib}: no end within {a.timeout} s", file=sys.stderr)
                sys.exit(2)
            if r.returncode != 0:
                print(f"{lib}: exit status {r.returncode}\n{r.stderr[-4000:]}", file=sys.stderr)
                sys.exit(2)  # (a child that failed: nothing further is started)
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            device = rec["device"]
            for name, c in rec["cases"].items():
                windows[key].setdefault(name, []).extend(c["window_ms"])
                steps.setdefault(name, {})[key] = c["calls_per_window"]
    res = dict(device=device, case=CASE, order="parent, new" + ", parent, new" * (a.rounds - 1) + ": one process each", windows_per_library=a.rounds * a.windows,
               window_s=a.window, cases=[])
    for name in windows["parent"]:
        par, new = summary(windows["parent"][name]), summary(windows["new"][name])
        c = dict(case=name, calls_per_window=steps[name], parent=par, new=new, new_over_parent=new["median_ms"] / par["median_ms"],
                 not_slower_beyond_spread=bool(new["median_ms"] <= par["median_ms"] + par["spread_ms"]))
        res["cases"].append(c)
        print(f"{name}: parent {par['median_ms']:.4f} ms (spread {par['spread_ms']:.4f})   new {new['median_ms']:.4f} ms (spread {new['spread_ms']:.4f})   "
              f"ratio {c['new_over_parent']:.3f}   not_slower_beyond_spread {c['not_slower_beyond_spread']}", flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            head = {k: v for k, v in res.items() if k != "cases"}  # one line per case
            fh.write(json.dumps(head)[:-1] + ', "cases": [\n' + ",\n".join(json.dumps(c) for c in res["cases"]) + "\n]}\n")
    sys.exit(0 if all(c["not_slower_beyond_spread"] for c in res["cases"]) else 1)


if __name__ == "__main__":
    main()
