"""Did a change of the backward's HOST code move the time of a whole call?  Times three calls against another build of libgnx.so (the parent
commit's), never against another form of the code under test:

  a  gnx_block_backward_narrow, bf16, (3,2,4)=>(3,4,5) on the 1M-edge graph (BASELINE configs[1], "C2"): the run-time wave kernel
  b  gnx_core_backward_narrow, fp32, (10,5,3) on C2
  c  gnx_block_backward_narrow, fp32, (10,5,0)=>(3,4,5) on tests/test_gpu_bw_fused.py's small40: 40 graphs of at most 40 nodes — the call is
     a dozen launches of almost no work each, so its time is the host's

  python tools/time_bw_plan.py --libs graphnets.jl_amd/libgnx_parent.so graphnets.jl_amd/libgnx.so [--rounds 2] [--windows 4] [--out profiles/bw_plan_ab.json]

One child process per library and round (GNX_LIB_PATH), each under its own time limit, in the order parent, new, parent, new; a child that fails
ends the run.  Windows as tools/time_bw_fused.py: timed_windows; rounds x windows >= 7 per library.  `not_slower_beyond_spread` (as
tools/time_bw_narrow.py): new median <= parent median + the parent's spread (max - min over its windows).  `--run` is the child.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.time_bw_fused import summary, timed_windows  # noqa: E402


def block_narrow(gn, g, in_dims, out_dims, bf16):
    import torch
    from oracle import gn_oracle as O
    from tests import util as U
    lib, L = gn._lib.load(), gn._lib
    elem, dt = (L.ELEM_BF16, torch.bfloat16) if bf16 else (L.ELEM_F32, torch.float32)
    rng = np.random.default_rng(0)
    blk = U.block_from_params(gn, O.make_block_params(rng, in_dims, out_dims, act=(1, 2, 0)))
    keep = []
    p = blk._c(keep)
    s = torch.cuda.current_stream().cuda_stream
    rows = (g.n_edges, g.n_nodes, g.n_graphs)
    ptr = lambda t: None if t is None else t.data_ptr()
    ins = [torch.from_numpy(rng.random((1, T, d), dtype=np.float32) * 4 - 2).cuda().to(dt) if d else None for T, d in zip(rows, in_dims)]
    cot = [torch.from_numpy(rng.standard_normal((1, T, d)).astype(np.float32)).cuda().to(dt) for T, d in zip(rows, out_dims)]
    outs = [torch.empty((1, T, d), dtype=dt, device="cuda") for T, d in zip(rows, out_dims)]
    ws = torch.empty(int(lib.gnx_block_typed_workspace_bytes(g._h, C.byref(p), 1, elem, 0)), dtype=torch.uint8, device="cuda")
    assert lib.gnx_block_forward_typed(g._h, C.byref(p), elem, *map(ptr, ins), 1, *map(ptr, outs), ws.data_ptr(), ws.numel(), 0, s) == 0, lib.gnx_last_error()
    nine = [ptr(t) for t in ins + outs + cot]
    d = [torch.empty((1, T, w), dtype=dt, device="cuda") if w else None for T, w in zip(rows, in_dims)]
    gs = [t for l in (blk.edgefn, blk.nodefn, blk.graphfn) for t in (torch.empty((l.weight.shape[1], l.weight.shape[0]), device="cuda"), torch.empty_like(l.bias))]
    gr = L.BlockGrads(*[L.DenseGrad(gs[2 * i].data_ptr(), gs[2 * i + 1].data_ptr()) for i in range(3)])
    assert lib.gnx_block_backward_narrow_applies(g._h, C.byref(p), 1, elem) == 1
    nb = int(lib.gnx_block_backward_narrow_workspace_bytes(g._h, C.byref(p), 1, elem))
    w = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dp = [ptr(t) for t in d]
    keep += [ins, cot, outs, d, gs, gr, w, p]

    def call():
        assert lib.gnx_block_backward_narrow(g._h, C.byref(p), elem, *nine, 1, *dp, C.byref(gr), w.data_ptr(), nb, s) == 0

    return call, keep


def core_narrow(gn, g, dims):
    import torch
    from oracle import gn_oracle as O
    from tests import util as U
    lib, L = gn._lib.load(), gn._lib
    rng = np.random.default_rng(0)
    core = U.core_from_params(gn, O.make_core_params(rng, dims))
    keep = []
    p = core._c(keep)
    s = torch.cuda.current_stream().cuda_stream
    rows = (g.n_edges, g.n_nodes, g.n_graphs)
    six = [torch.from_numpy(rng.random((1, T, d), dtype=np.float32) * 4 - 2).cuda() for T, d in zip(rows, dims)]
    six += [torch.from_numpy(rng.standard_normal((1, T, d)).astype(np.float32)).cuda() for T, d in zip(rows, dims)]
    d = [torch.empty_like(t) for t in six[:3]]
    gs = [torch.empty((q.shape[1], q.shape[0]), dtype=torch.float32, device="cuda").t() if q.dim() == 2 else torch.empty_like(q) for q in core.parameters()]
    gr = gn.api._core_grads(core, gs)
    assert lib.gnx_core_backward_narrow_applies(g._h, C.byref(p), 1, L.ELEM_F32) == 1
    nb = int(lib.gnx_core_backward_narrow_workspace_bytes(g._h, C.byref(p), 1, L.ELEM_F32))
    w = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ptrs, dp = [t.data_ptr() for t in six], [t.data_ptr() for t in d]
    keep += [six, d, gs, gr, w, p, core]

    def call():
        assert lib.gnx_core_backward_narrow(g._h, C.byref(p), L.ELEM_F32, None, *ptrs, 1, *dp, C.byref(gr), w.data_ptr(), nb, s) == 0

    return call, keep


def run(a):
    import torch
    import bench
    import graphnets_jl_amd as gn
    from tests.test_gpu_bw_fused import _graph
    torch.cuda.set_device(0)
    c2 = gn.GNGraphBatch.from_csc(*bench.make_c2())
    cases = {"a block narrow bf16 (3,2,4)=>(3,4,5) C2": block_narrow(gn, c2, (3, 2, 4), (3, 4, 5), True),
             "b core narrow fp32 (10,5,3) C2": core_narrow(gn, c2, (10, 5, 3)),
             "c block narrow fp32 (10,5,0)=>(3,4,5) small40": block_narrow(gn, _graph(gn, "small40"), (10, 5, 0), (3, 4, 5), False)}
    res = {}
    for name, (call, _keep) in cases.items():
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
    ap.add_argument("--timeout", type=int, default=200, help="seconds per child")
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
    res = dict(device=device, order="parent, new" + ", parent, new" * (a.rounds - 1) + ": one process each", windows_per_library=a.rounds * a.windows,
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
            json.dump(res, fh, indent=1)
            fh.write("\n")
    sys.exit(0 if all(c["not_slower_beyond_spread"] for c in res["cases"]) else 1)


if __name__ == "__main__":
    main()
