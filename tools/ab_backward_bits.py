"""Are the backward entries of two builds of libgnx.so the same function?  For a fixed, seeded list of cases — the smallest that reach every form
of the block-backward plan and of the core-backward plan, and one chain backward — this prints, for every entry that takes the case,
its _applies result, its _workspace_bytes result and a SHA-256 of every output tensor.  Tests that compare the forms with each other cannot see a
change that moves all of them together; two builds run on the same device can.

  python tools/ab_backward_bits.py --libs graphnets.jl_amd/libgnx_parent.so graphnets.jl_amd/libgnx.so [--out profiles/bw_plan_bits.json]

runs the list once per library (GNX_LIB_PATH), each in a child process of its own under a time limit, one after the other — the second is not
started when the first fails — and exits 1 unless the two records are identical.  `--run` is the child: the record of the library the process
loaded, as one JSON line.

Graphs: tests/test_gpu_bw_fused.py's small40, degrees, edgeless and e20k.  Outputs start as NaN and the workspace as 0xA5 bytes in every call.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (label, graph, in_dims, out_dims, act codes (edge, node, graph), R, only d_nf and grads NULL)
BLOCK_CASES = (
    ("aot (10,5,0)=>(3,4,5)", "small40", (10, 5, 0), (3, 4, 5), (1, 2, 0), 1, False),        # an ahead-of-time wave kernel
    ("jit (3,2,4)=>(3,4,5)", "small40", (3, 2, 4), (3, 4, 5), (1, 2, 0), 1, False),          # the run-time wave kernel
    ("refused (10,5,3)=>(3,4,5)", "degrees", (10, 5, 3), (3, 4, 5), (2, 2, 2), 1, False),    # oe Ke = 69: no wave kernel, the generic edge level
    ("mfma (8,8,8)=>(8,8,8)", "e20k", (8, 8, 8), (8, 8, 8), (1, 2, 0), 1, False),            # both levels on the matrix cores; bf16: staged
    ("gelu (3,4,5)=>(3,4,5)", "small40", (3, 4, 5), (3, 4, 5), (4, 2, 3), 1, False),         # a gelu edge function: the wave kernel is refused
    ("R2 (10,5,0)=>(3,4,5)", "degrees", (10, 5, 0), (3, 4, 5), (1, 2, 3), 2, False),
    ("edgeless (3,2,4)=>(3,4,5)", "edgeless", (3, 2, 4), (3, 4, 5), (2, 2, 2), 1, False),
    ("d_nf only, grads NULL (10,5,0)=>(3,4,5)", "degrees", (10, 5, 0), (3, 4, 5), (1, 2, 3), 1, True),
)
# (label, graph, dims, entry, bf16, Dropout p or None)
CORE_CASES = (
    ("core (10,5,3)", "small40", (10, 5, 3), "gnx_core_backward", False, None),
    ("core (10,5,3) Dropout 0.25", "small40", (10, 5, 3), "gnx_core_backward_train", False, 0.25),
    ("core (10,5,3) bf16", "small40", (10, 5, 3), "gnx_core_backward_typed", True, None),
    ("core (10,5,3) narrow", "small40", (10, 5, 3), "gnx_core_backward_narrow", False, None),
    ("core (10,5,3) narrow Dropout 0.25", "small40", (10, 5, 3), "gnx_core_backward_narrow", False, 0.25),
    ("core (10,5,3) narrow bf16", "small40", (10, 5, 3), "gnx_core_backward_narrow", True, None),
    ("core (64,32,16)", "e20k", (64, 32, 16), "gnx_core_backward", False, None),
    ("core (64,32,16) narrow: does not apply", "e20k", (64, 32, 16), "gnx_core_backward_narrow", False, None),
)
CHAIN_CASE = "chain/backward/small/layernorm"  # of tests/test_gpu_memory_contract.py


def sha(t):
    import torch
    return None if t is None else hashlib.sha256(t.detach().contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def block_case(gn, g, in_dims, out_dims, act, R, dnf_only, bf16):
    import torch
    from oracle import gn_oracle as O
    from tests import util as U
    lib, L = gn._lib.load(), gn._lib
    elem, dt = (L.ELEM_BF16, torch.bfloat16) if bf16 else (L.ELEM_F32, torch.float32)
    rng = np.random.default_rng(0)
    blk = U.block_from_params(gn, O.make_block_params(rng, in_dims, out_dims, act=act))
    keep = []
    p = C.byref(blk._c(keep))
    s = torch.cuda.current_stream().cuda_stream
    rows = (g.n_edges, g.n_nodes, g.n_graphs)
    ins = [torch.from_numpy(rng.random((R, T, d), dtype=np.float32) * 4 - 2).cuda().to(dt) if d else None for T, d in zip(rows, in_dims)]
    cot = [torch.from_numpy(rng.standard_normal((R, T, d)).astype(np.float32)).cuda().to(dt) for T, d in zip(rows, out_dims)]
    outs = [torch.empty((R, T, d), dtype=dt, device="cuda") for T, d in zip(rows, out_dims)]
    ws = torch.empty(max(int(lib.gnx_block_typed_workspace_bytes(g._h, p, R, elem, 0)), 256), dtype=torch.uint8, device="cuda")
    assert lib.gnx_block_forward_typed(g._h, p, elem, *map(ptr, ins), R, *map(ptr, outs), ws.data_ptr(), ws.numel(), 0, s) == 0, lib.gnx_last_error()
    torch.cuda.synchronize()
    nine = ins + outs + cot
    layers = (blk.edgefn, blk.nodefn, blk.graphfn)
    e = (elem,)
    # entry: (the arguments its queries take after (h, p, R), the ones its call takes after (h, p)); the fp32-only entries exist for fp32 alone
    entries = {"gnx_block_backward_typed": (e, e), "gnx_block_backward_fused_typed": (e, e), "gnx_block_backward_narrow": (e, e)}
    if not bf16:
        entries = {"gnx_block_backward": ((), ()), "gnx_block_backward_fused": ((), ()), **entries}
    rec = {}
    for name, (qa, ca) in entries.items():
        nan = lambda shape, dtype: torch.full(shape, float("nan"), dtype=dtype, device="cuda")
        d = [nan((R, T, w), dt) if w and (i == 1 or not dnf_only) else None for i, (T, w) in enumerate(zip(rows, in_dims))]
        gs = [t for l in layers for t in (nan((l.weight.shape[1], l.weight.shape[0]), torch.float32), nan(tuple(l.bias.shape), torch.float32))]
        grads = L.BlockGrads(*[L.DenseGrad(ptr(gs[2 * i]), ptr(gs[2 * i + 1])) for i in range(3)])
        applies = getattr(lib, name + "_applies", None)
        nb = int(getattr(lib, name + "_workspace_bytes")(g._h, p, R, *qa))
        w = torch.full((max(nb, 256),), 0xA5, dtype=torch.uint8, device="cuda")
        rc = getattr(lib, name)(g._h, p, *ca, *map(ptr, nine), R, *map(ptr, d), None if dnf_only else C.byref(grads), w.data_ptr(), nb, s)
        assert rc == 0, (name, lib.gnx_last_error())
        torch.cuda.synchronize()
        names = ("d_ef", "d_nf", "d_gf", "dWe", "dbe", "dWn", "dbn", "dWg", "dbg")
        rec[name] = dict(applies=None if applies is None else int(applies(g._h, p, R, *qa)), workspace_bytes=nb,
                         sha256={n: sha(t) for n, t in zip(names, d + ([None] * 6 if dnf_only else gs))})
    return rec


def core_case(gn, g, dims, entry, bf16, drop_p):
    import torch
    from oracle import gn_oracle as O
    from tests import util as U
    lib, L = gn._lib.load(), gn._lib
    elem, dt = (L.ELEM_BF16, torch.bfloat16) if bf16 else (L.ELEM_F32, torch.float32)
    rng = np.random.default_rng(0)
    core = U.core_from_params(gn, O.make_core_params(rng, dims))
    keep = []
    p = C.byref(core._c(keep))
    params = core.parameters()
    s = torch.cuda.current_stream().cuda_stream
    rows = (g.n_edges, g.n_nodes, g.n_graphs)
    six = [torch.from_numpy(rng.random((1, T, d), dtype=np.float32) * 4 - 2).cuda().to(dt) for T, d in zip(rows, dims)]
    six += [torch.from_numpy(rng.standard_normal((1, T, d)).astype(np.float32)).cuda().to(dt) for T, d in zip(rows, dims)]
    d = [torch.full_like(t, float("nan")) for t in six[:3]]
    gs = [torch.full((q.shape[1], q.shape[0]), float("nan"), dtype=torch.float32, device="cuda").t() if q.dim() == 2 else torch.full_like(q, float("nan"))
          for q in params]
    gr = gn.api._core_grads(core, gs)
    dr = None if drop_p is None else C.byref(L.Dropout(drop_p, 0, 1234))
    query, head = {"gnx_core_backward": (lambda: lib.gnx_core_backward_workspace_bytes(g._h, p, 1), ()),
                   "gnx_core_backward_train": (lambda: lib.gnx_core_backward_workspace_bytes(g._h, p, 1), (dr,)),
                   "gnx_core_backward_typed": (lambda: lib.gnx_core_backward_typed_workspace_bytes(g._h, p, 1, elem), (elem,)),
                   "gnx_core_backward_narrow": (lambda: lib.gnx_core_backward_narrow_workspace_bytes(g._h, p, 1, elem), (elem, dr))}[entry]
    nb = int(query())
    w = torch.full((max(nb, 256),), 0xA5, dtype=torch.uint8, device="cuda")
    rc = getattr(lib, entry)(g._h, p, *head, *(t.data_ptr() for t in six), 1, *(t.data_ptr() for t in d), C.byref(gr), w.data_ptr(), nb, s)
    assert rc == 0, (entry, lib.gnx_last_error())
    torch.cuda.synchronize()
    names = ["d_ef", "d_nf", "d_gf"] + [f"param[{i}]" for i in range(len(params))]
    return {entry: dict(narrow_applies=int(lib.gnx_core_backward_narrow_applies(g._h, p, 1, elem)), workspace_bytes=nb,
                        sha256={n: sha(t.t() if t.dim() == 2 else t) for n, t in zip(names, d + gs)})}


def chain_case(gn):
    import torch
    from tests import arena as AR
    from tests import test_gpu_memory_contract as M
    a = AR.Arena("cuda")
    run, _ = M.CASES[CHAIN_CASE](gn, a)
    a.build(ws_fill=0xA5)
    torch.cuda.synchronize()
    rc = run(a)
    torch.cuda.synchronize()
    assert rc == 0, gn._lib.load().gnx_last_error()
    return {"gnx_chain_block_backward": dict(workspace_bytes=int(a.nbytes("ws")), sha256={k: sha(v) for k, v in sorted(a.output_bits().items())})}


def run():
    import torch
    import graphnets_jl_amd as gn
    from tests.test_gpu_bw_fused import _graph
    torch.cuda.set_device(0)
    rec = {}
    for label, graph, in_dims, out_dims, act, R, dnf_only in BLOCK_CASES:
        for bf16 in (False, True):
            rec[f"block {label} {'bf16' if bf16 else 'fp32'} on {graph}"] = block_case(gn, _graph(gn, graph), in_dims, out_dims, act, R, dnf_only, bf16)
    for label, graph, dims, entry, bf16, drop_p in CORE_CASES:
        rec[f"{label} on {graph}"] = core_case(gn, _graph(gn, graph), dims, entry, bf16, drop_p)
    rec[CHAIN_CASE] = chain_case(gn)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true", help="the child: the record of the library this process loads")
    ap.add_argument("--libs", nargs=2, metavar=("PARENT", "NEW"), help="the two builds")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.run:
        return run()
    recs = []
    for lib in a.libs:  # one after the other; a failure ends the run
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--run"], env=dict(os.environ, GNX_LIB_PATH=os.path.abspath(lib)), capture_output=True,
                               text=True, timeout=a.timeout, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print(f"{lib}: no end within {a.timeout} s", file=sys.stderr)
            sys.exit(2)
        if r.returncode != 0:
            print(f"{lib}: exit status {r.returncode}\n{r.stderr[-4000:]}", file=sys.stderr)
            sys.exit(2)  # (a child that failed: nothing further is started)
        recs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    same = recs[0] == recs[1]
    differing = [] if same else sorted(k for k in set(recs[0]) | set(recs[1]) if recs[0].get(k) != recs[1].get(k))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(dict(identical=same, differing_cases=differing, cases=recs[1], **({} if same else dict(parent_cases=recs[0]))), fh, indent=1)
            fh.write("\n")
    print(f"{len(recs[1])} cases: " + ("the two libraries agree on every applies result, workspace size and output bit" if same else f"DIFFERENT: {differing}"))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
