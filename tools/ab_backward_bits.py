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
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import calls, timing  # noqa: E402
from tools.timing import sha  # noqa: E402

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


def block_case(gn, g, in_dims, out_dims, act, R, dnf_only, bf16):
    import torch
    L = gn._lib
    elem = L.ELEM_BF16 if bf16 else L.ELEM_F32
    case = calls.block_case(gn, g, in_dims, out_dims, act=act, dtype=calls.elem_dtype(gn, elem), R=R)
    fw = calls.build(gn, case, "block", "forward", elem, "gnx_block_forward_typed", poison=True)
    fw.f()
    torch.cuda.synchronize()
    # the fp32-only entries exist for fp32 alone
    entries = ("gnx_block_backward_typed", "gnx_block_backward_fused_typed", "gnx_block_backward_narrow")
    if not bf16:
        entries = ("gnx_block_backward", "gnx_block_backward_fused") + entries
    names = ("d_ef", "d_nf", "d_gf", "dWe", "dbe", "dWn", "dbn", "dWg", "dbg")
    rec = {}
    for name in entries:
        c = calls.build(gn, case, "block", "backward", elem, name, fwd=fw.outs, poison=True, want=(not dnf_only, True, not dnf_only), grads=not dnf_only)
        c.f()
        torch.cuda.synchronize()
        has_applies = hasattr(gn._lib.load(), name + "_applies")
        rec[name] = dict(applies=calls.applies(gn, case, name + "_applies", *c.entry.query_tail) if has_applies else None, workspace_bytes=c.nbytes,
                         sha256={n: sha(t) for n, t in zip(names, c.outs + (c.grads or [None] * 6))})
    return rec


def core_case(gn, g, dims, entry, bf16, drop_p):
    import torch
    L = gn._lib
    elem = L.ELEM_BF16 if bf16 else L.ELEM_F32
    case = calls.core_case(gn, g, dims, dtype=calls.elem_dtype(gn, elem))
    c = calls.build(gn, case, "core", "backward", elem, entry, drop=None if drop_p is None else L.Dropout(drop_p, 0, 1234), poison=True)
    c.f()
    torch.cuda.synchronize()
    names = ["d_ef", "d_nf", "d_gf"] + [f"param[{i}]" for i in range(len(c.grads))]
    return {entry: dict(narrow_applies=calls.applies(gn, case, "gnx_core_backward_narrow_applies", elem), workspace_bytes=c.nbytes,
                        sha256={n: sha(t.t() if t.dim() == 2 else t) for n, t in zip(names, c.outs + c.grads)})}


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


def run(limit=None, core_limit=None):
    """the child's record; limit / core_limit: the first block and core cases only, and no chain case (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    from tests.test_gpu_bw_fused import _graph
    torch.cuda.set_device(0)
    rec = {}
    for label, graph, in_dims, out_dims, act, R, dnf_only in BLOCK_CASES[:limit]:
        for bf16 in (False, True):
            rec[f"block {label} {'bf16' if bf16 else 'fp32'} on {graph}"] = block_case(gn, _graph(gn, graph), in_dims, out_dims, act, R, dnf_only, bf16)
    for label, graph, dims, entry, bf16, drop_p in CORE_CASES[:0 if limit is not None and core_limit is None else core_limit]:
        rec[f"{label} on {graph}"] = core_case(gn, _graph(gn, graph), dims, entry, bf16, drop_p)
    if limit is None and core_limit is None:
        rec[CHAIN_CASE] = chain_case(gn)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true", help="the child: the record of the library this process loads")
    ap.add_argument("--libs", nargs=2, metavar=("PARENT", "NEW"), help="the two builds")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.run:
        return timing.print_record(run())
    recs = [rec for _, rec in timing.library_rounds(__file__, a.libs, 1, ["--run"], a.timeout, cwd=ROOT)]  # one after the other; a failure ends the run
    same = recs[0] == recs[1]
    differing = [] if same else sorted(k for k in set(recs[0]) | set(recs[1]) if recs[0].get(k) != recs[1].get(k))
    timing.RecordWriter(a.out, identical=same, differing_cases=differing, cases=recs[1], **({} if same else dict(parent_cases=recs[0]))).write()
    print(f"{len(recs[1])} cases: " + ("the two libraries agree on every applies result, workspace size and output bit" if same else f"DIFFERENT: {differing}"))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
