"""Are the Chain-block entries of two builds of libgnx.so the same function?  For the cases of tests/chain_bw_cases.py (through `data(cid)`: the
smallest shapes that reach every form of the Chain plan), a batch without edges and a forward-only block without edge output, this
prints, for every forward and backward entry — the fp32 entries, their narrow forms and the typed entries in fp32 and bf16 with narrow 0 and 1 —
the _applies result, the _workspace_bytes result, the return code and a SHA-256 of every output and gradient tensor.  Tests that compare the forms
with each other cannot see a change that moves all of them together; two builds run on the same device can.

  python tools/ab_chain_bits.py --libs graphnets.jl_amd/libgnx_parent.so graphnets.jl_amd/libgnx.so [--out profiles/chain_plan_bits.json]

runs the list once per library (GNX_LIB_PATH), each in a child process of its own under a time limit, one after the other — the second is not
started when the first fails — and exits 1 unless the two records are identical.  `--run` is the child: the record of the library the process
loaded, as one JSON line.  Outputs start as NaN and the workspace as 0xA5 bytes in every call.

Forms the child asserts it reached.  Forward: mask 0, mask 7, a partial mask (X-partial-forward: 6), a LayerNorm-first edge function generic and fused
(N-ln-both-modes, N-ln-sqrt-first), R = 2, a zero-width output, bf16 native, bf16 staged by narrow = 0 and by a live function outside the rule.
Backward: the generic pullback, the all-fused one, the fused node pullback behind a generic graph function (N-mixed as listed: backward mask 2 with a
graph output), a hidden gelu, a gelu last layer, a wide case, grads = NULL, bf16 staged.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import calls, timing  # noqa: E402
from tools.calls import FN  # noqa: E402
from tools.timing import sha  # noqa: E402

# (label, graph, in_dims, edge / node / graph widths): the cases tests/chain_bw_cases.py does not have
EXTRA = (("X-edgeless", "edgeless", (10, 5, 3), [16, 3], [8, 4], [6, 5]),
         ("X-forward-only-oe0", "batch", (10, 5, 3), [], [8, 4], [6, 5]),
         ("X-partial-forward", "batch", (10, 5, 3), [33, 3], [8, 4], [6, 5]))  # the edge function outside the forward's rule, the other two inside


def out_widths(p):
    from tests import test_gpu_memory_contract as MC
    return MC._chain_out_widths(p)


def run_case(gn, g, d, grads_null=False):
    """{entry label: record} of one case on handle g; d = dict(p, x, cot, R)"""
    import torch
    L = gn._lib
    keep = []
    q = calls.chain_params(gn, d["p"], keep)
    ow = out_widths(d["p"])
    to = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(dt)
    rec = {}
    # (label, elem or None for the fp32-only entries, narrow)
    forms = [("fp32", None, 0), ("fp32 narrow", None, 1)] + [(f"typed {en} narrow={n}", e, n) for en, e in (("fp32", L.ELEM_F32), ("bf16", L.ELEM_BF16)) for n in (0, 1)]
    for label, elem, narrow in forms:
        typed = elem is not None
        elem = L.ELEM_F32 if elem is None else elem
        dt = calls.elem_dtype(gn, elem)
        case = calls.given_case(g, q, keep, [to(v, dt) for v in d["x"]], [to(v, dt) for v in d["cot"]], ow, R=d["R"], oracle=d["p"])
        for direction in ("forward", "backward"):
            if direction == "backward" and ow[0] == 0:  # no pullback without an edge output: a forward-only block
                continue
            if typed:  # (the typed entries take `narrow` as a value, the fp32-only ones are two names)
                c = calls.build(gn, case, "chain", direction, elem, f"gnx_chain_block_{direction}_typed", narrow=narrow, poison=True, grads=not grads_null)
            else:
                c = calls.build(gn, case, "chain", direction, elem, f"gnx_chain_block_{direction}" + ("_narrow" if narrow else ""), poison=True, grads=not grads_null)
            c.f()
            torch.cuda.synchronize()
            if direction == "forward":
                ap = calls.applies(gn, case, "gnx_chain_block_forward_typed_applies", elem, narrow) if typed else calls.applies(gn, case, "gnx_chain_block_forward_narrow_applies")
                hashes = {n: sha(t) for n, t in zip(("ef_out", "nf_out", "gf_out"), c.outs)}
            else:
                ap = calls.applies(gn, case, "gnx_chain_block_backward_narrow_applies")
                hashes = {n: sha(t) for n, t in zip(("d_ef", "d_nf", "d_gf"), c.outs)}
                slots = iter(c.grads if c.grads else calls.grad_slots(gn, case, "chain", poison=True)[0])  # (grads = NULL: slots nobody wrote, still NaN)
                hashes.update({f"{name}{i}.{k}": sha(next(slots)) for name, _ in FN for i in range(len(d["p"][name])) for k in ("dW", "db")})
            rec[f"{direction} {label}"] = dict(applies=ap, workspace_bytes=c.nbytes, rc=0, sha256=hashes)
    return rec


def run(limit=None):
    """the child's record; limit: the first cases of tests/chain_bw_cases.py only, without the assertion over all of them (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    from oracle import gn_oracle as O
    from tests import bw_x6_cases as BC
    from tests import chain_bw_cases as CC
    from tests import test_gpu_memory_contract as MC
    from tests import util as U
    torch.cuda.set_device(0)
    edgeless = [(np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64)) for n in (5, 3, 7)]
    handles = {k: MC._from_csc(gn, parts)[0] for k, parts in (("batch", list(CC.batch_parts())), ("one", [BC.graph_parts()]), ("edgeless", edgeless))}
    rec = {}
    for cid in CC.CASE_IDS[:limit]:
        d = CC.data(cid)
        rec[cid] = run_case(gn, handles["one" if d["R"] > 1 else "batch"], d)
    if limit is not None:
        return rec
    rec["N-w16-32 grads NULL"] = run_case(gn, handles["batch"], CC.data("N-w16-32"), grads_null=True)
    for k, (label, graph, in_dims, ew, nw, gw) in enumerate(EXTRA):
        g = handles[graph]
        rng = np.random.default_rng(16000 + k)
        p = O.make_chain_block_params(rng, in_dims, ew, nw, gw, acts=CC.SMOOTH, last_acts=None)
        x = tuple(U.packed_inputs(rng, 1, g.n_edges, g.n_nodes, g.n_graphs, in_dims))
        cot = tuple(rng.standard_normal((1, T, w)).astype(np.float32) if w else None for T, w in zip(MC._rows(g), out_widths(p)))
        rec[label] = run_case(gn, g, dict(p=p, x=x, cot=cot, R=1))
    # the forms the list exists for
    fw = lambda cid, form="fp32 narrow": rec[cid]["forward " + form]["applies"]
    bw = lambda cid: rec[cid]["backward fp32 narrow"]["applies"]
    want = {"forward mask 0": fw("W-plain") == 0, "forward mask 7": fw("N-w16-32") == 7, "forward partial mask": fw("X-partial-forward") == 6 and fw("N-mixed") != 0,
            "LayerNorm-first fused": fw("N-ln-sqrt-first") == 1 and fw("N-ln-both-modes") == 7,  # (generic: the same cases through the "fp32" entries, whose calls returned 0)
            "bf16 native": fw("N-w16-32", "typed bf16 narrow=1") == 1, "bf16 staged by narrow=0": fw("N-w16-32", "typed bf16 narrow=0") == 0,
            "bf16 staged by a function outside the rule": fw("X-partial-forward", "typed bf16 narrow=1") == 0,
            "backward generic": bw("W-plain") == 0, "backward all fused": bw("N-w16-32") == 7 and bw("N-R2") == 7, "hidden gelu fused": bw("N-gelu-hidden") == 7,
            "gelu last fused": bw("N-last-act") == 7, "fused node behind a generic graph function": bw("N-mixed") == 2 and CC.out_widths("N-mixed")[2] > 0,
            "forward only": "backward fp32" not in rec["X-forward-only-oe0"], "edgeless backward": rec["X-edgeless"]["backward fp32 narrow"]["rc"] == 0}
    assert all(want.values()), [k for k, v in want.items() if not v]
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
    recs = [rec for _, rec in timing.library_rounds(__file__, a.libs, 1, ["--run"], a.timeout, cwd=ROOT)]  # one after the other, parent first; a failure ends the run
    same = recs[0] == recs[1]
    differing = [] if same else sorted(f"{k} / {e}" for k in set(recs[0]) | set(recs[1]) for e in set(recs[0].get(k, {})) | set(recs[1].get(k, {}))
                                       if recs[0].get(k, {}).get(e) != recs[1].get(k, {}).get(e))
    if a.out:  # one line per call: the tensors' hashes (compared one by one above) folded into one SHA-256 over "name:hash" lines in name order
        fold = lambda e: dict(applies=e["applies"], workspace_bytes=e["workspace_bytes"], rc=e["rc"], tensors=sum(h is not None for h in e["sha256"].values()),
                              sha256=hashlib.sha256("\n".join(f"{n}:{h}" for n, h in sorted(e["sha256"].items())).encode()).hexdigest())
        folded = lambda rec: {f"{k} / {e}": fold(v) for k, c in rec.items() for e, v in c.items()}
        with open(a.out, "w") as fh:
            fh.write('{"identical": %s, "differing": %s' % (json.dumps(same), json.dumps(differing)))
            for key, rec in (("calls", recs[1]),) + (() if same else (("parent_calls", recs[0]),)):
                fh.write(',\n"%s": {\n' % key + ",\n".join(f"{json.dumps(call)}: {json.dumps(v)}" for call, v in folded(rec).items()) + "\n}")
            fh.write("}\n")
    n = sum(len(v) for v in recs[1].values())
    print(f"{len(recs[1])} cases, {n} calls: " + ("the two libraries agree on every applies result, workspace size, return code and output bit" if same else f"DIFFERENT: {differing}"))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
