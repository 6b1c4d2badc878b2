"""Child process of tests/test_gpu_bw_x6_stress.py: the backward's entry points take no flags, the form of their matrix-core products (six bf16 terms,
or the fp32 instruction under GNX_FFN_FP32 / GNX_EDGE_FP32) is read from the environment once per process — so each form gets a process of its own.
`python -m tests.bw_x6_stress_child OUTDIR` runs every case of tests/bw_x6_cases.py once through the C ABI (gnx_block_backward / gnx_core_backward,
inside the sentinel arena and with the descriptors of tests/test_gpu_backward_replicas.py) and writes OUTDIR/<case>.npz (every gradient) and
OUTDIR/meta.json ({"flags": gnx_default_flags, "scopes": {case: profiler scope names}}).  Nothing is compared here; any failed call raises."""
import ctypes as C
import json
import os
import sys

import numpy as np


def _call_block(gn, g, d, what):
    from tests import arena as AR
    from tests import test_gpu_backward_replicas as RP
    from tests import test_gpu_memory_contract as MC
    lib = gn._lib.load()
    p, R = d["p"], 1
    a = AR.Arena("cuda")
    MC._decl_block(a, p)
    ins = [a.input(n, v) for n, v in zip(("ef", "nf", "gf"), d["x"])]
    fws = [a.input(n, v) for n, v in zip(("ef_out", "nf_out", "gf_out"), d["y"])]
    gs = [a.input(n, c) for n, c in zip(RP.COTS, d["cot"])]
    dx = [a.output(n, v.shape) for n, v in zip(RP.DX, d["x"])]
    for fn, w, b in RP.FNS:
        MC._decl_dense_grad(a, f"grad.{fn}", p[w], p[b])
    a.workspace("ws", lambda: lib.gnx_block_backward_workspace_bytes(g._h, C.byref(MC._block_params(gn, a, p)), R))

    def call(a):
        P = a.ptr
        gr = gn._lib.BlockGrads(*[MC._dense_grad(gn, a, f"grad.{fn}") for fn, _, _ in RP.FNS])
        return lib.gnx_block_backward(g._h, C.byref(MC._block_params(gn, a, p)), *map(P, ins), *map(P, fws), *map(P, gs), R, *map(P, dx), C.byref(gr),
                                      P("ws"), a.nbytes("ws"), MC._stream())

    return RP._launch(gn, a, call, what)


def main(outdir):
    import torch
    import graphnets_jl_amd as gn
    from tests import bw_x6_cases as BC
    from tests import test_gpu_backward_replicas as RP
    from tests import test_gpu_memory_contract as MC
    torch.cuda.set_device(0)
    g, csc = MC._from_csc(gn, [BC.graph_parts()])
    assert (g.n_edges, g.n_nodes, g.n_graphs) == BC.ROWS
    for got, want in zip(csc, BC.csc()):  # the graph the references are computed on
        assert np.array_equal(np.asarray(got), want)
    meta = dict(flags=int(gn._lib.load().gnx_default_flags()), scopes={})
    for cid in BC.CASE_IDS:
        d = BC.data(cid)
        if d["kind"] == "block":
            got, seen = _call_block(gn, g, d, cid)
        else:
            got, seen = RP._call_core(gn, g, d["p"], d["act"], list(d["x"]), list(d["cot"]), cid)
        assert set(got) == BC.names(cid), (cid, sorted(set(got) ^ BC.names(cid)))
        np.savez(os.path.join(outdir, cid + ".npz"), **got)
        meta["scopes"][cid] = sorted(seen)
    with open(os.path.join(outdir, "meta.json"), "w") as f:
        json.dump(meta, f)
    print("done", len(BC.CASE_IDS))


if __name__ == "__main__":
    main(sys.argv[1])
