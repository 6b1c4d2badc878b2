"""Child process of tests/test_gpu_chain_bw_stress.py: gnx_chain_block_backward takes no flags, the form of its matrix-core products (six bf16 terms,
or the fp32 instruction under GNX_FFN_FP32 / GNX_EDGE_FP32) is read from the environment once per process — so each form gets a process of its own.
`python -m tests.chain_bw_stress_child OUTDIR` builds the batch of tests/chain_bw_cases.py, asserts that the library's CSC and offsets are those the
references use, and runs every case once through the C ABI: gnx_chain_block_forward and gnx_chain_block_backward, and for the narrow family
gnx_chain_block_forward_narrow and gnx_chain_block_backward_narrow as well — every call inside a sentinel arena (tests/arena.py: outputs filled
with NaN bytes, the workspace of exactly the queried size, guards checked after the call) with the descriptors of
tests/test_gpu_memory_contract.py, which carry the sqrt-eps kind of a LayerNorm and any activation on a last layer.  It writes
OUTDIR/<case>.<fw|bw>.<entry>.npz and OUTDIR/meta.json ({"flags": gnx_default_flags, "masks": {case: [forward, backward]}, "scopes": {case: {entry:
{profiler scope: kernels}}}}).  Nothing is compared here; any failed call raises."""
import ctypes as C
import json
import os
import sys

import numpy as np


def _forward(gn, g, d, narrow, what):
    from tests import arena as AR
    from tests import test_gpu_backward_replicas as RP
    from tests import test_gpu_memory_contract as MC
    lib = gn._lib.load()
    p, R = d["p"], d["R"]
    a = AR.Arena("cuda")
    MC._decl_chains(a, p)
    ins = [MC._decl(a, n, v) for n, v in zip(("ef", "nf", "gf"), d["x"])]
    outs = MC._decl_outputs(a, "", R, MC._rows(g), MC._chain_out_widths(p))
    keep = []
    query = lib.gnx_chain_block_forward_narrow_workspace_bytes if narrow else lib.gnx_chain_block_workspace_bytes
    entry = lib.gnx_chain_block_forward_narrow if narrow else lib.gnx_chain_block_forward
    a.workspace("ws", lambda: query(g._h, C.byref(MC._chain_params(gn, a, p, keep)), R))

    def call(a):
        P = a.ptr
        return entry(g._h, C.byref(MC._chain_params(gn, a, p, keep)), *map(P, ins), R, *map(P, outs), P("ws"), a.nbytes("ws"), 0, MC._stream())

    got, _ = RP._launch(gn, a, call, what)
    return got


def _backward(gn, g, d, narrow, what):
    from tests import arena as AR
    from tests import test_gpu_backward_replicas as RP
    from tests import test_gpu_memory_contract as MC
    L, lib = gn._lib, gn._lib.load()
    p, R = d["p"], d["R"]
    a = AR.Arena("cuda")
    MC._decl_chains(a, p)
    ins = [MC._decl(a, n, v) for n, v in zip(("ef", "nf", "gf"), d["x"])]
    gs = [MC._decl(a, n, c) for n, c in zip(RP.COTS, d["cot"])]
    dx = [a.output(n, v.shape) if v is not None else None for n, v in zip(RP.DX, d["x"])]
    for name in ("edge", "node", "graph"):
        for i, (w, b, c) in enumerate(p[name]):
            if isinstance(w, str):
                a.output(f"grad.{name}{i}.dW", b.shape)
                a.output(f"grad.{name}{i}.db", c.shape)
            else:
                MC._decl_dense_grad(a, f"grad.{name}{i}", w, b)
    keep = []
    query = lib.gnx_chain_block_backward_narrow_workspace_bytes if narrow else lib.gnx_chain_block_backward_workspace_bytes
    entry = lib.gnx_chain_block_backward_narrow if narrow else lib.gnx_chain_block_backward
    a.workspace("ws", lambda: query(g._h, C.byref(MC._chain_params(gn, a, p, keep)), R))

    def call(a):
        P = a.ptr
        arrays = []
        for name in ("edge", "node", "graph"):
            arr = (L.DenseGrad * max(len(p[name]), 1))()
            for i in range(len(p[name])):
                arr[i] = MC._dense_grad(gn, a, f"grad.{name}{i}")
            arrays.append(arr)
        gr = L.ChainBlockGrads(*[C.cast(x_, C.POINTER(L.DenseGrad)) for x_ in arrays])
        return entry(g._h, C.byref(MC._chain_params(gn, a, p, keep)), *map(P, ins), *map(P, gs), R, *map(P, dx), C.byref(gr), P("ws"), a.nbytes("ws"), MC._stream())

    got, seen = RP._launch(gn, a, call, what)
    cp = MC._chain_params(gn, a, p, keep)
    masks = [int(lib.gnx_chain_block_forward_narrow_applies(g._h, C.byref(cp), R)), int(lib.gnx_chain_block_backward_narrow_applies(g._h, C.byref(cp), R))]
    return {n[5:] if n.startswith("grad.") else n: v for n, v in got.items()}, {n: int(v["kernels"]) for n, v in seen.items()}, masks


def main(outdir):
    import torch
    import graphnets_jl_amd as gn
    from tests import bw_x6_cases as BC
    from tests import chain_bw_cases as CC
    from tests import test_gpu_memory_contract as MC
    torch.cuda.set_device(0)
    handles = {}
    for key, parts, want in (("batch", list(CC.batch_parts()), CC.batch()), ("one", [BC.graph_parts()], BC.csc())):
        g, csc = MC._from_csc(gn, parts)
        for got, w in zip(csc, want):  # the graphs the references are computed on
            assert np.array_equal(np.asarray(got), w), key
        handles[key] = g
    assert MC._rows(handles["batch"]) == (CC.N_EDGES, CC.N_NODES, CC.N_GRAPHS)
    meta = dict(flags=int(gn._lib.load().gnx_default_flags()), masks={}, scopes={})
    for cid in CC.CASE_IDS:
        d = CC.data(cid)
        g = handles["one" if d["R"] > 1 else "batch"]
        assert MC._rows(g) == CC.rows(cid)
        meta["scopes"][cid] = {}
        for entry in CC.entries(cid):
            narrow = entry == "narrow"
            np.savez(os.path.join(outdir, f"{cid}.fw.{entry}.npz"), **_forward(gn, g, d, narrow, f"{cid} forward {entry}"))
            got, seen, masks = _backward(gn, g, d, narrow, f"{cid} backward {entry}")
            assert set(got) == CC.grad_names(d["p"]), (cid, sorted(set(got) ^ CC.grad_names(d["p"])))
            np.savez(os.path.join(outdir, f"{cid}.bw.{entry}.npz"), **got)
            meta["scopes"][cid][entry] = seen
            meta["masks"][cid] = masks
    with open(os.path.join(outdir, "meta.json"), "w") as f:
        json.dump(meta, f)
    print("done", len(CC.CASE_IDS))


if __name__ == "__main__":
    main(sys.argv[1])
