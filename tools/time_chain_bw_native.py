"""Times gnx_chain_block_backward_narrow_typed on bfloat16 features where it is native — every update function of a Chain block pulled back in one
kernel that reads bf16 rows and upstream gradients and writes the bf16 d_ef itself (csrc/gnx_chain_bw_narrow_bf16.hip) — against what a user ran
before it existed, and against the fp32 call.  Shapes and blocks: the eight of tools/time_chain_bw_narrow.py (the one-graph batch C2 and the
512-graph 1M-edge batch of bench.py; the four CONFIGS of tools/time_chain_narrow.py).  All gradients are wanted.

Three forms alternate sample by sample in one process:
  native     (a) gnx_chain_block_backward_narrow_typed(GNX_ELEM_BF16) on bf16 tensors
  staged     (b) gnx_chain_block_backward_typed(GNX_ELEM_BF16, narrow = 1) on the same tensors: six widenings, the fp32 narrow pullback, three roundings
  narrow_f32 (c) gnx_chain_block_backward_narrow on fp32 tensors
Every sample is ONE whole call between two device events, cache-cold (512 MiB overwritten in front of it, outside the events); 30 warm-up calls
(settled clocks, loaded code objects); medians of 15 samples, min / max and the spread (max - min) of every form's samples, the workspace bytes
of each form, and whether (a)'s gradients are (b)'s bit for bit.
`not_slower_beyond_spread`: (a)'s median <= (b)'s median + the spread of (b)'s samples — what a register width or source form has to meet to
stay in the native rule (include/gnx.h).  A block outside the native rule (`native_applies` 0) runs the staged call under either name: it is
timed and recorded, and does not count.

  python tools/time_chain_bw_native.py [--samples 15] [--out profiles/chain_bw_native.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools.time_chain_narrow import CONFIGS, buckets, cold_samples, summary  # noqa: E402


def one_case(a, gn, g, cfg):
    import torch
    from oracle import gn_oracle as O
    from tests.test_gpu_chain import _block
    L, lib = gn._lib, gn._lib.load()
    BF = torch.bfloat16
    rng = np.random.default_rng(0)
    p = O.make_chain_block_params(rng, *cfg)
    blk = _block(gn, p)
    keep = []
    cp, _, outw = blk._chain_params(keep)
    s = torch.cuda.current_stream().cuda_stream
    rows = (g.n_edges, g.n_nodes, g.n_graphs)
    ptr = lambda t: None if t is None else t.data_ptr()
    xb = [torch.from_numpy(rng.random((1, T, d), dtype=np.float32)).cuda().to(BF) if d else None for T, d in zip(rows, cfg[0])]
    gb = [torch.from_numpy(rng.standard_normal((1, T, d)).astype(np.float32)).cuda().to(BF) if d else None for T, d in zip(rows, outw)]
    xw = [None if t is None else t.float() for t in xb]
    gw = [None if t is None else t.float() for t in gb]

    def form(nb, x, gout, entry):
        """entry(head..., ws, nb): one pullback with every gradient wanted"""
        nb = int(nb)
        assert nb > 0, lib.gnx_last_error()
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        dx = [None if t is None else torch.empty_like(t) for t in x]
        outs, arrays = [], []
        for name in ("edge", "node", "graph"):
            arr = (L.DenseGrad * max(len(p[name]), 1))()
            for i, (w, b, c) in enumerate(p[name]):
                gW = torch.empty(len(b) if isinstance(w, str) else w.size, dtype=torch.float32, device="cuda")
                gB = torch.empty(len(c) if isinstance(w, str) else len(b), dtype=torch.float32, device="cuda")
                outs += [gW, gB]
                arr[i] = L.DenseGrad(gW.data_ptr(), gB.data_ptr())
            arrays.append(arr)
        gr = L.ChainBlockGrads(*[C.cast(q, C.POINTER(L.DenseGrad)) for q in arrays])
        keep.extend(arrays)

        def call():
            assert entry(x, gout, dx, gr, ws, nb) == 0, lib.gnx_last_error()

        return call, nb, [t for t in dx if t is not None] + outs

    h, pp = g._h, C.byref(cp)
    forms, wsb, outs = {}, {}, {}
    forms["native"], wsb["native"], outs["native"] = form(
        lib.gnx_chain_block_backward_narrow_typed_workspace_bytes(h, pp, 1, L.ELEM_BF16), xb, gb,
        lambda x, go, dx, gr, ws, nb: lib.gnx_chain_block_backward_narrow_typed(h, pp, L.ELEM_BF16, *map(ptr, x), *map(ptr, go), 1, *map(ptr, dx), C.byref(gr), ws.data_ptr(), nb, s))
    forms["staged"], wsb["staged"], outs["staged"] = form(
        lib.gnx_chain_block_backward_typed_workspace_bytes(h, pp, 1, L.ELEM_BF16, 1), xb, gb,
        lambda x, go, dx, gr, ws, nb: lib.gnx_chain_block_backward_typed(h, pp, L.ELEM_BF16, *map(ptr, x), *map(ptr, go), 1, *map(ptr, dx), C.byref(gr), ws.data_ptr(), nb, 1, s))
    forms["narrow_f32"], wsb["narrow_f32"], outs["narrow_f32"] = form(
        lib.gnx_chain_block_backward_narrow_workspace_bytes(h, pp, 1), xw, gw,
        lambda x, go, dx, gr, ws, nb: lib.gnx_chain_block_backward_narrow(h, pp, *map(ptr, x), *map(ptr, go), 1, *map(ptr, dx), C.byref(gr), ws.data_ptr(), nb, s))

    rec = dict(in_dims=list(cfg[0]), edge=cfg[1], node=cfg[2], graph=cfg[3], E=g.n_edges, N=g.n_nodes, G=g.n_graphs,
               applies=int(lib.gnx_chain_block_backward_narrow_applies(h, pp, 1)),
               native_applies=int(lib.gnx_chain_block_backward_narrow_typed_applies(h, pp, 1, L.ELEM_BF16)), register_width=buckets(cfg))
    ms = cold_samples(torch, forms, a.samples, warmup=a.warmup)
    rec.update(forms={k: summary(v) for k, v in ms.items()}, workspace_bytes=wsb)
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int16 if t.dtype == BF else torch.int32)
    rec["native_bits_equal_staged"] = all(torch.equal(bits(u), bits(v)) for u, v in zip(outs["native"], outs["staged"]))
    f = rec["forms"]
    rec["native_over_staged"] = f["native"]["median_ms"] / f["staged"]["median_ms"]
    rec["native_over_narrow_f32"] = f["native"]["median_ms"] / f["narrow_f32"]["median_ms"]
    rec["not_slower_beyond_spread"] = bool(f["native"]["median_ms"] <= f["staged"]["median_ms"] + f["staged"]["spread_ms"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.chdir(HERE)
    import torch
    import bench
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), box="one MI355X; the three forms alternate in one process", samples=a.samples,
               method=f"one call per sample between device events, 512 MiB overwritten in front of every sample (cache-cold), forms alternating, {a.warmup} warm-up "
                      "calls each; all gradients wanted",
               forms=dict(native="gnx_chain_block_backward_narrow_typed(GNX_ELEM_BF16) on bf16 tensors",
                          staged="gnx_chain_block_backward_typed(GNX_ELEM_BF16, narrow = 1) on the same tensors",
                          narrow_f32="gnx_chain_block_backward_narrow on fp32 tensors"), cases=[])
    graphs = (("C2: one graph, 100k nodes, 1M edges", lambda: gn.GNGraphBatch.from_csc(*bench.make_c2())),
              ("512 graphs of 32..256 nodes, 1M edges", lambda: gn.GNGraphBatch.from_csc(*bench.make_hetero(3))))
    cut = []
    for gname, make in graphs:
        g = make()
        for cfg in CONFIGS:
            c = one_case(a, gn, g, cfg)
            c["graph_name"] = gname
            if c["native_applies"] and not c["not_slower_beyond_spread"]:
                cut.append(len(res["cases"]))
            res["cases"].append(c)
            f = c["forms"]
            print(f"{gname} {cfg}: native {f['native']['median_ms']:.4f}   staged {f['staged']['median_ms']:.4f} (spread {f['staged']['spread_ms']:.4f})   "
                  f"narrow fp32 {f['narrow_f32']['median_ms']:.4f} ms   native / staged {c['native_over_staged']:.3f}   ws {c['workspace_bytes']['native'] >> 20} / "
                  f"{c['workspace_bytes']['staged'] >> 20} / {c['workspace_bytes']['narrow_f32'] >> 20} MiB   native {c['native_applies']}   "
                  f"bits {c['native_bits_equal_staged']}", flush=True)
            res["native_slower_than_staged_beyond_spread"] = cut
            if a.out:  # (after every case: a run cut short leaves what it measured)
                with open(a.out, "w") as fh:
                    json.dump(res, fh, indent=1)
                    fh.write("\n")
        del g


if __name__ == "__main__":
    main()
