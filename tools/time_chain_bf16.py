"""Times gnx_chain_block_forward_typed on bfloat16 features where it is native — every narrow update function of a Chain block in one kernel that
reads and writes bf16 rows (csrc/gnx_chain_narrow_bf16.hip) — against what a user did before it existed, and against the fp32 call.  Shapes and
blocks: those of tools/time_chain_narrow.py (the 512-graph 1M-edge batch of bench.py and the one-graph batch C2; its four CONFIGS).

Three forms alternate sample by sample in one process:
  typed      (a) gnx_chain_block_forward_typed(GNX_ELEM_BF16, narrow = 1) on bf16 tensors
  torch_cast (b) torch casts around gnx_chain_block_forward_narrow: .float() of every bf16 input, the fp32 call, .to(bfloat16) of every output
  narrow_f32 (c) gnx_chain_block_forward_narrow on fp32 tensors
Every sample is ONE whole call between two device events, cache-cold (512 MiB overwritten in front of it, outside the events); 30 warm-up calls;
medians of 15 samples, min / max and the spread of every form's samples, the workspace bytes of (a) and (c).
`not_slower_beyond_spread`: (a)'s median <= (b)'s median + the spread of (b)'s samples — what a register width or source form has to meet to
stay in the native rule (include/gnx.h).

  python tools/time_chain_bf16.py [--samples 15] [--out profiles/chain_bf16.json]
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
    xw = [None if t is None else t.float() for t in xb]
    mk = lambda dtype: [torch.empty((1, T, d), dtype=dtype, device="cuda") if d else None for T, d in zip(rows, outw)]

    nb_t = int(lib.gnx_chain_block_forward_typed_workspace_bytes(g._h, C.byref(cp), 1, L.ELEM_BF16, 1))
    nb_n = int(lib.gnx_chain_block_forward_narrow_workspace_bytes(g._h, C.byref(cp), 1))
    assert nb_t > 0 and nb_n > 0, lib.gnx_last_error()
    ws_t, ws_n = (torch.empty(n, dtype=torch.uint8, device="cuda") for n in (nb_t, nb_n))
    y_t, y_n = mk(BF), mk(torch.float32)
    cast_out = []

    def typed():
        assert lib.gnx_chain_block_forward_typed(g._h, C.byref(cp), L.ELEM_BF16, *map(ptr, xb), 1, *map(ptr, y_t), ws_t.data_ptr(), nb_t, 1, 0, s) == 0, lib.gnx_last_error()

    def narrow_f32(x=xw):
        assert lib.gnx_chain_block_forward_narrow(g._h, C.byref(cp), *map(ptr, x), 1, *map(ptr, y_n), ws_n.data_ptr(), nb_n, 0, s) == 0, lib.gnx_last_error()

    def torch_cast():
        narrow_f32([None if t is None else t.float() for t in xb])
        cast_out[:] = [None if t is None else t.to(BF) for t in y_n]

    rec = dict(in_dims=list(cfg[0]), edge=cfg[1], node=cfg[2], graph=cfg[3], E=g.n_edges, N=g.n_nodes, G=g.n_graphs,
               applies=int(lib.gnx_chain_block_forward_narrow_applies(g._h, C.byref(cp), 1)),
               typed_applies=int(lib.gnx_chain_block_forward_typed_applies(g._h, C.byref(cp), 1, L.ELEM_BF16, 1)), register_width=buckets(cfg))
    ms = cold_samples(torch, dict(typed=typed, torch_cast=torch_cast, narrow_f32=narrow_f32), a.samples)
    rec.update(forms={k: summary(v) for k, v in ms.items()}, workspace_bytes=dict(typed=nb_t, narrow_f32=nb_n))
    torch.cuda.synchronize()
    same = lambda u, v: torch.equal(u.view(torch.int16), v.view(torch.int16))
    rec["typed_bits_equal_torch_cast"] = all(same(u, v) for u, v in zip(y_t, cast_out) if u is not None)
    f = rec["forms"]
    rec["typed_over_torch_cast"] = f["typed"]["median_ms"] / f["torch_cast"]["median_ms"]
    rec["typed_over_narrow_f32"] = f["typed"]["median_ms"] / f["narrow_f32"]["median_ms"]
    rec["not_slower_beyond_spread"] = bool(f["typed"]["median_ms"] <= f["torch_cast"]["median_ms"] + f["torch_cast"]["spread_ms"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.chdir(HERE)
    import torch
    import bench
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), box="one MI355X; the three forms alternate in one process", samples=a.samples,
               method="one call per sample between device events, 512 MiB overwritten in front of every sample (cache-cold), forms alternating, 30 warm-up calls each",
               forms=dict(typed="gnx_chain_block_forward_typed(GNX_ELEM_BF16, narrow = 1) on bf16 tensors",
                          torch_cast=".float() of every bf16 input, gnx_chain_block_forward_narrow, .to(bfloat16) of every output",
                          narrow_f32="gnx_chain_block_forward_narrow on fp32 tensors"), cases=[])
    graphs = (("512 graphs of 32..256 nodes, 1M edges", lambda: gn.GNGraphBatch.from_csc(*bench.make_hetero(3))),
              ("C2: one graph, 100k nodes, 1M edges", lambda: gn.GNGraphBatch.from_csc(*bench.make_c2())))
    cut = []
    for gname, make in graphs:
        g = make()
        for cfg in CONFIGS:
            c = one_case(a, gn, g, cfg)
            c["graph_name"] = gname
            if not c["not_slower_beyond_spread"]:
                cut.append(len(res["cases"]))
            res["cases"].append(c)
            f = c["forms"]
            print(f"{gname} {cfg}: typed {f['typed']['median_ms']:.4f}   torch casts {f['torch_cast']['median_ms']:.4f} (spread {f['torch_cast']['spread_ms']:.4f})   "
                  f"narrow fp32 {f['narrow_f32']['median_ms']:.4f} ms   typed / casts {c['typed_over_torch_cast']:.3f}   ws {c['workspace_bytes']['typed'] >> 20} / "
                  f"{c['workspace_bytes']['narrow_f32'] >> 20} MiB   native {c['typed_applies']}   bits {c['typed_bits_equal_torch_cast']}", flush=True)
            res["slower_than_torch_cast_beyond_spread"] = cut
            if a.out:  # (after every case: a run cut short leaves what it measured)
                with open(a.out, "w") as fh:
                    json.dump(res, fh, indent=1)
                    fh.write("\n")
        del g


if __name__ == "__main__":
    main()
