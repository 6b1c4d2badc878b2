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
of each form, and whether (a)'s gradients are (b)'s bit for bit (tools/timing.py: cold_samples).
`not_slower_beyond_spread`: (a)'s median <= (b)'s median + the spread of (b)'s samples — what a register width or source form has to meet to
stay in the native rule (include/gnx.h).  A block outside the native rule (`native_applies` 0) runs the staged call under either name: it is
timed and recorded, and does not count.

  python tools/time_chain_bw_native.py [--samples 15] [--out profiles/chain_bw_native.json]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools import calls, timing  # noqa: E402
from tools.time_chain_narrow import CONFIGS, buckets  # noqa: E402

BF16_CHAIN = {"bf16_chain", "bf16_backward"}  # the switches every bf16 Chain pullback needs


def one_case(a, gn, g, cfg):
    import torch
    L = gn._lib
    BF = torch.bfloat16
    case = calls.chain_case(gn, g, cfg, dtype=BF)
    widen = lambda ts: [None if t is None else t.float() for t in ts]
    built = dict(native=calls.build(gn, case, "chain", "backward", L.ELEM_BF16, BF16_CHAIN | {"native_chain_backward"}),
                 staged=calls.build(gn, case, "chain", "backward", L.ELEM_BF16, BF16_CHAIN | {"narrow_chain_backward"}),  # (narrow = 1)
                 narrow_f32=calls.build(gn, case, "chain", "backward", L.ELEM_F32, "gnx_chain_block_backward_narrow", x=widen(case.x), cot=widen(case.cot)))
    rec = dict(in_dims=list(cfg[0]), edge=cfg[1], node=cfg[2], graph=cfg[3], E=g.n_edges, N=g.n_nodes, G=g.n_graphs,
               applies=calls.applies(gn, case, "gnx_chain_block_backward_narrow_applies"),
               native_applies=calls.applies(gn, case, "gnx_chain_block_backward_narrow_typed_applies", L.ELEM_BF16), register_width=buckets(cfg))
    ms = timing.cold_samples(torch, {k: c.f for k, c in built.items()}, a.samples, a.warmup)
    rec.update(forms={k: timing.summary_samples(v) for k, v in ms.items()}, workspace_bytes={k: c.nbytes for k, c in built.items()})
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int16 if t.dtype == BF else torch.int32)
    written = lambda c: [t for t in c.outs if t is not None] + c.grads
    rec["native_bits_equal_staged"] = all(torch.equal(bits(u), bits(v)) for u, v in zip(written(built["native"]), written(built["staged"])))
    f = rec["forms"]
    rec["native_over_staged"] = f["native"]["median_ms"] / f["staged"]["median_ms"]
    rec["native_over_narrow_f32"] = f["native"]["median_ms"] / f["narrow_f32"]["median_ms"]
    rec["not_slower_beyond_spread"] = bool(f["native"]["median_ms"] <= f["staged"]["median_ms"] + f["staged"]["spread_ms"])
    return rec


def run(a, graphs=None, limit=None):
    """the record; graphs: {key: GNGraphBatch} in place of the full-size ones, limit: the first cases only (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    out = timing.RecordWriter(a.out, device=torch.cuda.get_device_name(0), box="one MI355X; the three forms alternate in one process", samples=a.samples,
                              method=f"one call per sample between device events, 512 MiB overwritten in front of every sample (cache-cold), forms alternating, {a.warmup} warm-up "
                                     "calls each; all gradients wanted",
                              timing=timing.cold_timing(a.samples, a.warmup),
                              forms=dict(native="gnx_chain_block_backward_narrow_typed(GNX_ELEM_BF16) on bf16 tensors",
                                         staged="gnx_chain_block_backward_typed(GNX_ELEM_BF16, narrow = 1) on the same tensors",
                                         narrow_f32="gnx_chain_block_backward_narrow on fp32 tensors"), cases=[])
    get = timing.OneGraph(gn, graphs)
    cut = []
    for i, (key, cfg) in enumerate([(key, cfg) for key in ("C2", "hetero512") for cfg in CONFIGS][:limit]):
        gname = timing.GRAPHS[key][0]
        c = one_case(a, gn, get(key), cfg)
        c["graph_name"] = gname
        if c["native_applies"] and not c["not_slower_beyond_spread"]:
            cut.append(i)
        f = c["forms"]
        print(f"{gname} {cfg}: native {f['native']['median_ms']:.4f}   staged {f['staged']['median_ms']:.4f} (spread {f['staged']['spread_ms']:.4f})   "
              f"narrow fp32 {f['narrow_f32']['median_ms']:.4f} ms   native / staged {c['native_over_staged']:.3f}   ws {c['workspace_bytes']['native'] >> 20} / "
              f"{c['workspace_bytes']['staged'] >> 20} / {c['workspace_bytes']['narrow_f32'] >> 20} MiB   native {c['native_applies']}   "
              f"bits {c['native_bits_equal_staged']}", flush=True)
        out.res["native_slower_than_staged_beyond_spread"] = cut
        out.add("cases", c)  # (after every case: a run cut short leaves what it measured)
    return out.res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.chdir(HERE)
    run(a)


if __name__ == "__main__":
    main()
