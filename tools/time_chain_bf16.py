"""Times gnx_chain_block_forward_typed on bfloat16 features where it is native — every narrow update function of a Chain block in one kernel that
reads and writes bf16 rows (csrc/gnx_chain_narrow_bf16.hip) — against what a user did before it existed, and against the fp32 call.  Shapes and
blocks: those of tools/time_chain_narrow.py (the 512-graph 1M-edge batch of bench.py and the one-graph batch C2; its four CONFIGS).

Three forms alternate sample by sample in one process:
  typed      (a) gnx_chain_block_forward_typed(GNX_ELEM_BF16, narrow = 1) on bf16 tensors
  torch_cast (b) torch casts around gnx_chain_block_forward_narrow: .float() of every bf16 input, the fp32 call, .to(bfloat16) of every output
  narrow_f32 (c) gnx_chain_block_forward_narrow on fp32 tensors
Every sample is ONE whole call between two device events, cache-cold (512 MiB overwritten in front of it, outside the events); 30 warm-up calls;
medians of 15 samples, min / max and the spread of every form's samples, the workspace bytes of (a) and (c) (tools/timing.py: cold_samples).
`not_slower_beyond_spread`: (a)'s median <= (b)'s median + the spread of (b)'s samples — what a register width or source form has to meet to
stay in the native rule (include/gnx.h).

  python tools/time_chain_bf16.py [--samples 15] [--out profiles/chain_bf16.json]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools import calls, timing  # noqa: E402
from tools.time_chain_narrow import CONFIGS, buckets  # noqa: E402

WARMUP = 30


def one_case(a, gn, g, cfg):
    import torch
    L = gn._lib
    BF = torch.bfloat16
    case = calls.chain_case(gn, g, cfg, dtype=BF, cot=False)
    xw = [None if t is None else t.float() for t in case.x]
    typed = calls.build(gn, case, "chain", "forward", L.ELEM_BF16, {"bf16_chain", "narrow_chain"})  # (narrow = 1)
    narrow = calls.build(gn, case, "chain", "forward", L.ELEM_F32, "gnx_chain_block_forward_narrow", x=xw)
    cast_out = []

    def torch_cast():
        narrow.f(x=[None if t is None else t.float() for t in case.x])
        cast_out[:] = [None if t is None else t.to(BF) for t in narrow.outs]

    rec = dict(in_dims=list(cfg[0]), edge=cfg[1], node=cfg[2], graph=cfg[3], E=g.n_edges, N=g.n_nodes, G=g.n_graphs,
               applies=calls.applies(gn, case, "gnx_chain_block_forward_narrow_applies"),
               typed_applies=calls.applies(gn, case, "gnx_chain_block_forward_typed_applies", L.ELEM_BF16, 1), register_width=buckets(cfg))
    ms = timing.cold_samples(torch, dict(typed=typed.f, torch_cast=torch_cast, narrow_f32=narrow.f), a.samples, WARMUP)
    rec.update(forms={k: timing.summary_samples(v) for k, v in ms.items()}, workspace_bytes=dict(typed=typed.nbytes, narrow_f32=narrow.nbytes))
    torch.cuda.synchronize()
    same = lambda u, v: torch.equal(u.view(torch.int16), v.view(torch.int16))
    rec["typed_bits_equal_torch_cast"] = all(same(u, v) for u, v in zip(typed.outs, cast_out) if u is not None)
    f = rec["forms"]
    rec["typed_over_torch_cast"] = f["typed"]["median_ms"] / f["torch_cast"]["median_ms"]
    rec["typed_over_narrow_f32"] = f["typed"]["median_ms"] / f["narrow_f32"]["median_ms"]
    rec["not_slower_beyond_spread"] = bool(f["typed"]["median_ms"] <= f["torch_cast"]["median_ms"] + f["torch_cast"]["spread_ms"])
    return rec


def run(a, graphs=None, limit=None):
    """the record; graphs: {key: GNGraphBatch} in place of the full-size ones, limit: the first cases only (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    out = timing.RecordWriter(a.out, device=torch.cuda.get_device_name(0), box="one MI355X; the three forms alternate in one process", samples=a.samples,
                              method="one call per sample between device events, 512 MiB overwritten in front of every sample (cache-cold), forms alternating, 30 warm-up calls each",
                              timing=timing.cold_timing(a.samples, WARMUP),
                              forms=dict(typed="gnx_chain_block_forward_typed(GNX_ELEM_BF16, narrow = 1) on bf16 tensors",
                                         torch_cast=".float() of every bf16 input, gnx_chain_block_forward_narrow, .to(bfloat16) of every output",
                                         narrow_f32="gnx_chain_block_forward_narrow on fp32 tensors"), cases=[])
    get = timing.OneGraph(gn, graphs)
    cut = []
    for i, (key, cfg) in enumerate([(key, cfg) for key in ("hetero512", "C2") for cfg in CONFIGS][:limit]):
        gname = timing.GRAPHS[key][0]
        c = one_case(a, gn, get(key), cfg)
        c["graph_name"] = gname
        if not c["not_slower_beyond_spread"]:
            cut.append(i)
        f = c["forms"]
        print(f"{gname} {cfg}: typed {f['typed']['median_ms']:.4f}   torch casts {f['torch_cast']['median_ms']:.4f} (spread {f['torch_cast']['spread_ms']:.4f})   "
              f"narrow fp32 {f['narrow_f32']['median_ms']:.4f} ms   typed / casts {c['typed_over_torch_cast']:.3f}   ws {c['workspace_bytes']['typed'] >> 20} / "
              f"{c['workspace_bytes']['narrow_f32'] >> 20} MiB   native {c['typed_applies']}   bits {c['typed_bits_equal_torch_cast']}", flush=True)
        out.res["slower_than_torch_cast_beyond_spread"] = cut
        out.add("cases", c)  # (after every case: a run cut short leaves what it measured)
    return out.res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.chdir(HERE)
    run(a)


if __name__ == "__main__":
    main()
