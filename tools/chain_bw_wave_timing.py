"""Times gnx_chain_block_backward_wave — the pullback of a Chain block with the node and the edge function in one wave-per-tile kernel
(csrc/gnx_chain_bw_wave.hip) — against the call it stands in for: gnx_chain_block_backward_narrow of the PARENT commit's library.  Shapes: the
one-graph 1M-edge batch ("C2") and the 512-graph 1M-edge batch of bench.py; on each the four blocks of tools/time_chain_narrow.py's CONFIGS.
All gradients are wanted: the three input gradients and every layer's weight / bias gradient.

Every sample is ONE whole call between two device events, cache-cold (tools/timing.py: cold_samples); 30 warm-up calls; medians, min / max and the
spread (max - min) are recorded with the workspace bytes of both calls and `_applies`.  `--parent-root DIR`: a checkout of the parent commit with
its library built; it is timed there first, in a process of its own (this script with --root DIR --baseline-only: one library per process), in
the same session on the same device.  In this build's process the new entry alternates with this build's untouched narrow entry, whose time
stands next to the parent's to show the two sessions overlap.
`not_slower_beyond_spread`: wave median <= parent median + the parent's spread — what a class of the rule (register width x one graph or several)
has to meet on every case that reaches it to stay in chain_bw_wave_takes.
`--bf16`: the same for gnx_chain_block_backward_wave_typed on bfloat16 features (csrc/gnx_chain_bw_wave_bf16.hip).  The call it stands in for, and
the parent's baseline, is gnx_chain_block_backward_narrow_typed on the same bf16 tensors — what `wave_chain_backward` with `bf16_chain`,
`bf16_backward` and `native_chain_backward` ran before; the fp32 wave pullback on the widened tensors is timed beside both ("wave_f32").
(The name stays outside tools/time_*.py: tests/test_timing_tools_cpu.py counts those files.  Built from tools/timing.py and tools/calls.py alone.)

  python tools/chain_bw_wave_timing.py [--samples 15] [--parent-root DIR] [--out profiles/chain_bw_wave.json]
  python tools/chain_bw_wave_timing.py --bf16 [--samples 15] [--parent-root DIR] [--out profiles/chain_bw_wave_bf16.json]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools import calls, timing  # noqa: E402
from tools.time_chain_narrow import CONFIGS, buckets  # noqa: E402

WARMUP = 30
BF16_CHAIN = ("bf16_chain", "bf16_backward")  # the switches every bf16 Chain pullback needs


def one_case(a, gn, g, cfg, baseline_only):
    import torch
    F32, BF16 = gn._lib.ELEM_F32, gn._lib.ELEM_BF16
    if a.bf16:
        case = calls.chain_case(gn, g, cfg, dtype=torch.bfloat16)
        built = {"narrow": calls.build(gn, case, "chain", "backward", BF16, BF16_CHAIN + ("native_chain_backward",))}
    else:
        case = calls.chain_case(gn, g, cfg)
        built = {"narrow": calls.build(gn, case, "chain", "backward", F32, "gnx_chain_block_backward_narrow")}
    rec = dict(in_dims=list(cfg[0]), edge=cfg[1], node=cfg[2], graph=cfg[3], E=g.n_edges, N=g.n_nodes, G=g.n_graphs)
    if not baseline_only:
        b = buckets(cfg)
        rec["applies"] = calls.applies(gn, case, "gnx_chain_block_backward_wave_typed_applies", BF16) if a.bf16 else \
            calls.applies(gn, case, "gnx_chain_block_backward_wave_applies")
        rec["narrow_applies"] = calls.applies(gn, case, "gnx_chain_block_backward_narrow_applies")
        rec["class"] = dict(register_width=max(b["edge"], b["node"]), graphs="one" if g.n_graphs == 1 else "several")
        if a.bf16:
            widen = lambda ts: [None if t is None else t.float() for t in ts]
            built["wave"] = calls.build(gn, case, "chain", "backward", BF16, BF16_CHAIN + ("wave_chain_backward",))
            built["wave_f32"] = calls.build(gn, case, "chain", "backward", F32, ("wave_chain_backward",), x=widen(case.x), cot=widen(case.cot))
        else:
            built["wave"] = calls.build(gn, case, "chain", "backward", F32, ("wave_chain_backward",))
    ms = timing.cold_samples(torch, {k: c.f for k, c in built.items()}, a.samples, WARMUP)
    rec.update(forms={k: timing.summary_samples(v) for k, v in ms.items()}, workspace_bytes={k: c.nbytes for k, c in built.items()})
    if not baseline_only:  # the two calls of this build on the same inputs: how far apart the gradients are
        torch.cuda.synchronize()
        written = lambda c: [t for t in c.outs if t is not None] + c.grads
        if a.bf16:  # the contract: to_bf16 of the fp32 wave pullback's input gradients, its parameter gradients' bits
            bits = lambda t: t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
            w, f32 = built["wave"], built["wave_f32"]
            rec["wave_bits_equal_rounded_wave_f32"] = bool(
                all(torch.equal(bits(u), bits(v.to(torch.bfloat16))) for u, v in zip(w.outs, f32.outs) if u is not None) and
                all(torch.equal(bits(u), bits(v)) for u, v in zip(w.grads, f32.grads))) if rec["applies"] else None
            rec["wave_over_wave_f32"] = None
        rec["max_diff_wave_vs_narrow_over_scale"] = max(float((u.double() - v.double()).abs().max() / max(1.0, float(v.double().abs().max())))
                                                        for u, v in zip(written(built["wave"]), written(built["narrow"])) if u.numel())
        rec["profiler_one_call"] = {k: timing.profiled_once(gn, torch, c.f) for k, c in built.items()}
    if a.bf16 and not baseline_only:
        rec["wave_over_wave_f32"] = rec["forms"]["wave"]["median_ms"] / rec["forms"]["wave_f32"]["median_ms"]
    return rec


def run(a, parent=None, graphs=None, limit=None):
    """the record; parent: the parent's cases; graphs: {key: GNGraphBatch} in place of the full-size ones, limit: the first cases only"""
    import torch
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    out = timing.RecordWriter(None if a.baseline_only else a.out, device=torch.cuda.get_device_name(0),
                              box="one MI355X; parent and this build timed in one session, one process each", samples=a.samples,
                              method="one call per sample between device events, 512 MiB overwritten in front of every sample (cache-cold), forms alternating, "
                                     "30 warm-up calls each; all gradients wanted",
                              timing=timing.cold_timing(a.samples, WARMUP), measured=bool(parent), cases=[])
    get = timing.OneGraph(gn, graphs)
    cut = []
    for i, (key, cfg) in enumerate([(key, cfg) for key in ("C2", "hetero512") for cfg in CONFIGS][:limit]):
        c = one_case(a, gn, get(key), cfg, a.baseline_only)
        c["graph_name"] = timing.GRAPHS[key][0]
        if not a.baseline_only:
            f = c["forms"]
            if a.bf16:
                print(f"  wave fp32 on fp32 tensors {f['wave_f32']['median_ms']:.4f} ms   bf16 / fp32 {c['wave_over_wave_f32']:.3f}   "
                      f"bits {c['wave_bits_equal_rounded_wave_f32']}", flush=True)
            line = f"{c['graph_name']} {cfg}: narrow {f['narrow']['median_ms']:.4f}   wave {f['wave']['median_ms']:.4f} ms   ws {c['workspace_bytes']['wave'] >> 20} / " \
                   f"{c['workspace_bytes']['narrow'] >> 20} MiB   applies {c['applies']}   class {c['class']}"
            if parent:
                pc = parent[i]
                assert pc["graph_name"] == c["graph_name"] and pc["in_dims"] == c["in_dims"] and pc["edge"] == c["edge"]
                base = pc["forms"]["narrow"]
                c["parent"] = dict(forms=pc["forms"], workspace_bytes=pc["workspace_bytes"])
                c["wave_over_parent"] = f["wave"]["median_ms"] / base["median_ms"]
                c["not_slower_beyond_spread"] = bool(f["wave"]["median_ms"] <= base["median_ms"] + base["spread_ms"])
                if not c["not_slower_beyond_spread"]:
                    cut.append(i)
                out.res["slower_than_parent_beyond_spread"] = cut
                line += f"   parent {base['median_ms']:.4f} (spread {base['spread_ms']:.4f})   wave / parent {c['wave_over_parent']:.3f}"
            print(line, flush=True)
        out.add("cases", c)  # (after every case: a run cut short leaves what it measured)
    return out.res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--root", default=HERE, help="the checkout whose package and library are timed")
    ap.add_argument("--baseline-only", action="store_true", help="time gnx_chain_block_backward_narrow only and print one JSON line")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit, its library built")
    ap.add_argument("--bf16", action="store_true", help="gnx_chain_block_backward_wave_typed on bfloat16 features against gnx_chain_block_backward_narrow_typed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parent = None
    if a.parent_root:  # first, and in a process of its own: one library per process
        parent = timing.parent_baseline(__file__, a.parent_root, ["--samples", a.samples] + (["--bf16"] if a.bf16 else []), 500)["cases"]
    timing.child_root(a.root)
    res = run(a, parent)
    if a.baseline_only:
        timing.print_record(res)


if __name__ == "__main__":
    main()
