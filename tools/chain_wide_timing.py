"""Times gnx_chain_block_forward_wide — each update function of a Chain block at matrix-core widths in one kernel (csrc/gnx_chain_wide.hip) —
against the call it stands in for: gnx_chain_block_forward of the PARENT commit's library.  Shapes: the one-graph 1M-edge batch ("C2") and the
512-graph 1M-edge batch of bench.py; on each the four blocks of CONFIGS.

Every sample is ONE whole call between two device events, cache-cold (tools/timing.py: cold_samples); 30 warm-up calls; medians, min / max and the
spread (max - min) are recorded with the workspace bytes of both calls and the `_applies` mask.  `--parent-root DIR`: a checkout of the parent
commit with its library built; it is timed there first, in a process of its own (this script with --root DIR --baseline-only: one library per
process), in the same session on the same device.  In this build's process the new entry alternates with this build's untouched generic entry,
whose time stands next to the parent's to show the two sessions overlap.
`not_slower_beyond_spread`: wide median <= parent median + the parent's spread — what a class of the rule (accumulator blocks of each function x
source form x one graph or several) has to meet on every case that reaches it to stay in chain_wide_takes.
(The name stays outside tools/time_*.py: tests/test_timing_tools_cpu.py counts those files.  Built from tools/timing.py and tools/calls.py alone.)

`--backward`: the same comparison for the pullback — gnx_chain_block_backward_wide (csrc/gnx_chain_bw_wide.hip; the switch `wide_chain_backward`)
against gnx_chain_block_backward of the parent's library, all gradients wanted, on the same configs and batches; the class of a case is then
what chain_bw_wide_takes has to keep.

`--bf16`: the forward on bfloat16 features — gnx_chain_block_forward_wide_typed (csrc/gnx_chain_wide_bf16.hip; the switches `bf16_chain` +
`wide_chain`) against the parent's route for the same call, gnx_chain_block_forward_typed(narrow = 1) of the parent's library, on the two blocks of
BF16_CONFIGS and both batches; gnx_chain_block_forward_wide on the widened tensors is timed beside them for information.
`beats_parent_beyond_spread`: wide median < parent median - max(the parent's spread, the wide entry's spread) — what the native rule
(chain_wide_typed_native) has to meet on the 512-graph batch.

  python tools/chain_wide_timing.py [--samples 15] [--parent-root DIR] [--out profiles/chain_wide.json]
  python tools/chain_wide_timing.py --bf16 [--samples 15] [--parent-root DIR] [--out profiles/chain_wide_bf16.json]
  python tools/chain_wide_timing.py --backward [--samples 15] [--parent-root DIR] [--out profiles/chain_bw_wide.json]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools import calls, timing  # noqa: E402

WARMUP = 30
CONFIGS = [((10, 5, 0), [64, 3], [64, 4], [32, 5]),
           ((10, 5, 3), [64, 64, 3], [64, 4], [16, 5]),
           ((10, 5, 3), [128, "ln", 128, 3], [128, 4], [5]),
           ((32, 32, 8), [128, 128, 32], [128, 32], [64, 8])]
BF16_CONFIGS = [CONFIGS[1], CONFIGS[0]]


def blocks(widths):
    """32-column accumulator blocks of a function's widest Dense: 1 or 2 inside the rule; 3 and 4 count as 4, the class chain_wide_cut cuts"""
    nb = (max(w for w in widths if not isinstance(w, str)) + 31) // 32
    return 4 if nb == 3 else nb


def one_case_bf16(a, gn, g, cfg, baseline_only):
    """forms: "narrow" = gnx_chain_block_forward_typed(narrow = 1) on the bf16 tensors (the call the new entry stands in for), "wide" = the new
    entry on them, "wide_fp32" = gnx_chain_block_forward_wide on their widening"""
    import torch
    F32, BF16 = gn._lib.ELEM_F32, gn._lib.ELEM_BF16
    case = calls.chain_case(gn, g, cfg, dtype=torch.bfloat16, cot=False)
    built = {"narrow": calls.build(gn, case, "chain", "forward", BF16, "gnx_chain_block_forward_typed", narrow=1)}
    rec = dict(in_dims=list(cfg[0]), edge=cfg[1], node=cfg[2], graph=cfg[3], E=g.n_edges, N=g.n_nodes, G=g.n_graphs)
    if not baseline_only:
        rec["applies"] = calls.applies(gn, case, "gnx_chain_block_forward_wide_typed_applies", BF16)
        rec["class"] = dict(blocks={n: blocks(w) for n, w, bit in (("edge", cfg[1], 1), ("node", cfg[2], 2), ("graph", cfg[3], 4)) if rec["applies"] & bit},
                            graphs="one" if g.n_graphs == 1 else "several")
        built["wide"] = calls.build(gn, case, "chain", "forward", BF16, ("wide_chain", "bf16_chain"))
        built["wide_fp32"] = calls.build(gn, case, "chain", "forward", F32, ("wide_chain",), x=[None if t is None else t.float() for t in case.x])
    ms = timing.cold_samples(torch, {k: c.f for k, c in built.items()}, a.samples, WARMUP)
    rec.update(forms={k: timing.summary_samples(v) for k, v in ms.items()}, workspace_bytes={k: c.nbytes for k, c in built.items()})
    if not baseline_only:
        torch.cuda.synchronize()
        rec["bits_equal_to_bf16_of_fp32_wide"] = all(u is None or torch.equal(u.view(torch.int16), v.to(torch.bfloat16).view(torch.int16))
                                                     for u, v in zip(built["wide"].outs, built["wide_fp32"].outs))
        rec["profiler_one_call"] = {k: timing.profiled_once(gn, torch, c.f) for k, c in built.items()}
    return rec


def one_case(a, gn, g, cfg, baseline_only):
    if a.bf16:
        return one_case_bf16(a, gn, g, cfg, baseline_only)
    import torch
    F32 = gn._lib.ELEM_F32
    way = "backward" if a.backward else "forward"
    case = calls.chain_case(gn, g, cfg, cot=a.backward)
    built = {"generic": calls.build(gn, case, "chain", way, F32, "gnx_chain_block_" + way)}
    rec = dict(in_dims=list(cfg[0]), edge=cfg[1], node=cfg[2], graph=cfg[3], E=g.n_edges, N=g.n_nodes, G=g.n_graphs)
    if not baseline_only:
        rec["applies"] = calls.applies(gn, case, f"gnx_chain_block_{way}_wide_applies")
        rec["narrow_applies"] = calls.applies(gn, case, f"gnx_chain_block_{way}_narrow_applies")
        rec["class"] = dict(blocks={n: blocks(w) for n, w, bit in (("edge", cfg[1], 1), ("node", cfg[2], 2), ("graph", cfg[3], 4)) if rec["applies"] & bit},
                            graphs="one" if g.n_graphs == 1 else "several")
        built["wide"] = calls.build(gn, case, "chain", way, F32, ("wide_chain_backward",) if a.backward else ("wide_chain",))
    ms = timing.cold_samples(torch, {k: c.f for k, c in built.items()}, a.samples, WARMUP)
    rec.update(forms={k: timing.summary_samples(v) for k, v in ms.items()}, workspace_bytes={k: c.nbytes for k, c in built.items()})
    if not baseline_only:  # the two calls of this build on the same inputs: how far apart the outputs are
        torch.cuda.synchronize()
        rec["max_diff_wide_vs_generic_over_scale"] = max(float((u.double() - v.double()).abs().max() / max(1.0, float(v.double().abs().max())))
                                                         for u, v in zip(built["wide"].outs + built["wide"].grads, built["generic"].outs + built["generic"].grads) if u is not None)
        rec["profiler_one_call"] = {k: timing.profiled_once(gn, torch, c.f) for k, c in built.items()}
    return rec


def run(a, parent=None, graphs=None, limit=None):
    """the record; parent: the parent's cases; graphs: {key: GNGraphBatch} in place of the full-size ones, limit: the first cases only"""
    import torch
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    out = timing.RecordWriter(None if a.baseline_only else a.out, device=torch.cuda.get_device_name(0),
                              box="one MI355X; parent and this build timed in one session, one process each", samples=a.samples,
                              method="one call per sample between device events, 512 MiB overwritten in front of every sample (cache-cold), forms alternating, "
                                     "30 warm-up calls each",
                              timing=timing.cold_timing(a.samples, WARMUP), measured=bool(parent), cases=[])
    get = timing.OneGraph(gn, graphs)
    cut = []
    stood_in = "narrow" if a.bf16 else "generic"  # the form of the parent's library the new entry stands in for
    for i, (key, cfg) in enumerate([(key, cfg) for key in ("hetero512", "C2") for cfg in (BF16_CONFIGS if a.bf16 else CONFIGS)][:limit]):
        c = one_case(a, gn, get(key), cfg, a.baseline_only)
        c["graph_name"] = timing.GRAPHS[key][0]
        if not a.baseline_only:
            f = c["forms"]
            line = f"{c['graph_name']} {cfg}: {stood_in} {f[stood_in]['median_ms']:.4f}   wide {f['wide']['median_ms']:.4f} ms   ws {c['workspace_bytes']['wide'] >> 20} / " \
                   f"{c['workspace_bytes'][stood_in] >> 20} MiB   applies {c['applies']}   class {c['class']}"
            if parent:
                pc = parent[i]
                assert pc["graph_name"] == c["graph_name"] and pc["in_dims"] == c["in_dims"] and pc["edge"] == c["edge"]
                base = pc["forms"][stood_in]
                c["parent"] = dict(forms=pc["forms"], workspace_bytes=pc["workspace_bytes"])
                c["wide_over_parent"] = f["wide"]["median_ms"] / base["median_ms"]
                c["not_slower_beyond_spread"] = bool(f["wide"]["median_ms"] <= base["median_ms"] + base["spread_ms"])
                if a.bf16:
                    c["beats_parent_beyond_spread"] = bool(f["wide"]["median_ms"] < base["median_ms"] - max(base["spread_ms"], f["wide"]["spread_ms"]))
                if not c["not_slower_beyond_spread"]:
                    cut.append(i)
                out.res["slower_than_parent_beyond_spread"] = cut
                line += f"   parent {base['median_ms']:.4f} (spread {base['spread_ms']:.4f})   wide / parent {c['wide_over_parent']:.3f}"
            print(line, flush=True)
        out.add("cases", c)  # (after every case: a run cut short leaves what it measured)
    return out.res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--root", default=HERE, help="the checkout whose package and library are timed")
    ap.add_argument("--baseline-only", action="store_true", help="time gnx_chain_block_forward (--backward: gnx_chain_block_backward) only and print one JSON line")
    ap.add_argument("--backward", action="store_true", help="time the pullbacks: gnx_chain_block_backward_wide against gnx_chain_block_backward")
    ap.add_argument("--bf16", action="store_true", help="bfloat16 features: gnx_chain_block_forward_wide_typed against the parent's gnx_chain_block_forward_typed(narrow = 1)")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit, its library built")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parent = None
    if a.parent_root:  # first, and in a process of its own: one library per process
        parent = timing.parent_baseline(__file__, a.parent_root, ["--samples", a.samples] + (["--backward"] if a.backward else []) + (["--bf16"] if a.bf16 else []), 500)["cases"]
    timing.child_root(a.root)
    res = run(a, parent)
    if a.baseline_only:
        timing.print_record(res)


if __name__ == "__main__":
    main()
