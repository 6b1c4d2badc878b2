"""Times gnx_chain_block_forward_wave — a Chain block's edge and node function in one wave-per-tile kernel, the graph function from its partial rows
(csrc/gnx_chain_wave.hip) — against the call it stands in for: gnx_chain_block_forward_narrow of the PARENT commit's library.  Shapes: the
512-graph 1M-edge batch and the one-graph 1M-edge batch of bench.py; on each the four blocks of tools/time_chain_narrow.py's CONFIGS.

Every sample is ONE whole call between two device events, cache-cold (tools/timing.py: cold_samples); 30 warm-up calls; medians, min / max and the
spread (max - min) are recorded with the workspace bytes of both calls.  `--parent-root DIR`: a checkout of the parent commit with its library
built; it is timed there first, in a process of its own (this script with --root DIR --baseline-only), in the same session on the same device.
This build's own time for the untouched narrow entry stands next to the parent's to show the two sessions overlap.
`not_slower_beyond_spread`: wave median <= parent median + the parent's spread — what a class of the rule (register width x waves per workgroup)
has to meet on every case that reaches it to stay in chain_wave_takes.
`--bf16`: the same eight cases on bfloat16 features — gnx_chain_block_forward_wave_typed (csrc/gnx_chain_wave_bf16.hip) against
gnx_chain_block_forward_typed(narrow = 1) of the parent's library, with gnx_chain_block_forward_wave on the widened fp32 tensors beside it; the
class then has the bf16 form's slice max(cap (oe | 1), 64 (on | 1)); the record goes to profiles/chain_wave_bf16.json.
(The name stays outside tools/time_*.py: tests/test_timing_tools_cpu.py counts those files.  Built from tools/timing.py and tools/calls.py alone.)

  python tools/chain_wave_timing.py [--bf16] [--samples 15] [--parent-root DIR] [--out profiles/chain_wave.json]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools import calls, timing  # noqa: E402
from tools.time_chain_narrow import CONFIGS, buckets  # noqa: E402

WARMUP = 30
CAP = 128  # the default wave-tile edge cap


def rule_class(cfg, bf16=False):
    """(register width, waves per workgroup) of the wave kernel for cfg: include/gnx.h's LDS rule restated (bf16: the typed entry's slice)"""
    (de, dn, dg), ew, nw, _ = cfg
    c4 = lambda x: (x + 3) & ~3
    last = lambda ws, k: next((w for w in reversed(ws) if w != "ln"), k)

    def par(k, ws):
        n = 0
        for w in ws:
            n, k = (n + 2 * c4(k), k) if w == "ln" else (n + c4(k) * c4(w) + c4(w), w)
        return n

    ke = de + 2 * dn + dg
    oe = last(ew, ke)
    on = last(nw, oe + dn + dg)
    fit = (16384 - par(ke, ew) - par(oe + dn + dg, nw)) // max(CAP * (oe | 1), 64 * (on | 1) if bf16 else 0)
    b = buckets(cfg)
    return dict(register_width=max(b["edge"], b["node"]), waves_per_workgroup=4 if fit >= 4 else 2 if fit >= 2 else 0)


def one_case_bf16(a, gn, g, cfg, baseline_only):
    """forms: "narrow" = gnx_chain_block_forward_typed(narrow = 1) on the bf16 tensors (the call the new entry stands in for), "wave" = the new
    entry on them, "wave_fp32" = gnx_chain_block_forward_wave on their widening"""
    import torch
    F32, BF16 = gn._lib.ELEM_F32, gn._lib.ELEM_BF16
    case = calls.chain_case(gn, g, cfg, dtype=torch.bfloat16, cot=False)
    built = {"narrow": calls.build(gn, case, "chain", "forward", BF16, "gnx_chain_block_forward_typed", narrow=1)}
    rec = dict(in_dims=list(cfg[0]), edge=cfg[1], node=cfg[2], graph=cfg[3], E=g.n_edges, N=g.n_nodes, G=g.n_graphs)
    if not baseline_only:
        rec["applies"] = calls.applies(gn, case, "gnx_chain_block_forward_wave_typed_applies", BF16)
        rec["class"] = rule_class(cfg, bf16=True)
        built["wave"] = calls.build(gn, case, "chain", "forward", BF16, ("wave_chain", "bf16_chain"))
        built["wave_fp32"] = calls.build(gn, case, "chain", "forward", F32, ("wave_chain",), x=[None if t is None else t.float() for t in case.x])
    ms = timing.cold_samples(torch, {k: c.f for k, c in built.items()}, a.samples, WARMUP)
    rec.update(forms={k: timing.summary_samples(v) for k, v in ms.items()}, workspace_bytes={k: c.nbytes for k, c in built.items()})
    if not baseline_only:
        torch.cuda.synchronize()
        rec["bits_equal_to_bf16_of_fp32_wave"] = all(u is None or torch.equal(u.view(torch.int16), v.to(torch.bfloat16).view(torch.int16))
                                                     for u, v in zip(built["wave"].outs, built["wave_fp32"].outs))
        rec["profiler_one_call"] = {k: timing.profiled_once(gn, torch, c.f) for k, c in built.items()}
    return rec


def one_case(a, gn, g, cfg, baseline_only):
    if a.bf16:
        return one_case_bf16(a, gn, g, cfg, baseline_only)
    import torch
    F32 = gn._lib.ELEM_F32
    case = calls.chain_case(gn, g, cfg, cot=False)
    built = {"narrow": calls.build(gn, case, "chain", "forward", F32, "gnx_chain_block_forward_narrow")}
    rec = dict(in_dims=list(cfg[0]), edge=cfg[1], node=cfg[2], graph=cfg[3], E=g.n_edges, N=g.n_nodes, G=g.n_graphs)
    if not baseline_only:
        rec["applies"] = calls.applies(gn, case, "gnx_chain_block_forward_wave_applies")
        rec["class"] = rule_class(cfg)
        built["wave"] = calls.build(gn, case, "chain", "forward", F32, ("wave_chain",))
    ms = timing.cold_samples(torch, {k: c.f for k, c in built.items()}, a.samples, WARMUP)
    rec.update(forms={k: timing.summary_samples(v) for k, v in ms.items()}, workspace_bytes={k: c.nbytes for k, c in built.items()})
    if not baseline_only:
        torch.cuda.synchronize()
        rec["ef_nf_bits_equal_narrow"] = all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(built["wave"].outs[:2], built["narrow"].outs[:2]))
        rec["profiler_one_call"] = {k: timing.profiled_once(gn, torch, c.f) for k, c in built.items()}
    return rec


def run(a, parent=None, graphs=None, limit=None):
    """the record; parent: the parent's cases; graphs: {key: GNGraphBatch} in place of the full-size ones, limit: the first cases only"""
    import torch
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    out = timing.RecordWriter(None if a.baseline_only else a.out, device=torch.cuda.get_device_name(0),
                              box="one MI355X; parent and this build timed in one session, one process each", samples=a.samples,
                              method="one call per sample between device events, 512 MiB overwritten in front of every sample (cache-cold), forms alternating, 30 warm-up calls each",
                              timing=timing.cold_timing(a.samples, WARMUP), measured=bool(parent), cases=[])
    get = timing.OneGraph(gn, graphs)
    cut = []
    for i, (key, cfg) in enumerate([(key, cfg) for key in ("hetero512", "C2") for cfg in CONFIGS][:limit]):
        c = one_case(a, gn, get(key), cfg, a.baseline_only)
        c["graph_name"] = timing.GRAPHS[key][0]
        if not a.baseline_only:
            f = c["forms"]
            line = f"{c['graph_name']} {cfg}: narrow {f['narrow']['median_ms']:.4f}   wave {f['wave']['median_ms']:.4f} ms   applies {c['applies']}   class {c['class']}"
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
    ap.add_argument("--baseline-only", action="store_true", help="time gnx_chain_block_forward_narrow only and print one JSON line")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit, its library built")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bf16", action="store_true", help="bfloat16 features: gnx_chain_block_forward_wave_typed against the parent's gnx_chain_block_forward_typed(narrow = 1)")
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
