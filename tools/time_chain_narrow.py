"""Times gnx_chain_block_forward_narrow — a Chain block with every narrow update function in one kernel (csrc/gnx_chain_narrow.hip) — against the
call it stands in for: gnx_chain_block_forward of the PARENT commit's library.  Shapes: the 1M-edge / 100k-node graph (BASELINE configs[1],
"C2") and the 512-graph batch of bench.py; on each the four blocks of CONFIGS.

Every sample is ONE whole call between two device events, cache-cold: a 512 MiB buffer is overwritten in front of it (outside the events).
30 warm-up calls (settled clocks, loaded code objects); medians, min / max and the spread (max - min) of the samples are recorded, with the
workspace bytes of both calls (tools/timing.py: cold_samples).
`--parent-root DIR`: a checkout of the parent commit with its library built; it is timed there first, in a process of its own (this script
with --root DIR --baseline-only: one library per process), in the same session on the same device.  This build's own time for the untouched
gnx_chain_block_forward stands next to the parent's to show the two sessions overlap.  `not_slower_beyond_spread`: narrow median <= parent
median + the parent's spread — what a register-width bucket or source form has to meet to stay in the rule.  Without --parent-root the slots
of the parent stay empty.

  python tools/time_chain_narrow.py [--samples 41] [--parent-root DIR] [--out profiles/chain_narrow.json]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools import calls, timing  # noqa: E402

CONFIGS = (((10, 5, 0), [16, 3], [8, 4], [6, 5]),
           ((10, 5, 3), [32, 32, 3], [32, 4], [16, 5]),
           ((3, 2, 1), [8, 8, 2], [8, 3], [8, 2]),
           ((10, 5, 3), [16, "ln", 16, 3], [16, 4], [5]))
WARMUP = 30


def buckets(cfg):
    """register width (8 / 16 / 32) of each fused function: the smallest that covers its input width and every layer width"""
    (de, dn, dg), ew, nw, gw = cfg
    last = lambda ws, k: next((w for w in reversed(ws) if w != "ln"), k if ws else 0)
    ke = de + 2 * dn + dg
    oe = last(ew, ke)
    kn = oe + dn + dg
    kg = oe + last(nw, kn) + dg
    b = lambda k, ws: next(w for w in (8, 16, 32) if w >= max([k] + [v for v in ws if v != "ln"]))
    return dict(edge=b(ke, ew), node=b(kn, nw), graph=b(kg, gw))


def one_case(a, gn, g, cfg, baseline_only):
    import torch
    F32 = gn._lib.ELEM_F32
    case = calls.chain_case(gn, g, cfg, cot=False)
    built = {"chain": calls.build(gn, case, "chain", "forward", F32, "gnx_chain_block_forward")}
    rec = dict(in_dims=list(cfg[0]), edge=cfg[1], node=cfg[2], graph=cfg[3], E=g.n_edges, N=g.n_nodes, G=g.n_graphs)
    if not baseline_only:
        rec["applies"] = calls.applies(gn, case, "gnx_chain_block_forward_narrow_applies")
        rec["register_width"] = buckets(cfg)
        built["narrow"] = calls.build(gn, case, "chain", "forward", F32, "gnx_chain_block_forward_narrow")
    ms = timing.cold_samples(torch, {k: c.f for k, c in built.items()}, a.samples, WARMUP)
    rec.update(forms={k: timing.summary_samples(v) for k, v in ms.items()}, workspace_bytes={k: c.nbytes for k, c in built.items()})
    if not baseline_only:  # the two calls of this build on the same inputs: how far apart the outputs are
        torch.cuda.synchronize()
        rec["max_diff_narrow_vs_chain_over_scale"] = max(float((u.double() - v.double()).abs().max() / max(1.0, float(v.double().abs().max())))
                                                         for u, v in zip(built["narrow"].outs, built["chain"].outs) if u is not None)
    return rec


def run(a, parent=None, graphs=None, limit=None):
    """the record; parent: the parent's cases; graphs: {key: GNGraphBatch} in place of the full-size ones, limit: the first cases only
    (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    out = timing.RecordWriter(None if a.baseline_only else a.out, device=torch.cuda.get_device_name(0),
                              box="one MI355X; parent and this build timed in one session, one process each", samples=a.samples,
                              method="one call per sample between device events, 512 MiB overwritten in front of every sample (cache-cold), forms alternating, 30 warm-up calls each",
                              timing=timing.cold_timing(a.samples, WARMUP), measured=bool(parent), cases=[])
    get = timing.OneGraph(gn, graphs)
    cut = []
    for i, (key, cfg) in enumerate([(key, cfg) for key in ("C2", "hetero512") for cfg in CONFIGS][:limit]):
        gname = timing.GRAPHS[key][0]
        c = one_case(a, gn, get(key), cfg, a.baseline_only)
        c["graph_name"] = gname
        if not a.baseline_only:
            f = c["forms"]
            line = f"{gname} {cfg}: chain {f['chain']['median_ms']:.4f}   narrow {f['narrow']['median_ms']:.4f} ms   ws {c['workspace_bytes']['narrow'] >> 20} / " \
                   f"{c['workspace_bytes']['chain'] >> 20} MiB   applies {c['applies']}"
            if parent:
                line += timing.against_parent(c, parent[i], i, cut)
                out.res["slower_than_parent_beyond_spread"] = cut
            print(line, flush=True)
        out.add("cases", c)  # (after every case: a run cut short leaves what it measured)
    return out.res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=41)
    ap.add_argument("--root", default=HERE, help="the checkout whose package and library are timed")
    ap.add_argument("--baseline-only", action="store_true", help="time gnx_chain_block_forward only and print one JSON line")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit, its library built")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parent = None
    if a.parent_root:  # first, and in a process of its own: one library per process
        parent = timing.parent_baseline(__file__, a.parent_root, ["--samples", a.samples], 500)["cases"]
    timing.child_root(a.root)
    res = run(a, parent)
    if a.baseline_only:
        timing.print_record(res)


if __name__ == "__main__":
    main()
