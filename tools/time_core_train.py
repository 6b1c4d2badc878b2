"""Times gnx_core_forward_train_typed — a GNCore's training-mode forward with the Dropout mask applied inside one FeedForward kernel per entity
where the core is narrow (csrc/gnx_core_train_narrow.hip) — in fp32 and bf16, against the call it stands in for: gnx_core_forward_train of the
PARENT commit, and for bf16 against torch casts around that parent call (three .float() in front, three .to(bfloat16) behind).  Graph: the
1M-edge Erdős–Rényi graph (BASELINE configs[1], "C2"); widths (10,5,3) README ex.3, (16,16,16) examples/train_sort.py's default, (3,4,5) and
(1,1,1); p = 0.1.

Every sample is ONE whole call between two device events, cache-cold: a 512 MiB buffer is overwritten in front of it (outside the events), so
no call finds its inputs or weights in the L2 / MALL the previous one left.  The forms of a process alternate sample by sample after a warm-up
of 30 calls each (settled clocks, loaded code objects); medians, min / max and the spread (max - min) of the samples are recorded, with the
workspace bytes of every form (tools/timing.py: cold_samples).
`--parent-root DIR`: a checkout of the parent commit with its library built; its forms are timed there first, in a process of its own (this
script with --root DIR --baseline-only: one library per process), in the same session on the same device.  This build's own time for the
untouched gnx_core_forward_train stands next to the parent's to show the two sessions overlap.  `not_slower_beyond_spread`: typed median <=
parent median + the parent's spread — what a width has to meet to stay in gnx_core_train_fused_applies.

  python tools/time_core_train.py [--samples 41] [--parent-root DIR] [--out profiles/core_train_narrow.json]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools import calls, timing  # noqa: E402

WIDTHS = ((10, 5, 3), (16, 16, 16), (3, 4, 5), (1, 1, 1))
P_DROP = 0.1
WARMUP = 30


def one_width(a, gn, g, dims, baseline_only):
    import torch
    L = gn._lib
    case = calls.core_case(gn, g, dims, cot=False)
    x16 = [t.to(torch.bfloat16) for t in case.x]
    drop = L.Dropout(P_DROP, 0, 12345)
    train = calls.build(gn, case, "core", "forward", L.ELEM_F32, "gnx_core_forward_train", drop=drop)

    def casts():
        train.f(x=[t.float() for t in x16])
        return [t.to(torch.bfloat16) for t in train.outs]

    forms, ws = {"train_f32": train.f, "train_with_torch_casts_bf16": casts}, {"train_f32": train.nbytes, "train_with_torch_casts_bf16": train.nbytes}
    if not baseline_only:
        for key, elem, x in (("typed_f32", L.ELEM_F32, case.x), ("typed_bf16", L.ELEM_BF16, x16)):
            assert calls.applies(gn, case, "gnx_core_train_fused_applies", elem) == 1, (dims, key)
            # (the fp32 typed call writes the outputs of the untyped one, as in every record of this tool)
            typed = calls.build(gn, case, "core", "forward", elem, "gnx_core_forward_train_typed", drop=drop, x=x, outs=train.outs if key == "typed_f32" else None)
            forms[key], ws[key] = typed.f, typed.nbytes
    ms = timing.cold_samples(torch, forms, a.samples, WARMUP)
    rec = dict(dims=list(dims), E=g.n_edges, N=g.n_nodes, G=g.n_graphs, p=P_DROP, forms={k: timing.summary_samples(v) for k, v in ms.items()}, workspace_bytes=ws)
    if not baseline_only:  # the two forms of this build on the same inputs: how far apart the outputs are (the unfused form carries f_fused - f_unfused)
        train.f()
        ref = [t.clone() for t in train.outs]
        forms["typed_f32"]()
        torch.cuda.synchronize()
        rec["max_diff_typed_f32_vs_train_over_scale"] = max(float((u.double() - v.double()).abs().max() / max(1.0, float(v.double().abs().max())))
                                                            for u, v in zip(train.outs, ref))
    return rec


def run(a, parent=None, graphs=None, limit=None):
    """the record; parent: {dims: the parent's width}; graphs: {key: GNGraphBatch} in place of C2, limit: the first widths only
    (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    out = timing.RecordWriter(None if a.baseline_only else a.out, device=torch.cuda.get_device_name(0),
                              box="one MI355X; parent and this build timed in one session, one process each", samples=a.samples,
                              method="one call per sample between device events, 512 MiB overwritten in front of every sample (cache-cold), forms alternating, 30 warm-up calls each",
                              timing=timing.cold_timing(a.samples, WARMUP), widths=[])
    c2 = timing.graph(gn, "C2", graphs)
    cut = []
    for dims in WIDTHS[:limit]:
        c = one_width(a, gn, c2, dims, a.baseline_only)
        if a.baseline_only:
            out.add("widths", c)
            continue
        f = c["forms"]
        line = f"{tuple(dims)}: train {f['train_f32']['median_ms']:.4f}   typed f32 {f['typed_f32']['median_ms']:.4f}   typed bf16 {f['typed_bf16']['median_ms']:.4f}   " \
               f"casts {f['train_with_torch_casts_bf16']['median_ms']:.4f} ms   ws {c['workspace_bytes']['typed_f32'] >> 20} / {c['workspace_bytes']['typed_bf16'] >> 20} / " \
               f"{c['workspace_bytes']['train_f32'] >> 20} MiB"
        if parent:
            pf = parent[tuple(dims)]["forms"]
            c["parent"] = dict(forms=pf, workspace_bytes=parent[tuple(dims)]["workspace_bytes"])
            base, casts = pf["train_f32"], pf["train_with_torch_casts_bf16"]
            c["typed_f32_over_parent_train"] = f["typed_f32"]["median_ms"] / base["median_ms"]
            c["typed_bf16_over_parent_train"] = f["typed_bf16"]["median_ms"] / base["median_ms"]
            c["typed_bf16_over_parent_train_with_casts"] = f["typed_bf16"]["median_ms"] / casts["median_ms"]
            c["not_slower_beyond_spread"] = dict(f32=bool(f["typed_f32"]["median_ms"] <= base["median_ms"] + base["spread_ms"]),
                                                 bf16=bool(f["typed_bf16"]["median_ms"] <= base["median_ms"] + base["spread_ms"]))
            if not all(c["not_slower_beyond_spread"].values()):
                cut.append(list(dims))
            line += f"   parent train {base['median_ms']:.4f} (spread {base['spread_ms']:.4f}), with casts {casts['median_ms']:.4f}   f32 / parent {c['typed_f32_over_parent_train']:.3f}" \
                    f"   bf16 / parent {c['typed_bf16_over_parent_train']:.3f}   bf16 / casts {c['typed_bf16_over_parent_train_with_casts']:.3f}"
            out.res["slower_than_parent_beyond_spread"] = cut
            out.res["cut_from_gnx_core_train_fused_applies"] = "No width is cut" if not cut else "see the header: include/gnx.h"
        print(line, flush=True)
        out.add("widths", c)  # (after every width: a run cut short leaves what it measured)
    return out.res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=41)
    ap.add_argument("--root", default=HERE, help="the checkout whose package and library are timed")
    ap.add_argument("--baseline-only", action="store_true", help="time gnx_core_forward_train (and the torch casts around it) only and print one JSON line")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit, its library built")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parent = None
    if a.parent_root:  # first, and in a process of its own: one library per process
        parent = {tuple(c["dims"]): c for c in timing.parent_baseline(__file__, a.parent_root, ["--samples", a.samples], 900)["widths"]}
    timing.child_root(a.root)
    res = run(a, parent)
    if a.baseline_only:
        timing.print_record(res)


if __name__ == "__main__":
    main()
