"""Times the training entries of a Chain block with Dropout inside its update functions (gnx_chain_block_forward_train / _backward_train with
narrow = 1: every function inside the training rule in one kernel that regenerates its masks in registers — csrc/gnx_chain_train_narrow.hip,
csrc/gnx_chain_bw_train_narrow.hip) against the test-mode entries on the chains WITHOUT their Dropouts.  Shapes: the four blocks of
tools/time_chain_narrow.py's CONFIGS with a Dropout(0.1) behind every hidden Dense, on the 1M-edge / 100k-node graph (BASELINE configs[1], "C2")
and on the 512-graph batch of bench.py; forward and backward (all gradients wanted).

Forms, alternating sample by sample in one process:
  train_narrow   (a) the training call, narrow = 1
  generic        (b) gnx_chain_block_forward / gnx_chain_block_backward on the stripped chains: the generic test-mode entry, whose code this
                     change leaves as it was.  It does strictly less work than the generic TRAINING path (no mask passes): beating it is
                     beating that path
  narrow         (c) gnx_chain_block_forward_narrow / _backward_narrow on the stripped chains — informational: (a) / (c) is the price of the masks
  train_generic  the training call with narrow = 0 — informational, and for its workspace size
Every sample is ONE whole call between two device events, cache-cold: a 512 MiB buffer is overwritten in front of it (outside the events); 30
warm-up calls per form; medians, min / max and the spread (max - min) of 15 samples (tools/timing.py: cold_samples).
`slower_than_generic_beyond_spread`: (a)'s median > (b)'s median + (b)'s spread — a class (register width x source form, per direction) whose
measured cases are ALL slower in that sense is cut from the training rule (include/gnx.h).

  python tools/time_chain_train.py [--samples 15] [--out profiles/chain_train_narrow.json]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools import calls, timing  # noqa: E402
from tools.time_chain_narrow import CONFIGS, buckets  # noqa: E402

# form -> (a training call, the switches of its direction that are on)
FORMS = (("train_narrow", True, True), ("generic", False, False), ("narrow", False, True), ("train_generic", True, False))


def one_case(a, gn, g, cfg, backward):
    import torch
    from tests import chain_dropout_ref as DR
    F32 = gn._lib.ELEM_F32
    made = {}

    def make(p, keep):  # the block with its Dropouts (the case's own record) and, beside it, the chains without them
        made["drops"] = drops = DR.drop_after_hidden(p, 0.1)
        made["ent"], made["ent0"] = DR.entries(p, drops), DR.entries(p, {})
        owner = DR.block(gn, p, drops)
        cp, _, outw = owner._chain_train_params(keep)
        made["cp0"] = DR.block(gn, p, {})._chain_params(keep)[0]
        return owner, cp, outw

    case = calls.chain_case(gn, g, cfg, make=make)
    drops, ent = made["drops"], made["ent"]
    crec = gn.ChainDropout(12345, [[v if k == "dropout" else 0.0 for k, v in ent[name]] for name in DR.FN])._c(case.keep)
    direction = "backward" if backward else "forward"
    switch = "narrow_chain_backward" if backward else "narrow_chain"
    slots = lambda entries: {name: [None if kind == "dropout" else v for kind, v in entries[name]] for name in DR.FN}  # (a Dropout entry has no gradient)
    built = {}
    for key, train, narrow in FORMS:
        built[key] = calls.build(gn, case, "chain", direction, F32, {switch} if narrow else (), drop=crec if train else None, p=None if train else made["cp0"],
                                 layout=slots(ent if train else made["ent0"]))
    ms = timing.cold_samples(torch, {k: c.f for k, c in built.items()}, a.samples, a.warmup)
    f = {k: timing.summary_samples(v) for k, v in ms.items()}
    return dict(direction=direction, in_dims=list(cfg[0]), edge=cfg[1], node=cfg[2], graph=cfg[3], dropout_p=0.1,
                dropout_entries={name: len(drops[name]) for name in DR.FN}, E=g.n_edges, N=g.n_nodes, G=g.n_graphs,
                applies=calls.applies(gn, case, "gnx_chain_block_train_applies", int(backward)), register_width=buckets(cfg), forms=f,
                workspace_bytes={k: c.nbytes for k, c in built.items()},
                train_narrow_over_generic=f["train_narrow"]["median_ms"] / f["generic"]["median_ms"],
                train_narrow_over_narrow=f["train_narrow"]["median_ms"] / f["narrow"]["median_ms"],
                slower_than_generic_beyond_spread=bool(f["train_narrow"]["median_ms"] > f["generic"]["median_ms"] + f["generic"]["spread_ms"]))


def run(a, graphs=None, limit=None):
    """the record; graphs: {key: GNGraphBatch} in place of the full-size ones, limit: the first cases only (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    out = timing.RecordWriter(a.out, device=torch.cuda.get_device_name(0), box="one MI355X; every form timed in one process, alternating", samples=a.samples,
                              method=f"one call per sample between device events, 512 MiB overwritten in front of every sample (cache-cold), forms alternating, {a.warmup} warm-up "
                                     "calls each; backward: all gradients wanted; Dropout(0.1) behind every hidden Dense",
                              timing=timing.cold_timing(a.samples, a.warmup), cases=[])
    get = timing.OneGraph(gn, graphs)
    for key, cfg, backward in [(key, cfg, backward) for key in ("hetero512", "C2") for cfg in CONFIGS for backward in (False, True)][:limit]:
        gname = timing.GRAPHS[key][0]
        c = one_case(a, gn, get(key), cfg, backward)
        c["graph_name"] = gname
        f = c["forms"]
        print(f"{gname} {cfg} {c['direction']}: train_narrow {f['train_narrow']['median_ms']:.4f}  generic {f['generic']['median_ms']:.4f} "
              f"(spread {f['generic']['spread_ms']:.4f})  narrow {f['narrow']['median_ms']:.4f}  train_generic {f['train_generic']['median_ms']:.4f} ms   "
              f"applies {c['applies']}  ws {c['workspace_bytes']['train_narrow'] >> 20} / {c['workspace_bytes']['train_generic'] >> 20} MiB  "
              f"slower {c['slower_than_generic_beyond_spread']}", flush=True)
        out.res["slower_than_generic_beyond_spread"] = [i for i, q in enumerate(out.res["cases"] + [c]) if q["slower_than_generic_beyond_spread"]]
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
