"""Times gnx_chain_block_backward_narrow — the pullback of a Chain block with every update function inside the rule in one kernel
(csrc/gnx_chain_bw_narrow.hip) — against the call it stands in for: gnx_chain_block_backward of the PARENT commit's library.  Shapes: the
1M-edge / 100k-node graph (BASELINE configs[1], "C2") and the 512-graph batch of bench.py; on each the four blocks of
tools/time_chain_narrow.py's CONFIGS.  All gradients are wanted: the three input gradients and every layer's weight / bias gradient.

Every sample is ONE whole call between two device events, cache-cold: a 512 MiB buffer is overwritten in front of it (outside the events).
30 warm-up calls (settled clocks, loaded code objects); medians, min / max and the spread (max - min) of the samples are recorded, with the
workspace bytes of both calls.
`--parent-root DIR`: a checkout of the parent commit with its library built; it is timed there first, in a process of its own (this script
with --root DIR --baseline-only: one library per process), in the same session on the same device.  This build's own time for the untouched
gnx_chain_block_backward stands next to the parent's to show the two sessions overlap.  `not_slower_beyond_spread`: narrow median <= parent
median + the parent's spread — what a register-width bucket or source form has to meet to stay in the rule.  Without --parent-root the slots
of the parent stay empty.
`--accuracy-log FILE`: the output of `pytest tests/test_gpu_chain_bw_narrow.py -s`; the worst printed ratio of the narrow entry's error to its
bound (max(4 x the generic entry's error, 1e-5 max(1, max|ref|)) against float64) is recorded as `worst_ratio_to_bound`.

  python tools/time_chain_bw_narrow.py [--samples 21] [--parent-root DIR] [--accuracy-log FILE] [--out profiles/chain_bw_narrow.json]
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools.time_chain_narrow import CONFIGS, buckets, cold_samples, summary  # noqa: E402


def one_case(a, gn, g, cfg, baseline_only):
    import torch
    from oracle import gn_oracle as O
    from tests.test_gpu_chain import _block
    L, lib = gn._lib, gn._lib.load()
    rng = np.random.default_rng(0)
    p = O.make_chain_block_params(rng, *cfg)
    blk = _block(gn, p)
    keep = []
    cp, chains, outw = blk._chain_params(keep)
    s = torch.cuda.current_stream().cuda_stream
    rows = (g.n_edges, g.n_nodes, g.n_graphs)
    ptr = lambda t: None if t is None else t.data_ptr()
    x = [torch.from_numpy(rng.random((1, T, d), dtype=np.float32)).cuda() if d else None for T, d in zip(rows, cfg[0])]
    gout = [torch.from_numpy(rng.standard_normal((1, T, d)).astype(np.float32)).cuda() if d else None for T, d in zip(rows, outw)]

    def form(query, entry):
        nb = int(query(g._h, C.byref(cp), 1))
        assert nb > 0, lib.gnx_last_error()
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        dx = [None if t is None else torch.empty_like(t) for t in x]
        outs, arrays = [], []
        for name in ("edge", "node", "graph"):
            arr = (L.DenseGrad * max(len(p[name]), 1))()
            for i, (w, b, c) in enumerate(p[name]):
                gw = torch.empty(len(b) if isinstance(w, str) else w.size, dtype=torch.float32, device="cuda")
                gb = torch.empty(len(c) if isinstance(w, str) else len(b), dtype=torch.float32, device="cuda")
                outs += [gw, gb]
                arr[i] = L.DenseGrad(gw.data_ptr(), gb.data_ptr())
            arrays.append(arr)
        gr = L.ChainBlockGrads(*[C.cast(q, C.POINTER(L.DenseGrad)) for q in arrays])
        keep.extend(arrays)

        def call():
            assert entry(g._h, C.byref(cp), *map(ptr, x), *map(ptr, gout), 1, *map(ptr, dx), C.byref(gr), ws.data_ptr(), nb, s) == 0, lib.gnx_last_error()

        return call, nb, [t for t in dx if t is not None] + outs

    forms, wsb, outs = {}, {}, {}
    forms["chain"], wsb["chain"], outs["chain"] = form(lib.gnx_chain_block_backward_workspace_bytes, lib.gnx_chain_block_backward)
    rec = dict(in_dims=list(cfg[0]), edge=cfg[1], node=cfg[2], graph=cfg[3], E=g.n_edges, N=g.n_nodes, G=g.n_graphs)
    if not baseline_only:
        rec["applies"] = int(lib.gnx_chain_block_backward_narrow_applies(g._h, C.byref(cp), 1))
        rec["register_width"] = buckets(cfg)
        forms["narrow"], wsb["narrow"], outs["narrow"] = form(lib.gnx_chain_block_backward_narrow_workspace_bytes, lib.gnx_chain_block_backward_narrow)
    ms = cold_samples(torch, forms, a.samples, warmup=a.warmup)
    rec.update(forms={k: summary(v) for k, v in ms.items()}, workspace_bytes=wsb)
    if not baseline_only:  # the two calls of this build on the same inputs: how far apart the gradients are
        torch.cuda.synchronize()
        rec["max_diff_narrow_vs_chain_over_scale"] = max(float((u.double() - v.double()).abs().max() / max(1.0, float(v.double().abs().max())))
                                                         for u, v in zip(outs["narrow"], outs["chain"]) if u.numel())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--root", default=HERE, help="the checkout whose package and library are timed")
    ap.add_argument("--baseline-only", action="store_true", help="time gnx_chain_block_backward only and print one JSON line")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit, its library built")
    ap.add_argument("--accuracy-log", default=None, help="output of pytest tests/test_gpu_chain_bw_narrow.py -s")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parent = None
    if a.parent_root:  # first, and in a process of its own: one library per process
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", os.path.abspath(a.parent_root), "--baseline-only", "--samples", str(a.samples),
                            "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=560)
        assert r.returncode == 0, r.stderr[-3000:]
        parent = json.loads(r.stdout.strip().splitlines()[-1])["cases"]
    sys.path.insert(0, a.root)
    os.chdir(a.root)
    import torch
    import bench
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), box="one MI355X; parent and this build timed in one session, one process each", samples=a.samples,
               method=f"one call per sample between device events, 512 MiB overwritten in front of every sample (cache-cold), forms alternating, {a.warmup} warm-up "
                      "calls each; all gradients wanted",
               measured=bool(parent), cases=[])
    if a.accuracy_log:
        with open(a.accuracy_log) as fh:
            ratios = [float(v) for v in re.findall(r"chain bw narrow .*: worst narrow err / bound = ([0-9.e+-]+)", fh.read())]
        assert ratios, "no ratio line in the accuracy log"
        res["worst_ratio_to_bound"] = max(ratios)
        res["ratio_checks"] = len(ratios)
    graphs = (("C2: one graph, 100k nodes, 1M edges", lambda: gn.GNGraphBatch.from_csc(*bench.make_c2())),
              ("512 graphs of 32..256 nodes, 1M edges", lambda: gn.GNGraphBatch.from_csc(*bench.make_hetero(3))))
    cut = []
    for gname, make in graphs:
        g = make()
        for cfg in CONFIGS:
            c = one_case(a, gn, g, cfg, a.baseline_only)
            c["graph_name"] = gname
            i = len(res["cases"])
            res["cases"].append(c)
            if a.baseline_only:
                continue
            f = c["forms"]
            line = f"{gname} {cfg}: chain {f['chain']['median_ms']:.4f}   narrow {f['narrow']['median_ms']:.4f} ms   ws {c['workspace_bytes']['narrow'] >> 20} / " \
                   f"{c['workspace_bytes']['chain'] >> 20} MiB   applies {c['applies']}"
            if parent:
                pc = parent[i]
                assert pc["graph_name"] == gname and pc["in_dims"] == c["in_dims"] and pc["edge"] == c["edge"]
                base = pc["forms"]["chain"]
                c["parent"] = dict(forms=pc["forms"], workspace_bytes=pc["workspace_bytes"])
                c["narrow_over_parent"] = f["narrow"]["median_ms"] / base["median_ms"]
                c["not_slower_beyond_spread"] = bool(f["narrow"]["median_ms"] <= base["median_ms"] + base["spread_ms"])
                if not c["not_slower_beyond_spread"]:
                    cut.append(i)
                line += f"   parent {base['median_ms']:.4f} (spread {base['spread_ms']:.4f})   narrow / parent {c['narrow_over_parent']:.3f}"
            print(line, flush=True)
            if parent:
                res["slower_than_parent_beyond_spread"] = cut
            if a.out:  # (after every case: a run cut short leaves what it measured)
                with open(a.out, "w") as fh:
                    json.dump(res, fh, indent=1)
                    fh.write("\n")
        del g
    if a.baseline_only:
        print(json.dumps(res))


if __name__ == "__main__":
    main()
