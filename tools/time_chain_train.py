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
warm-up calls per form; medians, min / max and the spread (max - min) of 15 samples.  `slower_than_generic_beyond_spread`: (a)'s median >
(b)'s median + (b)'s spread — a class (register width x source form, per direction) whose measured cases are ALL slower in that sense is cut
from the training rule (include/gnx.h).

  python tools/time_chain_train.py [--samples 15] [--out profiles/chain_train_narrow.json]
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


def one_case(a, gn, g, cfg, backward):
    import torch
    from oracle import gn_oracle as O
    from tests import chain_dropout_ref as DR
    L, lib = gn._lib, gn._lib.load()
    rng = np.random.default_rng(0)
    p = O.make_chain_block_params(rng, *cfg)
    drops = DR.drop_after_hidden(p, 0.1)
    ent, ent0 = DR.entries(p, drops), DR.entries(p, {})
    keep = []
    cp, _, outw = DR.block(gn, p, drops)._chain_train_params(keep)
    cp0 = DR.block(gn, p, {})._chain_params(keep)[0]
    rec = gn.ChainDropout(12345, [[v if k == "dropout" else 0.0 for k, v in ent[name]] for name in DR.FN])
    crec = rec._c(keep)
    s = torch.cuda.current_stream().cuda_stream
    rows = (g.n_edges, g.n_nodes, g.n_graphs)
    ptr = lambda t: None if t is None else t.data_ptr()
    x = [torch.from_numpy(rng.random((1, T, d), dtype=np.float32)).cuda() if d else None for T, d in zip(rows, cfg[0])]
    gout = [torch.from_numpy(rng.standard_normal((1, T, d)).astype(np.float32)).cuda() if d else None for T, d in zip(rows, outw)]

    def grads(entries):
        outs, arrays = [], []
        for name in DR.FN:
            arr = (L.DenseGrad * max(len(entries[name]), 1))()
            for e, (kind, v) in enumerate(entries[name]):
                if kind == "dropout":
                    continue
                w, b, c = p[name][v]
                gw = torch.empty(len(b) if isinstance(w, str) else w.size, dtype=torch.float32, device="cuda")
                gb = torch.empty(len(c) if isinstance(w, str) else len(b), dtype=torch.float32, device="cuda")
                outs += [gw, gb]
                arr[e] = L.DenseGrad(gw.data_ptr(), gb.data_ptr())
            arrays.append(arr)
        keep.extend(arrays)
        return L.ChainBlockGrads(*[C.cast(q, C.POINTER(L.DenseGrad)) for q in arrays])

    def form(train, narrow):
        params, entries = (cp, ent) if train else (cp0, ent0)
        if backward:
            query = (lambda: lib.gnx_chain_block_backward_train_workspace_bytes(g._h, C.byref(params), 1, narrow)) if train else \
                    (lambda: (lib.gnx_chain_block_backward_narrow_workspace_bytes if narrow else lib.gnx_chain_block_backward_workspace_bytes)(g._h, C.byref(params), 1))
        else:
            query = (lambda: lib.gnx_chain_block_forward_train_workspace_bytes(g._h, C.byref(params), 1, narrow)) if train else \
                    (lambda: (lib.gnx_chain_block_forward_narrow_workspace_bytes if narrow else lib.gnx_chain_block_workspace_bytes)(g._h, C.byref(params), 1))
        nb = int(query())
        assert nb > 0, lib.gnx_last_error()
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        if backward:
            dx = [None if t is None else torch.empty_like(t) for t in x]
            gr = grads(entries)
            keep.append(dx)
            if train:
                call = lambda: lib.gnx_chain_block_backward_train(g._h, C.byref(params), C.byref(crec), *map(ptr, x), *map(ptr, gout), 1, *map(ptr, dx), C.byref(gr),
                                                                  ws.data_ptr(), nb, narrow, s)
            else:
                entry = lib.gnx_chain_block_backward_narrow if narrow else lib.gnx_chain_block_backward
                call = lambda: entry(g._h, C.byref(params), *map(ptr, x), *map(ptr, gout), 1, *map(ptr, dx), C.byref(gr), ws.data_ptr(), nb, s)
        else:
            outs = [torch.empty((1, T, d), dtype=torch.float32, device="cuda") if d else None for T, d in zip(rows, outw)]
            keep.append(outs)
            if train:
                call = lambda: lib.gnx_chain_block_forward_train(g._h, C.byref(params), C.byref(crec), *map(ptr, x), 1, *map(ptr, outs), ws.data_ptr(), nb, narrow, 0, s)
            else:
                entry = lib.gnx_chain_block_forward_narrow if narrow else lib.gnx_chain_block_forward
                call = lambda: entry(g._h, C.byref(params), *map(ptr, x), 1, *map(ptr, outs), ws.data_ptr(), nb, 0, s)

        def checked():
            assert call() == 0, lib.gnx_last_error()
        return checked, nb

    forms, wsb = {}, {}
    for key, train, narrow in (("train_narrow", True, 1), ("generic", False, 0), ("narrow", False, 1), ("train_generic", True, 0)):
        forms[key], wsb[key] = form(train, narrow)
    ms = cold_samples(torch, forms, a.samples, warmup=a.warmup)
    f = {k: summary(v) for k, v in ms.items()}
    return dict(direction="backward" if backward else "forward", in_dims=list(cfg[0]), edge=cfg[1], node=cfg[2], graph=cfg[3], dropout_p=0.1,
                dropout_entries={name: len(drops[name]) for name in DR.FN}, E=g.n_edges, N=g.n_nodes, G=g.n_graphs,
                applies=int(lib.gnx_chain_block_train_applies(g._h, C.byref(cp), 1, int(backward))), register_width=buckets(cfg), forms=f, workspace_bytes=wsb,
                train_narrow_over_generic=f["train_narrow"]["median_ms"] / f["generic"]["median_ms"],
                train_narrow_over_narrow=f["train_narrow"]["median_ms"] / f["narrow"]["median_ms"],
                slower_than_generic_beyond_spread=bool(f["train_narrow"]["median_ms"] > f["generic"]["median_ms"] + f["generic"]["spread_ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.chdir(HERE)
    import torch
    import bench
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), box="one MI355X; every form timed in one process, alternating", samples=a.samples,
               method=f"one call per sample between device events, 512 MiB overwritten in front of every sample (cache-cold), forms alternating, {a.warmup} warm-up "
                      "calls each; backward: all gradients wanted; Dropout(0.1) behind every hidden Dense", cases=[])
    graphs = (("512 graphs of 32..256 nodes, 1M edges", lambda: gn.GNGraphBatch.from_csc(*bench.make_hetero(3))),
              ("C2: one graph, 100k nodes, 1M edges", lambda: gn.GNGraphBatch.from_csc(*bench.make_c2())))
    for gname, make in graphs:
        g = make()
        for cfg in CONFIGS:
            for backward in (False, True):
                c = one_case(a, gn, g, cfg, backward)
                c["graph_name"] = gname
                res["cases"].append(c)
                f = c["forms"]
                print(f"{gname} {cfg} {c['direction']}: train_narrow {f['train_narrow']['median_ms']:.4f}  generic {f['generic']['median_ms']:.4f} "
                      f"(spread {f['generic']['spread_ms']:.4f})  narrow {f['narrow']['median_ms']:.4f}  train_generic {f['train_generic']['median_ms']:.4f} ms   "
                      f"applies {c['applies']}  ws {c['workspace_bytes']['train_narrow'] >> 20} / {c['workspace_bytes']['train_generic'] >> 20} MiB  "
                      f"slower {c['slower_than_generic_beyond_spread']}", flush=True)
                res["slower_than_generic_beyond_spread"] = [i for i, q in enumerate(res["cases"]) if q["slower_than_generic_beyond_spread"]]
                if a.out:  # (after every case: a run cut short leaves what it measured)
                    with open(a.out, "w") as fh:
                        json.dump(res, fh, indent=1)
                        fh.write("\n")
        del g


if __name__ == "__main__":
    main()
