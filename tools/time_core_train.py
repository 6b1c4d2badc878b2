"""Times gnx_core_forward_train_typed — a GNCore's training-mode forward with the Dropout mask applied inside one FeedForward kernel per entity
where the core is narrow (csrc/gnx_core_train_narrow.hip) — in fp32 and bf16, against the call it stands in for: gnx_core_forward_train of the
PARENT commit, and for bf16 against torch casts around that parent call (three .float() in front, three .to(bfloat16) behind).  Graph: the
1M-edge Erdős–Rényi graph (BASELINE configs[1], "C2"); widths (10,5,3) README ex.3, (16,16,16) examples/train_sort.py's default, (3,4,5) and
(1,1,1); p = 0.1.

Every sample is ONE whole call between two device events, cache-cold: a 512 MiB buffer is overwritten in front of it (outside the events), so
no call finds its inputs or weights in the L2 / MALL the previous one left.  The forms of a process alternate sample by sample after a warm-up
of 30 calls each (settled clocks, loaded code objects); medians, min / max and the spread (max - min) of the samples are recorded, with the
workspace bytes of every form.
`--parent-root DIR`: a checkout of the parent commit with its library built; its forms are timed there first, in a process of its own (this
script with --root DIR --baseline-only: one library per process), in the same session on the same device.  This build's own time for the
untouched gnx_core_forward_train stands next to the parent's to show the two sessions overlap.  `not_slower_beyond_spread`: typed median <=
parent median + the parent's spread — what a width has to meet to stay in gnx_core_train_fused_applies.

  python tools/time_core_train.py [--samples 41] [--parent-root DIR] [--out profiles/core_train_narrow.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = ((10, 5, 3), (16, 16, 16), (3, 4, 5), (1, 1, 1))
P_DROP = 0.1
FLUSH_BYTES = 512 << 20


def cold_samples(torch, forms, samples, warmup=30):
    """forms: {key: callable}; {key: [ms of each cache-cold call]}, the forms alternating sample by sample"""
    flush = torch.empty(FLUSH_BYTES, dtype=torch.uint8, device="cuda")
    for f in forms.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for i in range(samples):
        for key, f in forms.items():
            flush.fill_(i & 0xFF)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ms[key].append(e0.elapsed_time(e1))
    return ms


def summary(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), spread_ms=float(max(ms) - min(ms)),
                p10_ms=float(np.percentile(ms, 10)), p90_ms=float(np.percentile(ms, 90)), samples=len(ms))


def one_width(a, gn, g, dims, baseline_only):
    import torch
    from oracle import gn_oracle as O
    from tests import util as U
    lib, L = gn._lib.load(), gn._lib
    rng = np.random.default_rng(0)
    core = U.core_from_params(gn, O.make_core_params(rng, dims))
    keep = []
    p = core._c(keep)
    s = torch.cuda.current_stream().cuda_stream
    rows = (g.n_edges, g.n_nodes, g.n_graphs)
    x32 = [torch.from_numpy((rng.random((1, T, d), dtype=np.float32) * 4 - 2)).cuda() for T, d in zip(rows, dims)]
    x16 = [t.to(torch.bfloat16) for t in x32]
    drop = L.Dropout(P_DROP, 0, 12345)
    y32, y16 = [torch.empty_like(t) for t in x32], [torch.empty_like(t) for t in x16]
    nb_t = int(lib.gnx_core_train_workspace_bytes(g._h, C.byref(p), 1))
    ws_t = torch.empty(nb_t, dtype=torch.uint8, device="cuda")

    def train(x=x32):
        assert lib.gnx_core_forward_train(g._h, C.byref(p), C.byref(drop), *(t.data_ptr() for t in x), 1, *(t.data_ptr() for t in y32), ws_t.data_ptr(), nb_t, 0,
                                          s) == 0, lib.gnx_last_error()

    def casts():
        train([t.float() for t in x16])
        return [t.to(torch.bfloat16) for t in y32]

    forms, ws = {"train_f32": train, "train_with_torch_casts_bf16": casts}, {"train_f32": nb_t, "train_with_torch_casts_bf16": nb_t}
    if not baseline_only:
        for key, elem, x, y in (("typed_f32", L.ELEM_F32, x32, y32), ("typed_bf16", L.ELEM_BF16, x16, y16)):
            assert lib.gnx_core_train_fused_applies(g._h, C.byref(p), 1, elem) == 1, (dims, key)
            nb = int(lib.gnx_core_train_typed_workspace_bytes(g._h, C.byref(p), 1, elem, 0))
            w = torch.empty(nb, dtype=torch.uint8, device="cuda")

            def typed(elem=elem, x=x, y=y, w=w, nb=nb):
                assert lib.gnx_core_forward_train_typed(g._h, C.byref(p), elem, C.byref(drop), *(t.data_ptr() for t in x), 1, *(t.data_ptr() for t in y), w.data_ptr(),
                                                        nb, 0, s) == 0, lib.gnx_last_error()

            forms[key], ws[key] = typed, nb
    ms = cold_samples(torch, forms, a.samples)
    rec = dict(dims=list(dims), E=g.n_edges, N=g.n_nodes, G=g.n_graphs, p=P_DROP, forms={k: summary(v) for k, v in ms.items()}, workspace_bytes=ws)
    if not baseline_only:  # the two forms of this build on the same inputs: how far apart the outputs are (the unfused form carries f_fused - f_unfused)
        train()
        ref = [t.clone() for t in y32]
        forms["typed_f32"]()
        torch.cuda.synchronize()
        rec["max_diff_typed_f32_vs_train_over_scale"] = max(float((u.double() - v.double()).abs().max() / max(1.0, float(v.double().abs().max()))) for u, v in zip(y32, ref))
    return rec


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
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", os.path.abspath(a.parent_root), "--baseline-only", "--samples", str(a.samples)],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        parent = {tuple(c["dims"]): c for c in json.loads(r.stdout.strip().splitlines()[-1])["widths"]}
    sys.path.insert(0, a.root)
    os.chdir(a.root)
    import torch
    import bench
    import graphnets_jl_amd as gn
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), box="one MI355X; parent and this build timed in one session, one process each", samples=a.samples,
               method="one call per sample between device events, 512 MiB overwritten in front of every sample (cache-cold), forms alternating, 30 warm-up calls each",
               widths=[])
    c2 = gn.GNGraphBatch.from_csc(*bench.make_c2())
    cut = []
    for dims in WIDTHS:
        c = one_width(a, gn, c2, dims, a.baseline_only)
        res["widths"].append(c)
        if a.baseline_only:
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
        print(line, flush=True)
        if parent:
            res["slower_than_parent_beyond_spread"] = cut
            res["cut_from_gnx_core_train_fused_applies"] = "No width is cut" if not cut else "see the header: include/gnx.h"
        if a.out:  # (after every width: a run cut short leaves what it measured)
            with open(a.out, "w") as fh:
                json.dump(res, fh, indent=1)
                fh.write("\n")
    if a.baseline_only:
        print(json.dumps(res))


if __name__ == "__main__":
    main()
