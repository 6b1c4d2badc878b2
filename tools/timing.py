"""The one place the tools/time_*.py and tools/ab_*_bits.py measure from.  Two methods, each written once:

  windows        timed_windows: per form `warmup` calls, then `probe` calls between two device events that size a window (>= window_s of device
                 time, at least min_calls calls); then `windows` rounds in which the forms alternate window by window, one event pair and one
                 synchronise per window; ms per call = elapsed / calls.  summary_windows.
  cold_samples   per form `warmup` calls; then `samples` rounds in which the forms alternate sample by sample: FLUSH_BYTES overwritten in front of
                 every sample (outside the events), ONE call between two device events, one synchronise.  summary_samples.

warmup / probe / min_calls differ between the tools (each tool's TIMING constant says which it uses: the committed records under profiles/ were
measured with them) and go into every record under "timing".  Around them: one profiled call per form (profiled_once), the record that is
rewritten after every case (RecordWriter), the two A/B protocols between builds (parent_baseline with child_root for the child's side;
library_rounds), the two full-size graphs of bench.py, and sha / ptr.

This file imports nothing of the package at module level: a --baseline-only child loads it from ITS OWN checkout and then puts the parent's
checkout in front of sys.path (child_root)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

FLUSH_BYTES = 512 << 20
# the two full-size graphs: key -> (the name the records carry, bench.py's maker)
GRAPHS = {"C2": ("C2: one graph, 100k nodes, 1M edges", lambda bench: bench.make_c2()),
          "hetero512": ("512 graphs of 32..256 nodes, 1M edges", lambda bench: bench.make_hetero(3))}


def timed_windows(torch, forms, windows, window_s, warmup, probe, min_calls):
    """forms: {key: callable}; returns {key: [ms per call of each window]} and the calls per window"""
    steps, ms = {}, {k: [] for k in forms}
    for key, f in forms.items():
        for _ in range(warmup):
            f()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(probe):
            f()
        e1.record()
        torch.cuda.synchronize()
        steps[key] = max(min_calls, int(window_s * 1e3 / (e0.elapsed_time(e1) / probe)) + 1)
    for _ in range(windows):
        for key, f in forms.items():  # alternate the forms window by window
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps[key]):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms[key].append(e0.elapsed_time(e1) / steps[key])
    return ms, steps


def cold_samples(torch, forms, samples, warmup):
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


def windows_timing(a, warmup, probe, min_calls):
    """the "timing" entry of a record measured with timed_windows(..., a.windows, a.window, warmup, probe, min_calls)"""
    return dict(method="windows", warmup=warmup, probe=probe, min_calls=min_calls, windows=a.windows, window_s=a.window)


def cold_timing(samples, warmup):
    """the "timing" entry of a record measured with cold_samples(..., samples, warmup)"""
    return dict(method="cold_samples", warmup=warmup, samples=samples, flush_bytes=FLUSH_BYTES)


def summary_windows(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), spread_ms=float(max(ms) - min(ms)),
                window_ms=[round(x, 5) for x in ms])


def summary_samples(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), spread_ms=float(max(ms) - min(ms)),
                p10_ms=float(np.percentile(ms, 10)), p90_ms=float(np.percentile(ms, 90)), samples=len(ms))


def profiled(gn, torch, f, calls):
    """what the library's per-kernel profiler (gnx_profile_*) read over `calls` calls of f, sorted by scope; switched off again whatever f does"""
    gn.profile_reset()
    gn.profile_enable(True)
    try:
        for _ in range(calls):
            f()
        torch.cuda.synchronize()
    finally:
        gn.profile_enable(False)
    out = dict(sorted(gn.profile_read().items()))
    gn.profile_reset()
    return out


def profiled_once(gn, torch, f):
    """{scope: {kernels, total_ms}} of ONE call of f under the profiler"""
    return {n: dict(kernels=v["kernels"], total_ms=round(v["total_ms"], 5)) for n, v in profiled(gn, torch, f, 1).items()}


class RecordWriter:
    """The result dict of a tool and its --out file: write() after every case, so that a run cut short leaves what it measured."""

    def __init__(self, path, **head):
        self.path, self.res = path, dict(head)

    def write(self, lines=None):
        """lines: the key of a list that is written one element per line (a record of many short cases) in place of indent=1"""
        if not self.path:
            return
        with open(self.path, "w") as fh:
            if lines is None:
                json.dump(self.res, fh, indent=1)
                fh.write("\n")
            else:
                head = {k: v for k, v in self.res.items() if k != lines}
                fh.write(json.dumps(head)[:-1] + f', "{lines}": [\n' + ",\n".join(json.dumps(c) for c in self.res[lines]) + "\n]}\n")

    def add(self, key, case):
        self.res.setdefault(key, []).append(case)
        self.write()


def print_record(res):
    """the record as ONE line of JSON on stdout: what a parent process reads (last_json_line)"""
    print(json.dumps(res), flush=True)


def read_record(path):
    """the record a previous run left in `path`, {} where there is none"""
    if not path or not os.path.exists(path):
        return {}
    with open(path) as fh:
        return json.load(fh)


def last_json_line(text):
    return json.loads(text.strip().splitlines()[-1])


def parent_baseline(script, parent_root, argv, timeout):
    """The --parent-root protocol: `script` (a file of THIS checkout, or ["-c", code]) runs first and in a process of its own — one library per
    process — with --root PARENT --baseline-only and `argv`; the last line of its stdout is its record."""
    head = list(script) if isinstance(script, (list, tuple)) else [os.path.abspath(script)]
    r = subprocess.run([sys.executable, *head, "--root", os.path.abspath(parent_root), "--baseline-only", *map(str, argv)], capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return last_json_line(r.stdout)


def against_parent(c, pc, i, cut):
    """Case c (index i) of a Chain tool against the parent's record pc of the same case: c gains `parent`, `narrow_over_parent` and
    `not_slower_beyond_spread` (narrow median <= the parent's chain median + the spread of its samples); i joins `cut` where that is False.
    Returns what the case's printed line says about it."""
    assert pc["graph_name"] == c["graph_name"] and pc["in_dims"] == c["in_dims"] and pc["edge"] == c["edge"]
    base, narrow = pc["forms"]["chain"], c["forms"]["narrow"]
    c["parent"] = dict(forms=pc["forms"], workspace_bytes=pc["workspace_bytes"])
    c["narrow_over_parent"] = narrow["median_ms"] / base["median_ms"]
    c["not_slower_beyond_spread"] = bool(narrow["median_ms"] <= base["median_ms"] + base["spread_ms"])
    if not c["not_slower_beyond_spread"]:
        cut.append(i)
    return f"   parent {base['median_ms']:.4f} (spread {base['spread_ms']:.4f})   narrow / parent {c['narrow_over_parent']:.3f}"


def child_root(root):
    """The child's side of parent_baseline, and what every such tool does before it imports the package: the checkout `root` goes in front of
    sys.path and becomes the working directory, AFTER this module (and tools.calls) came from the script's own checkout — sys.modules keeps them,
    `bench`, `graphnets_jl_amd`, `oracle` and `tests` are then found in `root`."""
    from tools import calls  # noqa: F401  (this checkout's, before `root` shadows the tools package)
    sys.path.insert(0, root)
    os.chdir(root)


def library_rounds(script, libs, rounds, argv, timeout, cwd=None):
    """The GNX_LIB_PATH protocol: one child of `script` per library and round, strictly one after another in the order parent, new, parent, new,
    each under its own time limit.  Returns [(key, record)] in that order.  A child that does not end in time or exits non-zero ends the run
    with status 2: nothing further is started."""
    head = list(script) if isinstance(script, (list, tuple)) else [os.path.abspath(script)]
    recs = []
    for _ in range(rounds):
        for key, lib in zip(("parent", "new"), libs):
            env = dict(os.environ)
            env.pop("GNX_LIB_PATH", None)
            if lib:  # (None: the library of this checkout)
                env["GNX_LIB_PATH"] = os.path.abspath(lib)
            try:
                r = subprocess.run([sys.executable, *head, *map(str, argv)], env=env, capture_output=True, text=True, timeout=timeout, cwd=cwd)
            except subprocess.TimeoutExpired:
                print(f"{lib or 'this build'} ({key}): no end within {timeout} s", file=sys.stderr)
                sys.exit(2)
            if r.returncode != 0:
                print(f"{lib or 'this build'} ({key}): exit status {r.returncode}\n{r.stderr[-4000:]}", file=sys.stderr)
                sys.exit(2)  # (a child that failed: nothing further is started)
            recs.append((key, last_json_line(r.stdout)))
    return recs


def rounds_record(a, recs, triple, **head):
    """The record of library_rounds' [(key, child record)] where a child record is {device, cases: {name: {window_ms, calls_per_window}}}: per
    case the windows of each library over all rounds, summarised, and `not_slower_beyond_spread`: new median <= parent median + the parent's
    spread.  One line per case is printed.  a: the tool's arguments (rounds, windows, window); triple: its warmup / probe / min_calls."""
    windows, steps = {"parent": {}, "new": {}}, {}
    for key, rec in recs:
        for name, c in rec["cases"].items():
            windows[key].setdefault(name, []).extend(c["window_ms"])
            steps.setdefault(name, {})[key] = c["calls_per_window"]
    res = dict(device=recs[-1][1]["device"], **head, order="parent, new" + ", parent, new" * (a.rounds - 1) + ": one process each",
               windows_per_library=a.rounds * a.windows, window_s=a.window, timing=windows_timing(a, **triple), cases=[])
    for name in windows["parent"]:
        par, new = summary_windows(windows["parent"][name]), summary_windows(windows["new"][name])
        c = dict(case=name, calls_per_window=steps[name], parent=par, new=new, new_over_parent=new["median_ms"] / par["median_ms"],
                 not_slower_beyond_spread=bool(new["median_ms"] <= par["median_ms"] + par["spread_ms"]))
        res["cases"].append(c)
        print(f"{name}: parent {par['median_ms']:.4f} ms (spread {par['spread_ms']:.4f})   new {new['median_ms']:.4f} ms (spread {new['spread_ms']:.4f})   "
              f"ratio {c['new_over_parent']:.3f}   not_slower_beyond_spread {c['not_slower_beyond_spread']}", flush=True)
    return res


def graph(gn, key, graphs=None):
    """the GNGraphBatch of GRAPHS[key]; `graphs`: {key: GNGraphBatch} that stand in for the full-size ones (the tests' small batches)"""
    if graphs is not None:
        return graphs[key]
    import bench
    return gn.GNGraphBatch.from_csc(*GRAPHS[key][1](bench))


def er_1m(gn):
    """the graph of the bf16 tools' records: tests/util.py's Erdős–Rényi recipe with seed 0, 100k nodes, 1M edges, one graph (not bench.py's C2 draw)"""
    from tests import util as U
    colptr, rowval = U.er_csc(np.random.default_rng(0), 100_000, 1_000_000)
    return gn.GNGraphBatch.from_csc([colptr], [rowval], [100_000])


def pack512(gn):
    """512 graphs of 32..256 nodes with ~3 in-edges per node: every graph <= 8 wave tiles, so the batch takes the one-launch pack form"""
    from tests import util as U
    rng = np.random.default_rng(1)
    cps, rvs, ns = [], [], []
    for n in rng.integers(32, 257, 512):
        cp, rv = U.er_csc(rng, int(n), int(3 * n))
        cps.append(cp); rvs.append(rv); ns.append(int(n))
    return gn.GNGraphBatch.from_csc(cps, rvs, ns)


class OneGraph:
    """get = OneGraph(gn, graphs); get(key) is graph(gn, key, graphs), with at most one full-size batch alive at a time"""

    def __init__(self, gn, graphs=None):
        self.gn, self.graphs, self.key, self.g = gn, graphs, None, None

    def __call__(self, key):
        if key != self.key:
            self.g = None  # (released before the next one is built)
            self.key, self.g = key, graph(self.gn, key, self.graphs)
        return self.g


def sha(t):
    import torch
    return None if t is None else hashlib.sha256(t.detach().contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()
