"""Every timing tool still runs, and writes the record it wrote before its measuring code moved to tools/timing.py and its call plumbing to
tools/calls.py.  In process, on the smallest counts (one window of 0.01 s; two samples after one warm-up call), the first case of each tool, and
small graphs in place of the 1M-edge ones: tests/test_gpu_bw_fused.py's `degrees` (one graph, 260 nodes: every _applies a tool asserts is 1
there — the five ahead-of-time width sets and the run-time set (3,2,4)=>3 need E > 0, wave tiles and narrow widths, the core rules only widths
within 1..16: include/gnx.h) for C2 and its `small40` (40 graphs) for the 512-graph batch.

Per tool: every C call returned 0 (the closures of tools/calls.py assert it), the record is JSON, every key path of a case of the tool's
committed record under profiles/ exists in the produced case, and the bit-identity fields hold as they do in the committed records.  Below
`profiler_one_call.<form>` the keys are the profiler's scope names, which follow the kernels a graph size takes: there the produced scopes
must carry the fields of the committed ones.  Fields that exist only with --parent-root / --parent-lib are exempt (PARENT_ONLY); `timing`, and
`spread_ms` where a record lacked it, are the only additions.
profiles/bf16_core_backward.json and profiles/bf16_core_c4narrow.json hold no tool output ("not measured"): their tools run, nothing is compared.
The first use of the run-time width set (3,2,4)=>3 compiles its kernel once (tools/time_bw_narrow.py, tools/time_bw_plan.py)."""
import importlib
import json
import os
import types

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_ONLY = {"time_chain_narrow": ("parent", "narrow_over_parent", "not_slower_beyond_spread"),
               "time_chain_bw_narrow": ("parent", "narrow_over_parent", "not_slower_beyond_spread"),
               "time_core_bw_narrow": ("parent_gnx_core_backward", "narrow_over_parent", "not_slower_beyond_spread"),
               "time_core_train": ("parent", "typed_f32_over_parent_train", "typed_bf16_over_parent_train", "typed_bf16_over_parent_train_with_casts",
                                   "not_slower_beyond_spread"),
               "time_bf16_backward": ("fp32_parent_vs_this_build",)}
OPEN = ("profiler_one_call",)  # {form: {profiler scope: fields}}
ARGS = dict(windows=1, window=0.01, samples=2, warmup=1, out=None, baseline_only=False, fp32_only=False, accuracy_log=None, sets=2, repeats=1, steps=20,
            graph=False, only="c2", rounds=1)


@pytest.fixture(scope="module")
def gn():
    import torch
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


@pytest.fixture(scope="module")
def graphs(gn):
    from tests.test_gpu_bw_fused import _graph
    return {"C2": _graph(gn, "degrees"), "hetero512": _graph(gn, "small40")}


def _committed(name):
    with open(os.path.join(ROOT, "profiles", name)) as fh:
        return json.load(fh)


def _paths(x, prefix=()):
    """the key paths of a case; a list of dicts stands for its first element; below OPEN.<form> the keys are data"""
    if isinstance(x, dict) and x and not (len(prefix) >= 2 and prefix[-2] in OPEN):
        for k, v in x.items():
            yield from _paths(v, prefix + (k,))
    elif isinstance(x, list) and x and isinstance(x[0], dict):
        yield from _paths(x[0], prefix + (0,))
    else:
        yield prefix


def _at(x, path):
    for k in path:
        x = x[k]
    return x


def _same_shape(tool, committed, produced):
    json.loads(json.dumps(produced))
    missing = []
    for path in _paths(committed):
        if path[0] in PARENT_ONLY.get(tool, ()):
            continue
        try:
            got = _at(produced, path)
        except (KeyError, IndexError, TypeError):
            missing.append(path)
            continue
        if len(path) >= 2 and path[-2] in OPEN:  # the profiler's scopes: the fields of one scope
            fields = set(next(iter(_at(committed, path).values())))
            assert got and all(set(v) == fields for v in got.values()), (path, got)
    assert not missing, missing


def _is_timing(rec, method):
    assert rec["timing"]["method"] == method, rec["timing"]
    want = ("warmup", "probe", "min_calls", "windows", "window_s") if method == "windows" else ("warmup", "samples", "flush_bytes")
    assert set(rec["timing"]) == {"method", *want}


# (tool, committed record, where its first case is, how the tool is run for its first case, the produced case, method, fields that must be True)
def _first(key):
    return lambda r: r[key][0]


TOOLS = [
    ("time_bw_fused", "bw_fused_c2.json", _first("cases"), lambda m, a, g: m.run(a, graphs=g, limit=1), _first("cases"), "windows",
     ("input_and_node_graph_gradients_bit_identical",)),
    ("time_bw_fused_bf16", "bw_fused_bf16_c2.json", _first("cases"), lambda m, a, g: m.run(a, graphs=g, limit=1), _first("cases"), "windows",
     ("input_and_node_graph_gradients_bits_of_typed", "edge_gradients_bits_of_fused_fp32_on_widened", "input_gradients_are_rounded_fused_fp32_on_widened")),
    ("time_bw_narrow", "bw_narrow_c2.json", _first("cases"), lambda m, a, g: m.run(a, graphs=g, limit=1), _first("cases"), "windows",
     ("input_and_node_graph_gradients_bit_identical",)),
    ("time_core_bw_narrow", "core_bw_narrow.json", _first("cases"), lambda m, a, g: m.run(a, graphs=g, limit=1), _first("cases"), "windows", ()),
    ("time_core_train", "core_train_narrow.json", _first("widths"), lambda m, a, g: m.run(a, graphs=g, limit=1), _first("widths"), "cold_samples", ()),
    ("time_chain_narrow", "chain_narrow.json", _first("cases"), lambda m, a, g: m.run(a, graphs=g, limit=1), _first("cases"), "cold_samples", ()),
    ("time_chain_bw_narrow", "chain_bw_narrow.json", _first("cases"), lambda m, a, g: m.run(a, graphs=g, limit=1), _first("cases"), "cold_samples", ()),
    ("time_chain_bw_native", "chain_bw_native.json", _first("cases"), lambda m, a, g: m.run(a, graphs=g, limit=1), _first("cases"), "cold_samples",
     ("native_bits_equal_staged",)),
    ("time_chain_bf16", "chain_bf16.json", _first("cases"), lambda m, a, g: m.run(a, graphs=g, limit=1), _first("cases"), "cold_samples",
     ("typed_bits_equal_torch_cast",)),
    ("time_chain_train", "chain_train_narrow.json", _first("cases"), lambda m, a, g: m.run(a, graphs=g, limit=1), _first("cases"), "cold_samples", ()),
    ("time_bf16_backward", "bf16_backward_c2.json", lambda r: r["timing_tool"], lambda m, a, g: m.run(a, False, g=g["C2"]), lambda r: r, "windows",
     ("c_bit_identical_to_b",)),
    ("time_bf16_block", "bf16_block_c2.json", lambda r: r["timing_tool"]["results"][0], lambda m, a, g: m.run(a, graphs=[g["C2"], g["hetero512"]]),
     _first("results"), "windows", ("bit_identical",)),
    ("time_bf16_steps", "bf16_steps_c2.json", lambda r: r["timing_tool"]["results"][0], lambda m, a, g: m.run(a, graphs=[g["C2"]]), _first("results"),
     "windows", ("bf16_steps_bit_identical_to_separate_calls",)),
    ("time_bf16_core", None, None, lambda m, a, g: m.run(a, g=g["C2"]), lambda r: r, "windows", ("i_bit_identical_to_ii",)),
    ("time_bf16_core_backward", None, None, lambda m, a, g: m.run(a, g=g["C2"], widths=m.WIDTHS[:1]), lambda r: r, "windows", ()),
]


@pytest.mark.parametrize("tool, record, committed_case, run, produced_case, method, true_fields", TOOLS, ids=[t[0] for t in TOOLS])
def test_tool_runs_and_writes_its_record(gn, graphs, tmp_path, tool, record, committed_case, run, produced_case, method, true_fields):
    mod = importlib.import_module("tools." + tool)
    a = types.SimpleNamespace(**dict(ARGS, out=str(tmp_path / "rec.json") if tool == "time_chain_narrow" else None))
    res = run(mod, a, graphs)
    _is_timing(res, method)
    case = produced_case(res)
    if record is not None:
        _same_shape(tool, committed_case(_committed(record)), case)
    else:
        json.loads(json.dumps(res))
    for f in true_fields:
        assert case[f] is True, (f, case[f])
    if tool == "time_bf16_core_backward":
        assert all(w["i_bit_identical_to_ii"] is True for w in res["widths"].values())
    if a.out:  # the record on disk after the case is the record returned
        with open(a.out) as fh:
            assert json.load(fh) == json.loads(json.dumps(res))
    if method == "windows" and "forms" in case:  # the window form always carries spread_ms
        assert all("spread_ms" in f for f in case["forms"].values())


def test_chain_train_backward_case(gn, graphs):
    """tools/time_chain_train.py's second case is the pullback: the training entries with a Dropout record, narrow 1 and 0, and gradient slots laid
    out behind an entry list with Dropout slots"""
    mod = importlib.import_module("tools.time_chain_train")
    res = mod.run(types.SimpleNamespace(**ARGS), graphs=graphs, limit=2)
    assert [c["direction"] for c in res["cases"]] == ["forward", "backward"]
    committed = next(c for c in _committed("chain_train_narrow.json")["cases"] if c["direction"] == "backward")
    _same_shape("time_chain_train", committed, res["cases"][1])
    assert res["cases"][1]["dropout_entries"] == committed["dropout_entries"] and all(v > 0 for v in res["cases"][1]["workspace_bytes"].values())


PLAN = [("time_bw_plan", "bw_plan_ab.json", lambda m, a, g: m.run(a, graphs=g, limit=1)), ("time_chain_plan", "chain_plan_ab.json", lambda m, a, g: m.run(a, limit=1))]


@pytest.mark.parametrize("tool, record, run", PLAN, ids=[t[0] for t in PLAN])
def test_libs_tool_child_side(gn, graphs, tool, record, run):
    """the --run side alone; its record goes through tools/timing.py's rounds_record as both libraries to take the committed record's shape"""
    from tools import timing
    mod = importlib.import_module("tools." + tool)
    a = types.SimpleNamespace(**ARGS)
    child = json.loads(json.dumps(run(mod, a, graphs)))
    committed = _committed(record)
    assert list(child["cases"]) == [committed["cases"][0]["case"]]
    res = timing.rounds_record(a, [("parent", child), ("new", child)], mod.TIMING)
    _is_timing(res, "windows")
    _same_shape(tool, committed["cases"][0], res["cases"][0])
    assert {k for k in committed if k not in ("note", "earlier_runs_summary", "earlier_run_that_missed", "case")} <= set(res)


def test_bits_tools_child_side(gn):
    """tools/ab_backward_bits.py and tools/ab_chain_bits.py: the first case of each through the shared call builders, in the committed records' structure"""
    ab = importlib.import_module("tools.ab_backward_bits")
    rec = json.loads(json.dumps(ab.run(limit=1, core_limit=6)))  # the six core cases on small40: every core entry, with and without a Dropout record
    committed = _committed("bw_plan_bits.json")["cases"]
    assert len(rec) == 2 + 6 and set(rec) <= set(committed)
    assert {e for label, entries in rec.items() if label.startswith("core") for e in entries} == \
        {"gnx_core_backward", "gnx_core_backward_train", "gnx_core_backward_typed", "gnx_core_backward_narrow"}
    for label, entries in rec.items():
        assert set(entries) == set(committed[label])
        for e, v in entries.items():
            assert set(v) == set(committed[label][e]) and set(v["sha256"]) == set(committed[label][e]["sha256"]), (label, e)
            assert {n for n, h in v["sha256"].items() if h is None} == {n for n, h in committed[label][e]["sha256"].items() if h is None}
            assert v["workspace_bytes"] >= 0 and all(h is None or len(h) == 64 for h in v["sha256"].values()), (label, e)
            if "applies" in v:
                assert (v["applies"] is None) == (committed[label][e]["applies"] is None), (label, e)
    ac = importlib.import_module("tools.ab_chain_bits")
    rec = json.loads(json.dumps(ac.run(limit=1)))
    committed = _committed("chain_plan_bits.json")["calls"]
    (cid, entries), = rec.items()
    assert {f"{cid} / {e}" for e in entries} == {k for k in committed if k.startswith(cid + " / ")}
    for e, v in entries.items():
        c = committed[f"{cid} / {e}"]
        assert set(c) == {"applies", "workspace_bytes", "rc", "tensors", "sha256"}
        assert (v["rc"], sum(h is not None for h in v["sha256"].values())) == (c["rc"], c["tensors"]) and v["workspace_bytes"] >= 0, e
