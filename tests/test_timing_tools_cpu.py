"""tools/timing.py and tools/calls.py are the only places the timing tools measure and build calls from, and the method is the one the committed
records under profiles/ were measured with.  No GPU: the two methods run on a stand-in `torch` whose events return scripted times.

The windows method, as every copy of it read before they became one (W warm-up calls, P probe calls, floor M, window_s seconds):
    per form: W calls; one event pair around P calls; one synchronise; steps = max(M, int(window_s * 1e3 / (probe_ms / P)) + 1)
    then `windows` times, per form in dict order: one event pair around `steps` calls, one synchronise, ms = elapsed / steps
Expected numbers below, at window_s = 0.01 (10 ms) for every triple (W, P, M) in use:
    form "a": the probe takes P * 0.25 ms -> 0.25 ms per call -> int(10 / 0.25) + 1 = 41 calls per window (above every floor: 5, 6, 20, 24, 50)
    form "b": the probe takes P * 4 ms    -> 4 ms per call    -> int(2.5) + 1 = 3, below every floor -> M calls per window
    windows: a takes 41 * 0.5 then 41 * 0.75 ms -> 0.5, 0.75 ms per call; b takes M * 2 then M * 3 ms -> 2.0, 3.0 ms per call
    calls of a: W + P + 2 * 41; calls of b: W + P + 2 * M; synchronises: 2 probes + 4 windows
The cold-samples method (S samples, W warm-up calls): W calls per form, one synchronise; then per sample i and form, in order: the flush buffer
(FLUSH_BYTES of uint8) filled with i & 0xFF, event, ONE call, event, synchronise; ms = elapsed."""
import ast
import glob
import importlib
import json
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import timing  # noqa: E402

TOOLS = sorted(glob.glob(os.path.join(ROOT, "tools", "time_*.py")) + glob.glob(os.path.join(ROOT, "tools", "ab_*.py")))
SHARED = ("tools/timing.py", "tools/calls.py")
# warm-up calls, probe calls, floor on the calls per window: what each tool's records were measured with
TRIPLES = {"time_bw_fused": (10, 20, 20), "time_bw_fused_bf16": (10, 20, 20), "time_bw_narrow": (10, 20, 20), "time_bw_plan": (10, 20, 20),
           "time_chain_plan": (10, 20, 20), "time_bf16_backward": (10, 20, 20), "time_bf16_core": (12, 24, 24), "time_bf16_core_backward": (6, 6, 6),
           "time_core_bw_narrow": (5, 10, 5), "time_bf16_block": (20, 50, 50), "time_bf16_steps": (5, 10, 10)}
COLD = ("time_chain_narrow", "time_chain_bw_narrow", "time_chain_bw_native", "time_chain_bf16", "time_chain_train", "time_core_train")


def _tree(path):
    with open(path) as fh:
        return ast.parse(fh.read())


# ---------------------------------------------------------------- structure
def test_shared_helpers_are_defined_once():
    shared = lambda n: n in ("timed_windows", "cold_samples", "profiled", "profiled_once", "sha", "ptr") or n.startswith("summary")
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tools", "*.py"))):
        rel = os.path.relpath(path, ROOT)
        for node in ast.walk(_tree(path)):
            names = [node.name] if isinstance(node, (ast.FunctionDef, ast.ClassDef)) else \
                [t.id for t in node.targets if isinstance(t, ast.Name)] if isinstance(node, ast.Assign) else []
            for n in filter(shared, names):
                found.setdefault(n, []).append(rel)
    assert found and all(len(v) == 1 and v[0] in SHARED for v in found.values()), found
    assert {"timed_windows", "cold_samples", "summary_windows", "summary_samples", "profiled_once", "sha", "ptr"} <= set(found)


@pytest.mark.parametrize("path", [p for p in TOOLS if os.path.basename(p).startswith("time_")], ids=os.path.basename)
def test_time_tools_hold_no_measuring_or_process_code(path):
    with open(path) as fh:
        text = fh.read()
    for word in ("subprocess", "Event(", "json.dump"):
        assert word not in text, word
    # tool-to-tool imports: only CONFIGS and buckets of tools/time_chain_narrow.py
    for node in ast.walk(_tree(path)):
        if isinstance(node, ast.ImportFrom) and node.module and (node.module.startswith("tools.time_") or node.module.startswith("tools.ab_")):
            assert node.module == "tools.time_chain_narrow" and {a.name for a in node.names} <= {"CONFIGS", "buckets"}, ast.dump(node)
        if isinstance(node, ast.Import):
            assert not any(a.name.startswith(("tools.time_", "tools.ab_")) for a in node.names)


def test_every_tool_imports_without_a_device():
    """in a fresh process: no tool may load torch or the package (and with it the GPU) at import time"""
    names = [os.path.basename(p)[:-3] for p in TOOLS]
    code = ("import importlib, sys\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            f"for n in {names!r}:\n"
            "    importlib.import_module('tools.' + n)\n"
            "assert 'torch' not in sys.modules and 'graphnets_jl_amd' not in sys.modules, sorted(m for m in sys.modules if m.startswith(('torch', 'graphnets')))[:5]\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(names) == 21  # 19 time_*.py and the two ab_*_bits.py


def test_every_named_entry_is_what_the_bindings_table_gives():
    """tools/calls.py's NAMED: each C entry name resolves, through api._entry under the listed switches, to that very entry in either element type
    it takes, with the element code where the entry expects it; narrow = 1 reaches the typed and training Chain entries' `narrow` value"""
    import graphnets_jl_amd as gn
    from tools import calls
    F32, BF16 = gn._lib.ELEM_F32, gn._lib.ELEM_BF16
    fp32_only = ("gnx_block_forward", "gnx_block_backward", "gnx_block_backward_fused", "gnx_chain_block_forward", "gnx_chain_block_forward_narrow",
                 "gnx_chain_block_forward_train", "gnx_chain_block_backward", "gnx_chain_block_backward_narrow", "gnx_chain_block_backward_train",
                 "gnx_core_forward", "gnx_core_forward_train", "gnx_core_backward", "gnx_core_backward_train")
    assert set(calls.TYPED) <= set(calls.NAMED) and not set(calls.TYPED) & set(fp32_only)
    for name in calls.NAMED:
        family = "chain" if "_chain_" in name else "core" if "_core_" in name else "block"
        direction = "backward" if "_backward" in name else "forward"
        record = "_train" in name
        for elem in (F32,) if name in fp32_only else (F32, BF16):
            e = calls.resolve(gn, family, direction, elem, name, record=record)
            assert e.call == name
            codes = [t for t in e.query_tail + e.head if not isinstance(t, str)]
            if name in calls.TYPED or name.endswith(("_narrow", "_train_typed")) and family != "chain":
                assert e.head[0] == elem and e.query_tail[0] == elem, (name, elem, e)
            else:
                assert not codes or family == "chain", (name, e)
    for name, direction in (("gnx_chain_block_forward_typed", "forward"), ("gnx_chain_block_backward_typed", "backward")):
        for elem in (F32, BF16):
            for n in (0, 1):
                e = calls.resolve(gn, "chain", direction, elem, name, narrow=n)
                assert e.call == name and e.query_tail == (elem, n) and e.head == (elem,) and e.tail[0] == n
    for name, direction in (("gnx_chain_block_forward_train", "forward"), ("gnx_chain_block_backward_train", "backward")):
        e = calls.resolve(gn, "chain", direction, F32, name, record=True, narrow=1)
        assert e.call == name and e.query_tail == (1,) and e.head == ("drop",) and e.tail[0] == 1
    assert calls.resolve(gn, "core", "backward", F32, "gnx_core_backward_narrow", record=True).head == (F32, "drop")


# ---------------------------------------------------------------- the method, on a stand-in torch
class FakeTorch:
    """torch.cuda.Event / synchronize and torch.empty().fill_ that log what is done; elapsed_time returns the scripted values in order"""
    uint8 = "uint8"

    def __init__(self, elapsed):
        self.log, self.elapsed, self.allocated = [], list(elapsed), []
        fake = self

        class Event:
            def __init__(self, enable_timing=False):
                assert enable_timing

            def record(self):
                fake.log.append("event")

            def elapsed_time(self, other):
                assert other is not self
                return fake.elapsed.pop(0)

        self.cuda = types.SimpleNamespace(Event=Event, synchronize=lambda: self.log.append("sync"))

    def empty(self, n, dtype=None, device=None):
        self.allocated.append((n, dtype, device))
        return types.SimpleNamespace(fill_=lambda v: self.log.append(("fill", v)))


@pytest.mark.parametrize("triple", sorted(set(TRIPLES.values())))
def test_timed_windows_is_the_parents_method(triple):
    W, P, M = triple
    assert M < 41 or M == 50
    above = 41 if M < 41 else M  # (floor 50: 41 is below it, both forms sit on the floor)
    fake = FakeTorch([P * 0.25, P * 4.0, above * 0.5, M * 2.0, above * 0.75, M * 3.0])
    forms = {k: (lambda k=k: fake.log.append(k)) for k in ("a", "b")}
    ms, steps = timing.timed_windows(fake, forms, 2, 0.01, warmup=W, probe=P, min_calls=M)
    assert steps == {"a": above, "b": M}
    assert ms == {"a": [0.5, 0.75], "b": [2.0, 3.0]}
    assert not fake.elapsed
    expect = []
    for k in ("a", "b"):  # warm-up, then the probe between two events, one synchronise
        expect += [k] * W + ["event"] + [k] * P + ["event", "sync"]
    for _ in range(2):  # the forms alternate window by window, in dict order; one synchronise per window
        for k in ("a", "b"):
            expect += ["event"] + [k] * steps[k] + ["event", "sync"]
    assert fake.log == expect
    assert fake.log.count("a") == W + P + 2 * above and fake.log.count("b") == W + P + 2 * M and fake.log.count("sync") == 6


def test_timed_windows_sizes_a_window_above_the_floor_of_50():
    """the fourth probe: 0.1 ms per call -> int(10 / 0.1) + 1 = 101 calls, above time_bf16_block.py's floor of 50"""
    fake = FakeTorch([50 * 0.1, 101 * 0.5])
    ms, steps = timing.timed_windows(fake, {"a": lambda: None}, 1, 0.01, warmup=20, probe=50, min_calls=50)
    assert steps == {"a": 101} and ms == {"a": [0.5]}


def test_cold_samples_is_the_parents_method():
    fake = FakeTorch([1.5, 2.5, 3.5, 4.5, 5.5, 6.5])
    forms = {k: (lambda k=k: fake.log.append(k)) for k in ("a", "b")}
    ms = timing.cold_samples(fake, forms, 3, warmup=4)
    assert ms == {"a": [1.5, 3.5, 5.5], "b": [2.5, 4.5, 6.5]}
    assert fake.allocated == [(512 << 20, "uint8", "cuda")] and timing.FLUSH_BYTES == 512 << 20
    expect = ["a"] * 4 + ["b"] * 4 + ["sync"]
    for i in range(3):  # per sample and form: flush, event, ONE call, event, synchronise
        for k in ("a", "b"):
            expect += [("fill", i), "event", k, "event", "sync"]
    assert fake.log == expect


def test_cold_samples_flush_value_wraps_at_a_byte():
    fake = FakeTorch([1.0] * 258)
    timing.cold_samples(fake, {"a": lambda: None}, 258, warmup=0)
    assert [v for v in fake.log if isinstance(v, tuple)][-2:] == [("fill", 0), ("fill", 1)]


def test_summaries():
    ms = [1.0, 2.0, 4.0, 3.123456789]
    w = timing.summary_windows(ms)
    assert w.pop("median_ms") == pytest.approx(2.5617283945, rel=1e-12)
    assert w == dict(min_ms=1.0, max_ms=4.0, spread_ms=3.0, window_ms=[1.0, 2.0, 4.0, 3.12346])  # spread_ms always; the windows rounded to 5 places
    s = timing.summary_samples([1.0, 2.0, 4.0, 3.0])
    assert set(s) == {"median_ms", "min_ms", "max_ms", "spread_ms", "p10_ms", "p90_ms", "samples"}
    assert (s["median_ms"], s["min_ms"], s["max_ms"], s["spread_ms"], s["samples"]) == (2.5, 1.0, 4.0, 3.0, 4)
    assert s["p10_ms"] == pytest.approx(1.3) and s["p90_ms"] == pytest.approx(3.7)
    a = types.SimpleNamespace(windows=7, window=0.2)
    assert timing.windows_timing(a, 5, 10, 5) == dict(method="windows", warmup=5, probe=10, min_calls=5, windows=7, window_s=0.2)
    assert timing.cold_timing(15, 30) == dict(method="cold_samples", warmup=30, samples=15, flush_bytes=512 << 20)


@pytest.mark.parametrize("name", sorted(TRIPLES))
def test_each_windows_tool_passes_its_own_triple(name):
    """TIMING is the tool's triple, and every timed_windows / windows_timing call of the tool passes exactly **TIMING"""
    mod = importlib.import_module("tools." + name)
    assert (mod.TIMING["warmup"], mod.TIMING["probe"], mod.TIMING["min_calls"]) == TRIPLES[name] and len(mod.TIMING) == 3
    tree = _tree(os.path.join(ROOT, "tools", name + ".py"))
    assert sum(isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "TIMING" for t in n.targets) for n in ast.walk(tree)) == 1
    calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr in ("timed_windows", "windows_timing")]
    assert {n.func.attr for n in calls} >= {"timed_windows"}
    for n in calls:
        assert [(k.arg, getattr(k.value, "id", None)) for k in n.keywords] == [(None, "TIMING")], ast.dump(n)
    # the record says so too: windows_timing(a, **TIMING), or rounds_record(a, recs, TIMING) for the two --libs tools
    assert any(c.func.attr == "windows_timing" for c in calls) or \
        any(isinstance(n, ast.Call) and getattr(n.func, "attr", "") == "rounds_record" and getattr(n.args[2], "id", "") == "TIMING" for n in ast.walk(tree))


@pytest.mark.parametrize("name", COLD)
def test_each_cold_tool_warms_up_30_calls_and_records_it(name):
    mod = importlib.import_module("tools." + name)
    tree = _tree(os.path.join(ROOT, "tools", name + ".py"))
    src = {getattr(n.func, "attr", ""): n for n in ast.walk(tree) if isinstance(n, ast.Call)}
    assert "cold_samples" in src and "cold_timing" in src
    warm = lambda call, i: ast.unparse(call.args[i])
    assert warm(src["cold_samples"], 3) == warm(src["cold_timing"], 1)  # what is recorded is what is passed
    if warm(src["cold_samples"], 3) == "WARMUP":
        assert mod.WARMUP == 30
    else:  # the flag --warmup, default 30
        assert warm(src["cold_samples"], 3) == "a.warmup"
        default = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, "attr", "") == "add_argument" and n.args and
                   getattr(n.args[0], "value", None) == "--warmup"]
        assert len(default) == 1 and [k.value.value for k in default[0].keywords if k.arg == "default"] == [30]


# ---------------------------------------------------------------- the protocols, on stand-in children
def test_parent_baseline_reads_the_last_line_and_raises_on_failure(tmp_path):
    child = "import sys, json; print('noise'); print('more noise'); print(json.dumps(dict(argv=sys.argv[1:])))"
    rec = timing.parent_baseline(["-c", child], str(tmp_path), ["--samples", 3], 30)
    assert rec == dict(argv=["--root", str(tmp_path), "--baseline-only", "--samples", "3"])
    with pytest.raises(AssertionError, match="the tail of stderr"):
        timing.parent_baseline(["-c", "import sys; sys.stderr.write('x' * 5000 + 'the tail of stderr'); sys.exit(3)"], str(tmp_path), [], 30)


def test_child_root_puts_the_parents_checkout_in_front_of_this_ones_modules(tmp_path, monkeypatch):
    """the child's side of --parent-root: the measuring modules stay this checkout's, everything imported afterwards comes from the root"""
    (tmp_path / "only_in_the_parent_checkout.py").write_text("WHERE = 'parent'\n")
    monkeypatch.setattr(sys, "path", list(sys.path))
    monkeypatch.chdir(ROOT)
    before = sys.modules["tools.timing"]
    timing.child_root(str(tmp_path))
    assert sys.path[0] == str(tmp_path) and os.getcwd() == os.path.realpath(str(tmp_path))
    assert importlib.import_module("only_in_the_parent_checkout").WHERE == "parent"
    assert sys.modules["tools.timing"] is before and os.path.dirname(sys.modules["tools.calls"].__file__) == os.path.join(ROOT, "tools")
    sys.modules.pop("only_in_the_parent_checkout")


CHILD = ("import os, sys, json, time\n"
         "lib = os.environ['GNX_LIB_PATH']\n"
         "open(sys.argv[1], 'a').write(lib + '\\n')\n"
         "mode = sys.argv[2]\n"
         "if lib.endswith('new.so') and mode == 'fail': sys.exit(5)\n"
         "if lib.endswith('new.so') and mode == 'hang': time.sleep(20)\n"
         "print('noise'); print(json.dumps(dict(lib=lib)))\n")


def test_library_rounds_order_and_environment(tmp_path):
    log, libs = tmp_path / "log", (str(tmp_path / "parent.so"), str(tmp_path / "new.so"))
    recs = timing.library_rounds(["-c", CHILD], libs, 2, [log, "ok"], 30)
    assert recs == [("parent", dict(lib=libs[0])), ("new", dict(lib=libs[1]))] * 2
    assert log.read_text().split() == [libs[0], libs[1]] * 2


@pytest.mark.parametrize("mode", ["fail", "hang"])
def test_library_rounds_starts_nothing_after_a_child_that_failed(tmp_path, mode, capsys):
    log, libs = tmp_path / "log", (str(tmp_path / "parent.so"), str(tmp_path / "new.so"))
    with pytest.raises(SystemExit) as e:
        timing.library_rounds(["-c", CHILD], libs, 2, [log, mode], 1 if mode == "hang" else 30)
    assert e.value.code == 2
    assert log.read_text().split() == [libs[0], libs[1]]  # round 1's two children and no more
    assert ("no end within 1 s" if mode == "hang" else "exit status 5") in capsys.readouterr().err


def test_record_writer_leaves_every_case_on_disk(tmp_path):
    path = tmp_path / "rec.json"
    out = timing.RecordWriter(str(path), device="d", cases=[])
    for i in range(3):
        out.add("cases", dict(i=i))
        text = path.read_text()
        assert json.loads(text) == dict(device="d", cases=[dict(i=j) for j in range(i + 1)])
        assert text.endswith("}\n") and text.startswith('{\n "device"')  # indent=1 and a trailing newline
    out.write(lines="cases")  # a record of many short cases: one per line
    assert json.loads(path.read_text()) == out.res and path.read_text().count("\n") == 5
    assert timing.read_record(str(path)) == out.res and timing.read_record(str(tmp_path / "none.json")) == {}
    timing.RecordWriter(None, a=1).write()  # no --out: nothing is written


def test_rounds_record_follows_the_beyond_spread_rule(capsys):
    a = types.SimpleNamespace(rounds=2, windows=2, window=0.2)
    child = lambda ms: dict(device="dev", cases={"c": dict(window_ms=ms, calls_per_window=20)})
    recs = [("parent", child([1.0, 1.2])), ("new", child([1.25, 1.25])), ("parent", child([1.1, 1.1])), ("new", child([1.25, 1.5]))]
    res = timing.rounds_record(a, recs, dict(warmup=10, probe=20, min_calls=20), case="X")
    c = res["cases"][0]
    assert c["parent"]["window_ms"] == [1.0, 1.2, 1.1, 1.1] and c["new"]["median_ms"] == 1.25 and c["parent"]["spread_ms"] == pytest.approx(0.2)
    assert c["not_slower_beyond_spread"] is True and c["calls_per_window"] == dict(parent=20, new=20)  # 1.25 <= 1.1 + 0.2
    slower = timing.rounds_record(a, recs[:1] + [("new", child([1.4, 1.4]))] + recs[2:], dict(warmup=10, probe=20, min_calls=20))
    assert slower["cases"][0]["not_slower_beyond_spread"] is False  # median of 1.4, 1.4, 1.25, 1.5 = 1.4 > 1.3
    assert res["order"] == "parent, new, parent, new: one process each" and res["windows_per_library"] == 4 and res["case"] == "X"
    assert res["timing"] == dict(method="windows", warmup=10, probe=20, min_calls=20, windows=2, window_s=0.2)
    assert "not_slower_beyond_spread True" in capsys.readouterr().out
