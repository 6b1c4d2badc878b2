"""Did a change of the backward's HOST code move the time of a whole call?  Times three calls against another build of libgnx.so (the parent
commit's), never against another form of the code under test:

  a  gnx_block_backward_narrow, bf16, (3,2,4)=>(3,4,5) on the 1M-edge graph (BASELINE configs[1], "C2"): the run-time wave kernel
  b  gnx_core_backward_narrow, fp32, (10,5,3) on C2
  c  gnx_block_backward_narrow, fp32, (10,5,0)=>(3,4,5) on tests/test_gpu_bw_fused.py's small40: 40 graphs of at most 40 nodes — the call is
     a dozen launches of almost no work each, so its time is the host's

  python tools/time_bw_plan.py --libs graphnets.jl_amd/libgnx_parent.so graphnets.jl_amd/libgnx.so [--rounds 2] [--windows 4] [--out profiles/bw_plan_ab.json]

One child process per library and round (GNX_LIB_PATH), each under its own time limit, in the order parent, new, parent, new; a child that fails
ends the run (tools/timing.py: library_rounds).  Windows as tools/timing.py: timed_windows; rounds x windows >= 7 per library.
`not_slower_beyond_spread` (as tools/time_bw_narrow.py): new median <= parent median + the parent's spread (max - min over its windows).
`--run` is the child.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import calls, timing  # noqa: E402

TIMING = dict(warmup=10, probe=20, min_calls=20)
# (name, graph, family, widths, bf16)
CASES = (("a block narrow bf16 (3,2,4)=>(3,4,5) C2", "C2", "block", ((3, 2, 4), (3, 4, 5)), True),
         ("b core narrow fp32 (10,5,3) C2", "C2", "core", (10, 5, 3), False),
         ("c block narrow fp32 (10,5,0)=>(3,4,5) small40", "small40", "block", ((10, 5, 0), (3, 4, 5)), False))


def narrow_call(gn, g, family, widths, bf16):
    """the narrow pullback of the family on g, every gradient wanted"""
    L = gn._lib
    elem = L.ELEM_BF16 if bf16 else L.ELEM_F32
    if family == "core":
        case = calls.core_case(gn, g, widths)
        assert calls.applies(gn, case, "gnx_core_backward_narrow_applies", elem) == 1
        return calls.build(gn, case, "core", "backward", elem, "gnx_core_backward_narrow")
    case = calls.block_case(gn, g, *widths, act=(1, 2, 0), dtype=calls.elem_dtype(gn, elem))
    fw = calls.build(gn, case, "block", "forward", elem, "gnx_block_forward_typed")
    fw.f()
    assert calls.applies(gn, case, "gnx_block_backward_narrow_applies", elem) == 1
    return calls.build(gn, case, "block", "backward", elem, "gnx_block_backward_narrow", fwd=fw.outs)


def run(a, graphs=None, limit=None):
    """the child's record; graphs: {key: GNGraphBatch} in place of C2, limit: the first cases only (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    from tests.test_gpu_bw_fused import _graph
    torch.cuda.set_device(0)
    built = {key: _graph(gn, key) if key == "small40" else timing.graph(gn, key, graphs) for key in dict.fromkeys(c[1] for c in CASES[:limit])}  # each once
    made = {name: narrow_call(gn, built[key], family, widths, bf16) for name, key, family, widths, bf16 in CASES[:limit]}
    res = {}
    for name, call in made.items():
        ms, steps = timing.timed_windows(torch, {"call": call.f}, a.windows, a.window, **TIMING)
        res[name] = dict(window_ms=ms["call"], calls_per_window=steps["call"])
    return dict(device=torch.cuda.get_device_name(0), cases=res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true", help="the child: the windows of the library this process loads")
    ap.add_argument("--libs", nargs=2, metavar=("PARENT", "NEW"))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--windows", type=int, default=4, help="windows per child")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of device time per window")
    ap.add_argument("--timeout", type=int, default=200, help="seconds per child")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.run:
        return timing.print_record(run(a))
    assert a.rounds * a.windows >= 7
    recs = timing.library_rounds(__file__, a.libs, a.rounds, ["--run", "--windows", a.windows, "--window", a.window], a.timeout, cwd=ROOT)
    res = timing.rounds_record(a, recs, TIMING)
    timing.RecordWriter(a.out, **res).write()
    sys.exit(0 if all(c["not_slower_beyond_spread"] for c in res["cases"]) else 1)


if __name__ == "__main__":
    main()
