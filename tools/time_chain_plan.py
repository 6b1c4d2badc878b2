"""Did a change of the Chain block's HOST code move the time of a whole call?  Times three calls on tests/chain_bw_cases.py's N-w16-32 (131 graphs,
1031 nodes, 4099 edges: almost pure host and launch time) against another build of libgnx.so (the parent commit's), never against another form of
the code under test:

  a  gnx_chain_block_forward_narrow, fp32: three kernels
  b  gnx_chain_block_backward_narrow, fp32: the recompute, three pullback kernels and their finishers
  c  gnx_chain_block_forward_typed, bf16, narrow = 1: the native path

  python tools/time_chain_plan.py --libs graphnets.jl_amd/libgnx_parent.so graphnets.jl_amd/libgnx.so [--rounds 2] [--windows 4] [--out profiles/chain_plan_ab.json]

One child process per library and round (GNX_LIB_PATH), each under its own time limit, in the order parent, new, parent, new; a child that fails
ends the run (tools/timing.py: library_rounds).  Windows as tools/timing.py: timed_windows; rounds x windows >= 7 per library.
`not_slower_beyond_spread` (as tools/time_bw_plan.py): new median <= parent median + the parent's spread (max - min over its windows).
`--run` is the child.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import calls, timing  # noqa: E402

CASE = "N-w16-32"
TIMING = dict(warmup=10, probe=20, min_calls=20)


def chain_calls(gn, g, d):
    """{name: Call} of the three calls on case d = dict(p, x, cot, R) of tests/chain_bw_cases.py"""
    import numpy as np
    import torch
    from tests import test_gpu_memory_contract as MC
    L = gn._lib
    keep = []
    to = lambda v, dt: None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda().to(dt)
    x, cot = [to(v, torch.float32) for v in d["x"]], [to(v, torch.float32) for v in d["cot"]]
    case = calls.given_case(g, calls.chain_params(gn, d["p"], keep), keep, x, cot, MC._chain_out_widths(d["p"]), R=d["R"], oracle=d["p"])
    assert calls.applies(gn, case, "gnx_chain_block_forward_narrow_applies") == 7 and calls.applies(gn, case, "gnx_chain_block_backward_narrow_applies") == 7
    assert calls.applies(gn, case, "gnx_chain_block_forward_typed_applies", L.ELEM_BF16, 1) == 1
    return {"a gnx_chain_block_forward_narrow fp32": calls.build(gn, case, "chain", "forward", L.ELEM_F32, "gnx_chain_block_forward_narrow"),
            "b gnx_chain_block_backward_narrow fp32": calls.build(gn, case, "chain", "backward", L.ELEM_F32, "gnx_chain_block_backward_narrow"),
            "c gnx_chain_block_forward_typed bf16 native": calls.build(gn, case, "chain", "forward", L.ELEM_BF16, {"bf16_chain", "narrow_chain"},
                                                                      x=[to(v, torch.bfloat16) for v in d["x"]])}


def run(a, limit=None):
    """the child's record; limit: the first cases only (tests/test_gpu_timing_tools.py)"""
    import torch
    import graphnets_jl_amd as gn
    from tests import chain_bw_cases as CC
    from tests import test_gpu_memory_contract as MC
    torch.cuda.set_device(0)
    g = MC._from_csc(gn, list(CC.batch_parts()))[0]
    res = {}
    for name, call in list(chain_calls(gn, g, CC.data(CASE)).items())[:limit]:
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
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.run:
        return timing.print_record(run(a))
    assert a.rounds * a.windows >= 7
    recs = timing.library_rounds(__file__, a.libs, a.rounds, ["--run", "--windows", a.windows, "--window", a.window], a.timeout, cwd=ROOT)
    res = timing.rounds_record(a, recs, TIMING, case=CASE)
    timing.RecordWriter(a.out, **res).write(lines="cases")
    sys.exit(0 if all(c["not_slower_beyond_spread"] for c in res["cases"]) else 1)


if __name__ == "__main__":
    main()
