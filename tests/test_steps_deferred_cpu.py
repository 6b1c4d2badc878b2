"""Carrying runs of gnx_block_forward_steps (graphnets.jl_amd/csrc/gnx_step_hazard.h: run_defers, run_place), compiled on their own with g++:
the operations the library's planner (StepsPlanner, what gnx_forward.hip's steps_schedule issues) returns for two streams with runs whose
block launch carries the graph updates of the run before it, simulated (tests/c/steps_plan_sim.h) as a happens-before relation over ACTIVITIES — a step's edge + node update, and its graph update wherever that ends up (behind its
own block launch, at the front of the next one-step launch on its stream, at the front of the next run's block launch, or in a flush) — with
the two partial-row areas of a workspace as separate byte ranges.  Every two activities whose bytes conflict must be ordered.  The rotation
over eight buffer sets carries at every run boundary, feedback never carries, and with ONE partial-row area the same simulation reports the
race.  And the resource limits of the carrying kernels (k_block_wave_carry), from the compiler's resource remarks for gfx950."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphnets.jl_amd", "csrc")

SCHEDULE = r"""
#include "steps_plan_sim.h"
using namespace sim;
// defer: runs may carry (else: every run of several steps is two launches); two_areas: the plan as it is (else mutated: every run on
// partial-row area A, the negative control)
static Result plan(const Loop& sp, int run_max, bool defer, bool two_areas) {
  Config cf;
  cf.run_max = run_max;
  cf.defer = defer;
  cf.one_area = !two_areas;
  return check(sp, cf);
}
static int fails = 0;
static Result expect_clean(const Loop& sp, int run_max, const char* what, int p0, int p1) {
  Result on;
  for (int defer = 0; defer < 2; ++defer) {
    const Result r = plan(sp, run_max, defer, true);
    if (r.unordered || r.in_run || r.differs || (!defer && r.unordered_steps)) {
      std::printf("FAIL %s (%d, %d) run_max=%d defer=%d: unordered %d / %d, inside a run %d, decisions %d\n", what, p0, p1, run_max, defer, r.unordered, r.unordered_steps,
                  r.in_run, r.differs);
      ++fails;
    }
    if (!defer && r.carried) { std::printf("FAIL %s (%d, %d): carried with the switch off\n", what, p0, p1); ++fails; }
    on = r;
  }
  return on;
}
int main() {
  const int maxima[3] = {2, 4, 8};
  int ops_max = 0;
  for (int mi = 0; mi < 3; ++mi) {
    const int rm = maxima[mi];
    // rotating buffer sets, 1 .. 9 and 16 of them, every length
    for (int nsets = 1; nsets <= 16; nsets = nsets == 9 ? 16 : nsets + 1)
      for (int K = 1; K <= 40; ++K) {
        const Result r = expect_clean(rotation(K, nsets), rm, "rotating sets", nsets, K);
        // as many sets as a run has steps: every run after the first carries, and one flush ends the call (or precedes the single steps)
        if (nsets == rm && r.multi >= 1 && (r.carried != r.multi - 1 || r.flushed != 1)) {
          std::printf("FAIL rotation over %d sets, K=%d: %d runs of several, %d carried, %d flushed\n", nsets, K, r.multi, r.carried, r.flushed);
          ++fails;
        }
      }
    for (int K = 1; K <= 40; ++K) {
      Loop a, a2, b, b2, c, c2, d;
      for (int i = 0; i < K; ++i) {
        a.push_back(spans_of(i, i, 0));                       // ONE workspace for all steps: single steps
        a2.push_back(spans_of(i, i, i % rm));                 // workspaces in rotation, everything else a step's own: carried
        b.push_back(spans_chain(i == 0 ? 99 : i - 1, i, i));  // dims -> dims, step to step: single steps
        b2.push_back(i < rm ? spans_of(i, i, i) : spans_chain(i - rm, i, i % rm));  // ... run to run: runs form, none may carry
        StepSpans g = spans_of(i, i, i);
        g.wr[2] = byte_span(mem + 150 * 1024, 64);            // ONE gf_out for all steps: single steps
        c.push_back(g);
        StepSpans g2 = spans_of(i, i, i);
        g2.wr[2] = byte_span(mem + 150 * 1024 + (i % rm) * 64, 64);  // gf_out in rotation: carried
        c2.push_back(g2);
        d.push_back(spans_of(i, i, i % rm, (i / rm) % 2 ? 32 : 0));  // workspaces that overlap the previous run's without being the same: never carried
      }
      expect_clean(a, rm, "shared workspace", K, 0);
      const Result ra2 = expect_clean(a2, rm, "workspaces in rotation", K, 0);
      expect_clean(b, rm, "dims -> dims", K, 0);
      const Result rb2 = expect_clean(b2, rm, "feedback run to run", K, 0);
      expect_clean(c, rm, "shared gf_out", K, 0);
      const Result rc2 = expect_clean(c2, rm, "gf_out in rotation", K, 0);
      const Result rd = expect_clean(d, rm, "overlapping workspaces", K, 0);
      if (rb2.carried || rd.carried) { std::printf("FAIL: feedback / overlapping workspaces carried, K=%d run_max=%d\n", K, rm); ++fails; }
      if (rb2.multi >= 2 && rb2.flushed != rb2.multi) { std::printf("FAIL: feedback K=%d run_max=%d: %d runs, %d flushes\n", K, rm, rb2.multi, rb2.flushed); ++fails; }
      if (ra2.multi >= 1 && (ra2.carried != ra2.multi - 1 || rc2.carried != rc2.multi - 1)) { std::printf("FAIL: rotation of workspaces / gf_out not carried, K=%d run_max=%d\n", K, rm); ++fails; }
    }
    // random reuse of inputs, outputs and workspaces from small pools (some workspaces shifted onto their neighbours, some steps fed back)
    unsigned x = 4321u + 77u * (unsigned)rm;
    auto rnd = [&](int m) { x = x * 1664525u + 1013904223u; return (int)((x >> 8) % (unsigned)m); };
    for (int trial = 0; trial < 2500 && !fails; ++trial) {
      const int K = 1 + rnd(40), m = 1 + rnd(20), period = 1 + rnd(12);
      Loop sp;
      for (int i = 0; i < K; ++i) {
        const int mode = rnd(8);
        if (mode == 0 && i > 0) sp.push_back(spans_chain(rnd(m), rnd(m), rnd(m)));
        else if (mode == 1) sp.push_back(spans_of(rnd(m), rnd(m), rnd(m), 32));
        else if (mode <= 4) sp.push_back(spans_of(i % period, i % period, i % period));  // stretches of a rotation, so that runs form
        else sp.push_back(spans_of(20 + i, 20 + i, i % period));
      }
      const Result r = expect_clean(sp, rm, "random", trial, K);
      if (r.ops_max > ops_max) ops_max = r.ops_max;
    }
  }
  // known loops at run maximum 8 on 8 sets: 20 steps = 8 + 8 + 4, two carried and one flush; 12 steps = 8 + a tail of 4, carried; 9 steps =
  // a run and one step: the run's graph updates are flushed before the step
  {
    const Loop a = rotation(20, 8), b = rotation(12, 8), c = rotation(9, 8);
    const Result ra = plan(a, 8, true, true), rb = plan(b, 8, true, true), rc = plan(c, 8, true, true);
    if (ra.runs != 3 || ra.carried != 2 || ra.flushed != 1 || rb.runs != 2 || rb.carried != 1 || rb.flushed != 1 || rc.runs != 2 || rc.carried != 0 || rc.flushed != 1 ||
        ra.unordered || rb.unordered || rc.unordered) {
      std::printf("FAIL known loops: %d/%d/%d %d/%d/%d %d/%d/%d\n", ra.runs, ra.carried, ra.flushed, rb.runs, rb.carried, rb.flushed, rc.runs, rc.carried, rc.flushed);
      ++fails;
    }
    // the negative control: with ONE partial-row area the carried graph updates read the rows the carrying run's tiles write
    if (!plan(a, 8, true, false).unordered || !plan(b, 8, true, false).unordered) { std::printf("FAIL: one partial-row area was not flagged\n"); ++fails; }
    if (plan(c, 8, true, false).unordered) { std::printf("FAIL: one partial-row area flagged where nothing is carried\n"); ++fails; }
  }
  // the fixed-capacity operation list: no run of the sweep needs more than its seven operations
  if (ops_max > StepsPlan::kMax - 1) { std::printf("FAIL: a run of %d operations\n", ops_max); ++fails; }
  if (fails) return 1;
  std::printf("deferred ok (most operations in a run: %d)\n", ops_max);
  return 0;
}
"""


def test_carrying_runs_order_every_conflicting_pair(tmp_path):
    src = tmp_path / "deferred.cpp"
    src.write_text(SCHEDULE)
    exe = tmp_path / "deferred"
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "tests", "c"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "deferred ok" in out.stdout


def _key(de, dn, dg, oe, on):
    return "".join(f"Li{v}E" for v in (de, dn, dg, oe, on, 2))


# the width sets and graph-count forms with a carrying kernel (gnx_narrow_sets.h: NF_CARRY1 / NF_CARRYG), as the mangled names spell them
CARRY = {(_key(*d), g) for d in ((10, 5, 0, 3, 4), (3, 4, 5, 3, 4), (10, 5, 3, 3, 4), (0, 2, 0, 2, 2), (4, 3, 2, 3, 4)) for g in "01"}


def test_carrying_kernels_resource_audit():
    """Every k_block_wave_carry instantiation, compiled as build.py compiles gnx_narrow.hip: no scratch, at most 80 scalar registers (the
    eighth workgroup per CU), no more vector registers than the chained kernel of the same set and form; exactly the listed instantiations,
    fp32 rows only."""
    from tools.kernel_resources import HIPCC, remarks
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    res = remarks("gnx_narrow.hip")
    pat = re.compile(r"_ZN3gnx18k_block_wave_carryI((?:Li\d+E){6})Lb([01])EEEv")
    carry = {n: v for n, v in res.items() if "k_block_wave_carry" in n}
    assert all(pat.match(n) for n in carry), sorted(carry)
    assert {pat.match(n).groups() for n in carry} == CARRY, sorted(carry)
    for n, v in carry.items():
        dims, oneg = pat.match(n).groups()
        c = [w for m, w in res.items() if m.startswith(f"_ZN3gnx12k_block_waveI{dims}Lb0ELb{oneg}ELb0ELb0ELb1ELb0EEEv")]
        assert len(c) == 1, f"no chained kernel for {dims} ONEG={oneg}"
        print(n, v, "chained:", c[0])
        assert v["scratch"] == 0, (n, v)
        assert v["sgpr"] <= 80, (n, v)
        assert v["vgpr"] <= c[0]["vgpr"], (n, v, c[0])
    # (the bf16 kernels keep the two launches per run)
    with open(os.path.join(CSRC, "gnx_narrow_bf16.hip")) as f:
        assert "k_block_wave_carry" not in f.read()
