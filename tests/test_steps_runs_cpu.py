"""Runs of gnx_block_forward_steps (graphnets.jl_amd/csrc/gnx_step_hazard.h: neighbouring, hazard-free steps that share one launch), compiled on
their own with g++: the grouping (a full window of conflict-free neighbours or the last four or more steps of the loop, else one step) never
puts two conflicting steps into a run; the operations the library's planner (StepsPlanner) returns for runs without carrying, on two streams
and on one, simulated as a happens-before relation (tests/c/steps_plan_sim.h), order every conflicting pair of steps; with a run maximum of 1
the plan is the schedule of single steps.  And the resource limits of the run kernels (k_block_wave_run), read from the compiler's resource remarks for gfx950."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphnets.jl_amd", "csrc")

SCHEDULE = r"""
#include "steps_plan_sim.h"
using namespace sim;
// runs without carrying (the switch off: a run of several steps is its block launch and its graph updates right behind it), on two streams
// and on one; chain: a one-step launch leaves its graph update pending
static Result runs(const Loop& sp, int run_max, bool chain, bool two = true, bool wait3 = true) {
  Config cf;
  cf.run_max = run_max;
  cf.two = two;
  cf.defer = false;
  cf.chain = chain;
  cf.drop_wait3 = !wait3;
  return check(sp, cf);
}
static int fails = 0;
static void expect_clean(const Loop& sp, int run_max, bool chain, const char* what, int p0, int p1) {
  for (int two = 0; two < 2; ++two) {
    const Result r = runs(sp, run_max, chain, two);
    if (r.unordered || r.unordered_steps || r.in_run || r.differs || r.carried) {
      std::printf("FAIL %s (%d, %d) run_max=%d chain=%d two=%d: unordered %d / %d, inside a run %d, decisions %d\n", what, p0, p1, run_max, (int)chain, two, r.unordered,
                  r.unordered_steps, r.in_run, r.differs);
      ++fails;
    }
  }
}
int main() {
  const int maxima[4] = {1, 2, 4, 8};
  for (int mi = 0; mi < 4; ++mi) {
    const int rm = maxima[mi];
    for (int chain = 0; chain < 2; ++chain) {
      // rotating buffer sets: every count, every length
      for (int nsets = 1; nsets <= 9; ++nsets)
        for (int K = 1; K <= 24; ++K) {
          const Loop sp = rotation(K, nsets);
          expect_clean(sp, rm, chain, "rotating sets", nsets, K);
          // the grouping itself: full runs where the rotation and the step count allow them
          const Result r = runs(sp, rm, chain);
          if (nsets >= rm && K >= rm && r.longest != rm) { std::printf("FAIL longest run nsets=%d K=%d run_max=%d: %d\n", nsets, K, rm, r.longest); ++fails; }
          if (r.longest > (nsets < rm ? nsets : rm)) { std::printf("FAIL run longer than the rotation nsets=%d K=%d run_max=%d: %d\n", nsets, K, rm, r.longest); ++fails; }
        }
      // one shared workspace; one shared gf_out; dims -> dims: every step conflicts with its predecessor, so every run is one step
      for (int K = 1; K <= 12; ++K) {
        Loop a, b, c;
        for (int i = 0; i < K; ++i) {
          a.push_back(spans_of(i, i, 0));
          b.push_back(spans_chain(i == 0 ? 99 : i - 1, i, i));
          StepSpans g = spans_of(i, i, i);
          g.wr[2] = byte_span(mem + 150 * 1024, 64);
          c.push_back(g);
        }
        expect_clean(a, rm, chain, "shared workspace", K, 0);
        expect_clean(b, rm, chain, "dims -> dims", K, 0);
        expect_clean(c, rm, chain, "shared gf_out", K, 0);
        if (runs(a, rm, chain).longest != 1 || runs(b, rm, chain).longest != 1 || runs(c, rm, chain).longest != 1) {
          std::printf("FAIL: conflicting neighbours shared a run, K=%d run_max=%d\n", K, rm);
          ++fails;
        }
      }
      // random reuse of inputs, outputs and workspaces from small pools
      unsigned x = 12345u + 77u * (unsigned)rm;
      auto rnd = [&](int m) { x = x * 1664525u + 1013904223u; return (int)((x >> 8) % (unsigned)m); };
      for (int trial = 0; trial < 2500 && !fails; ++trial) {
        const int K = 1 + rnd(28), m = 1 + rnd(12);
        Loop sp;
        for (int i = 0; i < K; ++i) sp.push_back(rnd(4) == 0 && i > 0 ? spans_chain(rnd(m), rnd(m), rnd(m)) : spans_of(rnd(m), rnd(m), rnd(m)));
        expect_clean(sp, rm, chain, "random", trial, K);
      }
    }
  }
  // the grouping on three known loops at run maximum 8: 20 steps on 8 sets are runs of 8, 8 and 4; 8 steps on 4 sets are four single steps
  // (a conflict cuts their windows) and the last four as a run; three steps are single steps
  {
    Loop c;
    for (int i = 0; i < 3; ++i) c.push_back(spans_of(i, i, i));
    const Result ra = runs(rotation(20, 8), 8, true), rb = runs(rotation(8, 4), 8, true), rc = runs(c, 8, true);
    if (ra.runs != 3 || ra.longest != 8 || rb.runs != 5 || rb.longest != 4 || rc.runs != 3 || rc.longest != 1) {
      std::printf("FAIL known loops: %d/%d %d/%d %d/%d\n", ra.runs, ra.longest, rb.runs, rb.longest, rc.runs, rc.longest);
      ++fails;
    }
  }
  // the checker sees the race the wait for run j - 3 prevents: with that wait dropped from the plan, five rotating sets at run maximum 1
  // (step i + 5 reuses step i's set on the other stream, beyond run_order's look-back) and ten sets in runs of two (run j + 5 reuses run
  // j's) are unordered
  if (!runs(rotation(12, 5), 1, true, true, false).unordered_steps) { std::printf("FAIL: five rotating sets without the wait for run j - 3 were not flagged\n"); ++fails; }
  if (!runs(rotation(48, 10), 2, true, true, false).unordered_steps) { std::printf("FAIL: ten rotating sets in runs of two without the wait for run j - 3 were not flagged\n"); ++fails; }
  if (fails) return 1;
  std::printf("runs ok\n");
  return 0;
}
"""


def test_runs_grouping_and_schedule_order_every_conflicting_pair(tmp_path):
    src = tmp_path / "runs.cpp"
    src.write_text(SCHEDULE)
    exe = tmp_path / "runs"
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "tests", "c"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "runs ok" in out.stdout


# the width sets with a run kernel (gnx_narrow_sets.h: NF_RUN1 / NF_RUNG of either list), as the mangled names spell them
def _key(de, dn, dg, oe, on):
    return "".join(f"Li{v}E" for v in (de, dn, dg, oe, on, 2))


RUN_F32 = {(_key(*d), g) for d in ((10, 5, 0, 3, 4), (3, 4, 5, 3, 4), (10, 5, 3, 3, 4), (0, 2, 0, 2, 2), (2, 2, 2, 2, 2), (4, 3, 2, 3, 4)) for g in "01"}
RUN_BF16 = {(_key(10, 5, 0, 3, 4), "1"), (_key(3, 4, 5, 3, 4), "0"), (_key(3, 4, 5, 3, 4), "1")}
WIDE_F32 = {_key(8, 8, 8, 16, 8), _key(10, 5, 3, 10, 5), _key(10, 5, 0, 10, 5)}  # chained, but no run kernel: see the last assertion


def test_run_kernels_resource_audit():
    """Every k_block_wave_run instantiation (one graph and several graphs, fp32 and bf16), compiled as build.py compiles the two files: no
    scratch, at most 80 scalar registers (the eighth workgroup per CU), no more vector registers than the chained kernel of the same set.
    The instantiations are exactly the listed ones; the fp32 sets that chain but have no run kernel are the ones whose kernels are beyond the
    80 scalar registers in every form."""
    from tools.kernel_resources import HIPCC, remarks_many
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    res = dict(zip(("bf16", "f32"), remarks_many(["gnx_narrow_bf16.hip", "gnx_narrow.hip"])))  # (both compiles at once, as build.py compiles the files)
    pat = re.compile(r"_ZN3gnx16k_block_wave_runI((?:Li\d+E){6})Lb([01])ELb([01])EEEv")

    def chained(key, dims, oneg, bf16):  # k_block_wave<dims, LN = 0, ONEG, PACK = 0, FFE = 0, CHAIN = 1, BF16>
        c = [v for m, v in res[key].items() if m.startswith(f"_ZN3gnx12k_block_waveI{dims}Lb0ELb{oneg}ELb0ELb0ELb1ELb{bf16}EEEv")]
        assert len(c) == 1, f"no chained kernel for {dims} ONEG={oneg} in the {key} file"
        return c[0]

    for key, want_bf16, listed in (("f32", "0", RUN_F32), ("bf16", "1", RUN_BF16)):
        runs = {n: v for n, v in res[key].items() if pat.match(n)}
        assert {pat.match(n).groups()[:2] for n in runs} == listed, sorted(runs)
        for n, v in runs.items():
            dims, oneg, bf16 = pat.match(n).groups()
            assert bf16 == want_bf16, n
            c = chained(key, dims, oneg, bf16)
            print(n, v, "chained:", c)
            assert v["scratch"] == 0, (n, v)
            assert v["sgpr"] <= 80, (n, v)
            assert v["vgpr"] <= c["vgpr"], (n, v, c)
    for dims in WIDE_F32:
        for oneg in "01":
            assert chained("f32", dims, oneg, "0")["sgpr"] > 80, dims
