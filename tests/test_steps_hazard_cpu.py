"""The host-side hazard rule of gnx_block_forward_steps' two-stream schedule (graphnets.jl_amd/csrc/gnx_step_hazard.h), compiled on its
own with g++: two steps may be in flight together only if no byte range one writes overlaps a range the other reads or writes; and the
two-stream schedule of single steps built on it — the library's planner (StepsPlanner) at a run maximum of 1 — checked by simulating the
order its operations enforce (tests/c/steps_plan_sim.h)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include "gnx_step_hazard.h"
using namespace gnx;
static char buf[1 << 16];
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
// a step: inputs at in[0..2], outputs at out[0..2], workspace at ws; each 256 bytes
static StepSpans step(int in0, int in1, int in2, int o0, int o1, int o2, int ws, size_t n = 256) {
  StepSpans s;
  const int in[3] = {in0, in1, in2}, out[4] = {o0, o1, o2, ws};
  for (int t = 0; t < 3; ++t) s.rd[t] = in[t] < 0 ? ByteSpan{} : byte_span(buf + in[t], n);
  for (int t = 0; t < 4; ++t) s.wr[t] = out[t] < 0 ? ByteSpan{} : byte_span(buf + out[t], n);
  return s;
}
int main() {
  // the spans themselves: half-open, empty for NULL or zero bytes
  EXPECT(spans_overlap(byte_span(buf, 16), byte_span(buf + 15, 16)));
  EXPECT(!spans_overlap(byte_span(buf, 16), byte_span(buf + 16, 16)));
  EXPECT(!spans_overlap(byte_span(buf + 16, 16), byte_span(buf, 16)));
  EXPECT(spans_overlap(byte_span(buf, 64), byte_span(buf + 8, 8)));
  EXPECT(!spans_overlap(byte_span(buf, 0), byte_span(buf, 16)));
  EXPECT(!spans_overlap(byte_span(nullptr, 16), byte_span(nullptr, 16)));
  // two disjoint buffer sets: independent
  const StepSpans a = step(0, 256, 512, 1024, 1280, 1536, 2048);
  const StepSpans b = step(4096, 4352, 4608, 5120, 5376, 5632, 6144);
  EXPECT(!steps_conflict(a, b) && !steps_conflict(b, a));
  // the same set twice: every pair aliases
  EXPECT(steps_conflict(a, a));
  // both READ the same inputs: still independent
  const StepSpans c = step(0, 256, 512, 5120, 5376, 5632, 6144);
  EXPECT(!steps_conflict(a, c) && !steps_conflict(c, a));
  // dims -> dims: the next step reads this step's outputs (each output alone is enough), in either argument order
  EXPECT(steps_conflict(a, step(1024, 4352, 4608, 5120, 5376, 5632, 6144)));
  EXPECT(steps_conflict(step(4096, 1280, 4608, 5120, 5376, 5632, 6144), a));
  EXPECT(steps_conflict(a, step(4096, 4352, 1536, 5120, 5376, 5632, 6144)));
  // one shared workspace, or one shared output
  EXPECT(steps_conflict(a, step(4096, 4352, 4608, 5120, 5376, 5632, 2048)));
  EXPECT(steps_conflict(a, step(4096, 4352, 4608, 5120, 5376, 1536, 6144)));
  // a step that WRITES what the other reads, the other way round
  EXPECT(steps_conflict(a, step(4096, 4352, 4608, 0, 5376, 5632, 6144)));
  EXPECT(steps_conflict(step(4096, 4352, 4608, 5120, 5376, 5632, 200), a));
  // partial overlap of one byte at a range's end; touching ranges do not overlap
  EXPECT(steps_conflict(a, step(4096, 4352, 4608, 5120, 5376, 5632, 2048 + 255)));
  EXPECT(!steps_conflict(a, step(4096, 4352, 4608, 5120, 5376, 5632, 2048 + 256)));
  // widths of 0 (`nothing`): absent ranges never conflict
  EXPECT(!steps_conflict(step(-1, 256, -1, -1, 1280, -1, 2048), step(-1, 4352, -1, -1, 5376, -1, 6144)));
  if (fails) return 1;
  std::printf("hazard rule ok\n");
  return 0;
}
"""


def test_step_hazard_rule(tmp_path):
    src = tmp_path / "hazard.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "hazard"
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "graphnets.jl_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "hazard rule ok" in out.stdout


SCHEDULE = r"""
#include "steps_plan_sim.h"
using namespace sim;
// The planner at a run maximum of 1, on two streams: every run is one step.  Returns the unordered conflicting pairs (by whole steps: nothing
// is carried here) plus every way the plan is not the schedule of single steps.
static int check1(const Loop& sp, bool chain, bool wait3) {
  Config cf;
  cf.run_max = 1;
  cf.chain = chain;
  cf.drop_wait3 = !wait3;
  const Result r = check(sp, cf);
  return r.unordered + r.unordered_steps + r.differs + r.in_run + r.multi + r.carried + r.flushed;
}
int main() {
  int fails = 0;
  for (int chain = 0; chain < 2; ++chain) {
    // rotating buffer sets: every count, every length
    for (int nsets = 1; nsets <= 9; ++nsets)
      for (int K = 1; K <= 24; ++K)
        if (int b = check1(rotation(K, nsets), chain, true)) { std::printf("FAIL rotating nsets=%d K=%d chain=%d: %d\n", nsets, K, chain, b); ++fails; }
    // one shared workspace; dims -> dims
    for (int K = 1; K <= 12; ++K) {
      Loop a, b;
      for (int i = 0; i < K; ++i) { a.push_back(spans_of(i, i, 0)); b.push_back(spans_chain(i == 0 ? 99 : i - 1, i, i)); }
      if (check1(a, chain, true) || check1(b, chain, true)) { std::printf("FAIL shared / chain K=%d\n", K); ++fails; }
    }
    // random reuse of inputs, outputs and workspaces from small pools
    unsigned x = 12345u;
    auto rnd = [&](int m) { x = x * 1664525u + 1013904223u; return (int)((x >> 8) % (unsigned)m); };
    for (int trial = 0; trial < 3000; ++trial) {
      const int K = 1 + rnd(20), m = 1 + rnd(7);
      Loop sp;
      for (int i = 0; i < K; ++i) sp.push_back(rnd(4) == 0 && i > 0 ? spans_chain(rnd(m), rnd(m), rnd(m)) : spans_of(rnd(m), rnd(m), rnd(m)));
      if (int b = check1(sp, chain, true)) { std::printf("FAIL random trial %d chain=%d: %d\n", trial, chain, b); ++fails; break; }
    }
  }
  // the checker sees the race the wait for step i - 3 prevents: five rotating sets with that wait dropped from the plan
  if (!check1(rotation(12, 5), true, false)) { std::printf("FAIL: five rotating sets without the step i - 3 wait were not flagged\n"); ++fails; }
  if (fails) return 1;
  std::printf("schedule ok\n");
  return 0;
}
"""


def test_two_stream_schedule_orders_every_conflicting_pair(tmp_path):
    src = tmp_path / "schedule.cpp"
    src.write_text(SCHEDULE)
    exe = tmp_path / "schedule"
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "graphnets.jl_amd", "csrc"), "-I", os.path.join(ROOT, "tests", "c"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "schedule ok" in out.stdout
