"""Runs of gnx_block_forward_steps (graphnets.jl_amd/csrc/gnx_step_hazard.h: neighbouring, hazard-free steps that share one launch), compiled on
their own with g++: the grouping (a full window of conflict-free neighbours or the last four or more steps of the loop, else one step) never
puts two conflicting steps into a run; the two-stream schedule of runs (run_order + the wait of run
j for run j - 3), simulated as a happens-before relation, orders every conflicting pair of steps; with a run maximum of 1 the decisions are
step_order's.  And the resource limits of the run kernels (k_block_wave_run), read from the compiler's resource remarks for gfx950."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphnets.jl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SCHEDULE = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gnx_step_hazard.h"
using namespace gnx;
// Simulation of gnx_block_forward_steps' schedule of runs (gnx_forward.hip: steps_schedule) as a happens-before relation: launches are nodes
// on two streams (stream order), plus the waits the schedule adds.  An activity is a step's edge + node update or its graph update.  A run of
// one step is one launch (its graph update chained into the next one-step launch on its stream, or a flush launch); a run of several steps is
// a launch with the edge + node updates of all of them — nothing orders those against each other — and a second one with their graph updates.
// Every two activities of different steps whose buffers conflict must be ordered, whatever the streams' relative progress.
struct Node { int stream; std::vector<int> steps; };
struct Sim {
  std::vector<Node> nodes;
  std::vector<std::vector<int>> deps;  // explicit edges into a node
  int last[2] = {-1, -1};
  int add(int stream, std::vector<int> steps, std::vector<int> extra) {
    nodes.push_back({stream, steps});
    if (last[stream] >= 0) extra.push_back(last[stream]);
    deps.push_back(extra);
    return last[stream] = (int)nodes.size() - 1;
  }
};
static char mem[1 << 20];
static StepSpans spans_of(int in_set, int out_set, int ws_set) {
  StepSpans s;
  for (int t = 0; t < 3; ++t) s.rd[t] = byte_span(mem + in_set * 1024 + t * 64, 64);
  for (int t = 0; t < 3; ++t) s.wr[t] = byte_span(mem + out_set * 1024 + 512 + t * 64, 64);
  s.wr[3] = byte_span(mem + 200 * 1024 + ws_set * 64, 64);
  return s;
}
// dims -> dims: the inputs of a step are the outputs of src_out_set
static StepSpans spans_chain(int src_out_set, int out_set, int ws_set) {
  StepSpans s = spans_of(0, out_set, ws_set);
  for (int t = 0; t < 3; ++t) s.rd[t] = byte_span(mem + src_out_set * 1024 + 512 + t * 64, 64);
  return s;
}
static bool same_span(ByteSpan a, ByteSpan b) { return a.lo == b.lo && a.hi == b.hi; }
struct Result { int unordered = 0, in_run = 0, runs = 0, longest = 0, differs = 0; };
// two: the two-stream schedule; else every run on one stream (a pending graph update rides at the front of the next one-step launch)
static Result check(const std::vector<StepSpans>& sp, int run_max, bool chain, bool wait3, bool two) {
  const long long K = (long long)sp.size();
  Result res;
  Sim sim;
  int pend[2] = {-1, -1};
  std::vector<int> run_end;
  RunSpans recent[3];
  StepSpans srecent[3];
  long long i = 0;
  for (long long j = 0; i < K; ++j) {
    const RunSpans cur = group_run(sp.data(), K, i, run_max);
    if (cur.n < 1 || cur.n > run_max || cur.n > kRunMax) { ++res.differs; break; }
    for (int a = 0; a < cur.n; ++a) {
      for (int t = 0; t < 4; ++t) if (!same_span(cur.step[a].wr[t], sp[i + a].wr[t])) ++res.differs;  // the run is steps i .. i + n - 1, in order
      for (int b = a + 1; b < cur.n; ++b) if (steps_conflict(cur.step[a], cur.step[b])) ++res.in_run;
    }
    // a run is the greedy window if it is full or the end of the loop cut it at four steps or more; else one step
    {
      int len = 1;
      for (; len < run_max && i + len < K; ++len) {
        bool clash = false;
        for (int a = 0; a < len; ++a) clash = clash || steps_conflict(sp[i + a], sp[i + len]);
        if (clash) break;
      }
      const bool is_run = len >= 2 && (len == run_max || (i + len == K && len >= 4));
      if (cur.n != (is_run ? len : 1)) ++res.differs;
    }
    ++res.runs;
    if (cur.n > res.longest) res.longest = cur.n;
    const int k = two ? (int)(j & 1) : 0, o = k ^ 1;
    StepOrder ord;
    if (two) ord = run_order(cur, recent, j);
    else ord.flush_own = j >= 1 && runs_conflict(cur, recent[0]);
    if (run_max == 1 && two) {  // a run maximum of 1: the decisions of the schedule of single steps
      const StepOrder so = step_order(sp[i], srecent, i);
      if (cur.n != 1 || j != i || so.flush_own != ord.flush_own || so.after_other != ord.after_other) ++res.differs;
    }
    if ((ord.flush_own || cur.n > 1) && pend[k] >= 0) { sim.add(k, {pend[k]}, {}); pend[k] = -1; }
    std::vector<int> extra;
    if (two && wait3 && j >= 3) extra.push_back(run_end[j - 3]);
    if (ord.after_other) {
      if (pend[o] >= 0) { sim.add(o, {pend[o]}, {}); pend[o] = -1; }
      if (sim.last[o] >= 0) extra.push_back(sim.last[o]);
    }
    std::vector<int> acts;
    for (int a = 0; a < cur.n; ++a) acts.push_back((int)i + a);
    if (cur.n > 1) {
      sim.add(k, acts, extra);                     // the edge + node updates of every slot
      run_end.push_back(sim.add(k, acts, {}));     // their graph updates, right behind
    } else {
      if (pend[k] >= 0) acts.push_back(pend[k]);   // the chained graph update of the last one-step run on this stream, at the front
      run_end.push_back(sim.add(k, acts, extra));
      pend[k] = chain ? (int)i : -1;               // (not chained: the step's graph update is inside its own launch)
    }
    recent[2] = recent[1]; recent[1] = recent[0]; recent[0] = cur;
    srecent[2] = srecent[1]; srecent[1] = srecent[0]; srecent[0] = sp[i];
    i += cur.n;
  }
  for (int k = 0; k < 2; ++k)
    if (pend[k] >= 0) sim.add(k, {pend[k]}, {});
  const int n = (int)sim.nodes.size();
  std::vector<std::vector<char>> r(n, std::vector<char>(n, 0));  // r[a][b]: a ends before b starts
  for (int b = 0; b < n; ++b)
    for (int a : sim.deps[b]) {
      r[a][b] = 1;
      for (int x = 0; x < n; ++x) if (r[x][a]) r[x][b] = 1;
    }
  for (int a = 0; a < n; ++a)
    for (int b = a; b < n; ++b) {
      if (a != b && (r[a][b] || r[b][a])) continue;
      for (int s : sim.nodes[a].steps)
        for (int t : sim.nodes[b].steps)
          if (s != t && steps_conflict(sp[s], sp[t])) ++res.unordered;
    }
  return res;
}
static int fails = 0;
static void expect_clean(const std::vector<StepSpans>& sp, int run_max, bool chain, const char* what, int p0, int p1) {
  for (int two = 0; two < 2; ++two) {
    const Result r = check(sp, run_max, chain, true, two);
    if (r.unordered || r.in_run || r.differs) {
      std::printf("FAIL %s (%d, %d) run_max=%d chain=%d two=%d: unordered %d, inside a run %d, decisions %d\n", what, p0, p1, run_max, (int)chain, two, r.unordered,
                  r.in_run, r.differs);
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
          std::vector<StepSpans> sp;
          for (int i = 0; i < K; ++i) sp.push_back(spans_of(i % nsets, i % nsets, i % nsets));
          expect_clean(sp, rm, chain, "rotating sets", nsets, K);
          // the grouping itself: full runs where the rotation and the step count allow them
          const Result r = check(sp, rm, chain, true, true);
          if (nsets >= rm && K >= rm && r.longest != rm) { std::printf("FAIL longest run nsets=%d K=%d run_max=%d: %d\n", nsets, K, rm, r.longest); ++fails; }
          if (r.longest > (nsets < rm ? nsets : rm)) { std::printf("FAIL run longer than the rotation nsets=%d K=%d run_max=%d: %d\n", nsets, K, rm, r.longest); ++fails; }
        }
      // one shared workspace; one shared gf_out; dims -> dims: every step conflicts with its predecessor, so every run is one step
      for (int K = 1; K <= 12; ++K) {
        std::vector<StepSpans> a, b, c;
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
        if (check(a, rm, chain, true, true).longest != 1 || check(b, rm, chain, true, true).longest != 1 || check(c, rm, chain, true, true).longest != 1) {
          std::printf("FAIL: conflicting neighbours shared a run, K=%d run_max=%d\n", K, rm);
          ++fails;
        }
      }
      // random reuse of inputs, outputs and workspaces from small pools
      unsigned x = 12345u + 77u * (unsigned)rm;
      auto rnd = [&](int m) { x = x * 1664525u + 1013904223u; return (int)((x >> 8) % (unsigned)m); };
      for (int trial = 0; trial < 2500 && !fails; ++trial) {
        const int K = 1 + rnd(28), m = 1 + rnd(12);
        std::vector<StepSpans> sp;
        for (int i = 0; i < K; ++i) sp.push_back(rnd(4) == 0 && i > 0 ? spans_chain(rnd(m), rnd(m), rnd(m)) : spans_of(rnd(m), rnd(m), rnd(m)));
        expect_clean(sp, rm, chain, "random", trial, K);
      }
    }
  }
  // the grouping on three known loops at run maximum 8: 20 steps on 8 sets are runs of 8, 8 and 4; 8 steps on 4 sets are four single steps
  // (a conflict cuts their windows) and the last four as a run; three steps are single steps
  {
    std::vector<StepSpans> a, b, c;
    for (int i = 0; i < 20; ++i) a.push_back(spans_of(i % 8, i % 8, i % 8));
    for (int i = 0; i < 8; ++i) b.push_back(spans_of(i % 4, i % 4, i % 4));
    for (int i = 0; i < 3; ++i) c.push_back(spans_of(i, i, i));
    const Result ra = check(a, 8, true, true, true), rb = check(b, 8, true, true, true), rc = check(c, 8, true, true, true);
    if (ra.runs != 3 || ra.longest != 8 || rb.runs != 5 || rb.longest != 4 || rc.runs != 3 || rc.longest != 1) {
      std::printf("FAIL known loops: %d/%d %d/%d %d/%d\n", ra.runs, ra.longest, rb.runs, rb.longest, rc.runs, rc.longest);
      ++fails;
    }
  }
  // the checker sees the race the wait for run j - 3 prevents: without it, five rotating sets at run maximum 1 (step i + 5 reuses step i's
  // set on the other stream, beyond run_order's look-back) and ten sets in runs of two (run j + 5 reuses run j's) are unordered
  {
    std::vector<StepSpans> sp;
    for (int i = 0; i < 12; ++i) sp.push_back(spans_of(i % 5, i % 5, i % 5));
    if (!check(sp, 1, true, false, true).unordered) { std::printf("FAIL: five rotating sets without the wait for run j - 3 were not flagged\n"); ++fails; }
    std::vector<StepSpans> sq;
    for (int i = 0; i < 48; ++i) sq.push_back(spans_of(i % 10, i % 10, i % 10));
    if (!check(sq, 2, true, false, true).unordered) { std::printf("FAIL: ten rotating sets in runs of two without the wait for run j - 3 were not flagged\n"); ++fails; }
  }
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
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "runs ok" in out.stdout


def _resources(stderr):
    """kernel -> {sgpr, vgpr, scratch} from -Rpass-analysis=kernel-resource-usage remarks"""
    out = {}
    for blk in re.split(r"remark: Function Name: ", stderr)[1:]:
        name = blk.split()[0]
        g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))
        out[name] = dict(sgpr=g("TotalSGPRs"), vgpr=g("VGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"))
    return out


# the width sets with a run kernel (gnx_narrow.hip: GNX_NARROW_RUN_DIMS; gnx_narrow_bf16.hip: GNX_NARROW_RUN_DIMS_BF16), as the mangled names spell them
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
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    base = [HIPCC, "-x", "hip", "-c", "--cuda-device-only", "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
            "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull]
    procs = {k: subprocess.Popen(base + extra + [os.path.join(CSRC, f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for k, f, extra in (("bf16", "gnx_narrow_bf16.hip", ["-fno-slp-vectorize"]), ("f32", "gnx_narrow.hip", []))}
    res = {}
    for k, p in procs.items():
        _, err = p.communicate(timeout=1200)
        assert p.returncode == 0, err[-3000:]
        res[k] = _resources(err)
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
