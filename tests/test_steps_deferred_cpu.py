"""Carrying runs of gnx_block_forward_steps (graphnets.jl_amd/csrc/gnx_step_hazard.h: run_defers, run_place), compiled on their own with g++:
the two-stream schedule of gnx_forward.hip's steps_schedule with runs whose block launch carries the graph updates of the run before it,
simulated as a happens-before relation over ACTIVITIES — a step's edge + node update, and its graph update wherever that ends up (behind its
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
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SCHEDULE = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gnx_step_hazard.h"
using namespace gnx;
// An activity: step s's edge + node update (kind 0: reads ef, nf, gf; writes ef_out, nf_out and the partial rows in area `area` of its
// workspace) or its graph update (kind 1: reads gf and those partial rows; writes gf_out).
struct Act { int step, kind, area; };
struct Node { int stream; std::vector<Act> acts; };
struct Sim {
  std::vector<Node> nodes;
  std::vector<std::vector<int>> deps;
  int last[2] = {-1, -1};
  int add(int stream, std::vector<Act> acts, std::vector<int> extra) {
    nodes.push_back({stream, acts});
    if (last[stream] >= 0) extra.push_back(last[stream]);
    deps.push_back(extra);
    return last[stream] = (int)nodes.size() - 1;
  }
};
static char mem[1 << 20];
// a workspace is 64 bytes: area B (the head of the agg area) its bytes [0, 16), area A (the block's own partial rows) its bytes [32, 48);
// shift 32: a workspace that overlaps its neighbour without being the same one (its area B is the neighbour's area A)
static StepSpans spans_of(int in_set, int out_set, int ws_set, int shift = 0) {
  StepSpans s;
  for (int t = 0; t < 3; ++t) s.rd[t] = byte_span(mem + in_set * 1024 + t * 64, 64);
  for (int t = 0; t < 3; ++t) s.wr[t] = byte_span(mem + out_set * 1024 + 512 + t * 64, 64);
  s.wr[3] = byte_span(mem + 200 * 1024 + ws_set * 64 + shift, 64);
  return s;
}
// dims -> dims: the inputs of a step are the outputs of src_out_set
static StepSpans spans_chain(int src_out_set, int out_set, int ws_set) {
  StepSpans s = spans_of(0, out_set, ws_set);
  for (int t = 0; t < 3; ++t) s.rd[t] = byte_span(mem + src_out_set * 1024 + 512 + t * 64, 64);
  return s;
}
static ByteSpan part(const StepSpans& s, int area) {
  ByteSpan p;
  p.lo = s.wr[3].lo + (area ? 0 : 32);
  p.hi = p.lo + 16;
  return p;
}
struct Bytes { std::vector<ByteSpan> rd, wr; };
static Bytes bytes_of(const std::vector<StepSpans>& sp, const Act& a) {
  const StepSpans& s = sp[a.step];
  Bytes b;
  if (a.kind == 0) { b.rd = {s.rd[0], s.rd[1], s.rd[2]}; b.wr = {s.wr[0], s.wr[1], part(s, a.area)}; }
  else { b.rd = {s.rd[2], part(s, a.area)}; b.wr = {s.wr[2]}; }
  return b;
}
static bool acts_conflict(const std::vector<StepSpans>& sp, const Act& a, const Act& b) {
  const Bytes x = bytes_of(sp, a), y = bytes_of(sp, b);
  for (const ByteSpan& w : x.wr) {
    for (const ByteSpan& r : y.rd) if (spans_overlap(w, r)) return true;
    for (const ByteSpan& v : y.wr) if (spans_overlap(w, v)) return true;
  }
  for (const ByteSpan& w : y.wr)
    for (const ByteSpan& r : x.rd) if (spans_overlap(w, r)) return true;
  return false;
}
struct Result { int unordered = 0, runs = 0, multi = 0, carried = 0, flushed = 0; };
// defer: runs may carry (else: every run of several steps is two launches, today's schedule); two_areas: a carrying run writes the area the
// run before it did not (else always area A: the negative control)
static Result check(const std::vector<StepSpans>& sp, int run_max, bool defer, bool two_areas) {
  const long long K = (long long)sp.size();
  Result res;
  Sim sim;
  int pend[2] = {-1, -1};
  std::vector<int> run_end;
  RunSpans recent[3];
  int rstream[3] = {0, 0, 0};
  struct { bool has = false; int first = 0, n = 0, area = 0, stream = 0; long long j = 0; } rp;
  auto graph_acts = [&](int first, int n, int area) { std::vector<Act> v; for (int a = 0; a < n; ++a) v.push_back({first + a, 1, area}); return v; };
  auto flush_run = [&]() {
    if (!rp.has) return;
    rp.has = false;
    run_end[rp.j] = sim.add(rp.stream, graph_acts(rp.first, rp.n, rp.area), {});  // (the run's event again, behind its graph updates)
    ++res.flushed;
  };
  long long i = 0;
  for (long long j = 0; i < K; ++j) {
    const RunSpans cur = group_run(sp.data(), K, i, run_max);
    ++res.runs;
    res.multi += cur.n > 1;
    const bool carry_kernel = defer && cur.n > 1;
    const bool carries = rp.has && carry_kernel && run_defers(cur, recent[0]);
    if (!carries) flush_run();
    const RunPlace place = run_place(j, carries, rstream);
    const int k = place.stream, o = k ^ 1;
    StepOrder ord;
    if (place.regular) ord = run_order(cur, recent, j);
    else ord.flush_own = ord.after_other = true;
    if ((ord.flush_own || cur.n > 1) && pend[k] >= 0) { sim.add(k, {{pend[k], 1, 0}}, {}); pend[k] = -1; }
    std::vector<int> extra;
    if (j >= 3) extra.push_back(run_end[j - 3]);
    if (ord.after_other) {
      if (pend[o] >= 0) { sim.add(o, {{pend[o], 1, 0}}, {}); pend[o] = -1; }
      if (sim.last[o] >= 0) extra.push_back(sim.last[o]);
    }
    if (cur.n > 1) {
      const int area = carries && two_areas ? rp.area ^ 1 : 0;
      std::vector<Act> acts;
      for (int a = 0; a < cur.n; ++a) acts.push_back({(int)i + a, 0, area});
      if (carries) {
        for (const Act& g : graph_acts(rp.first, rp.n, rp.area)) acts.push_back(g);  // the front of this launch
        ++res.carried;
      }
      run_end.push_back(sim.add(k, acts, extra));
      if (carry_kernel) { rp.has = true; rp.first = (int)i; rp.n = cur.n; rp.area = area; rp.stream = k; rp.j = j; }
      else run_end[j] = sim.add(k, graph_acts((int)i, cur.n, 0), {});
    } else {
      std::vector<Act> acts = {{(int)i, 0, 0}};
      if (pend[k] >= 0) acts.push_back({pend[k], 1, 0});  // the chained graph update of the last one-step run on this stream
      run_end.push_back(sim.add(k, acts, extra));
      pend[k] = (int)i;
    }
    recent[2] = recent[1]; recent[1] = recent[0]; recent[0] = cur;
    rstream[2] = rstream[1]; rstream[1] = rstream[0]; rstream[0] = k;
    i += cur.n;
  }
  flush_run();
  for (int k = 0; k < 2; ++k)
    if (pend[k] >= 0) sim.add(k, {{pend[k], 1, 0}}, {});
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
      for (const Act& s : sim.nodes[a].acts)
        for (const Act& t : sim.nodes[b].acts)
          if (s.step != t.step && acts_conflict(sp, s, t)) ++res.unordered;
    }
  // a step's graph update follows its own edge + node update
  // ... and every step has both, once each, the graph update behind the edge + node update and on the area that one wrote
  std::vector<int> at[2] = {std::vector<int>(K, -1), std::vector<int>(K, -1)}, area[2] = {std::vector<int>(K, -1), std::vector<int>(K, -1)};
  for (int a = 0; a < n; ++a)
    for (const Act& s : sim.nodes[a].acts) {
      if (at[s.kind][s.step] >= 0) ++res.unordered;
      at[s.kind][s.step] = a;
      area[s.kind][s.step] = s.area;
    }
  for (long long s = 0; s < K; ++s)
    if (at[0][s] < 0 || at[1][s] < 0 || !r[at[0][s]][at[1][s]] || area[0][s] != area[1][s]) ++res.unordered;
  return res;
}
static int fails = 0;
static Result expect_clean(const std::vector<StepSpans>& sp, int run_max, const char* what, int p0, int p1) {
  Result on;
  for (int defer = 0; defer < 2; ++defer) {
    const Result r = check(sp, run_max, defer, true);
    if (r.unordered) { std::printf("FAIL %s (%d, %d) run_max=%d defer=%d: unordered %d\n", what, p0, p1, run_max, defer, r.unordered); ++fails; }
    if (!defer && r.carried) { std::printf("FAIL %s (%d, %d): carried with the switch off\n", what, p0, p1); ++fails; }
    on = r;
  }
  return on;
}
int main() {
  const int maxima[3] = {2, 4, 8};
  for (int mi = 0; mi < 3; ++mi) {
    const int rm = maxima[mi];
    // rotating buffer sets, 1 .. 9 and 16 of them, every length
    for (int nsets = 1; nsets <= 16; nsets = nsets == 9 ? 16 : nsets + 1)
      for (int K = 1; K <= 40; ++K) {
        std::vector<StepSpans> sp;
        for (int i = 0; i < K; ++i) sp.push_back(spans_of(i % nsets, i % nsets, i % nsets));
        const Result r = expect_clean(sp, rm, "rotating sets", nsets, K);
        // as many sets as a run has steps: every run after the first carries, and one flush ends the call (or precedes the single steps)
        if (nsets == rm && r.multi >= 1 && (r.carried != r.multi - 1 || r.flushed != 1)) {
          std::printf("FAIL rotation over %d sets, K=%d: %d runs of several, %d carried, %d flushed\n", nsets, K, r.multi, r.carried, r.flushed);
          ++fails;
        }
      }
    for (int K = 1; K <= 40; ++K) {
      std::vector<StepSpans> a, a2, b, b2, c, c2, d;
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
      std::vector<StepSpans> sp;
      for (int i = 0; i < K; ++i) {
        const int mode = rnd(8);
        if (mode == 0 && i > 0) sp.push_back(spans_chain(rnd(m), rnd(m), rnd(m)));
        else if (mode == 1) sp.push_back(spans_of(rnd(m), rnd(m), rnd(m), 32));
        else if (mode <= 4) sp.push_back(spans_of(i % period, i % period, i % period));  // stretches of a rotation, so that runs form
        else sp.push_back(spans_of(20 + i, 20 + i, i % period));
      }
      expect_clean(sp, rm, "random", trial, K);
    }
  }
  // known loops at run maximum 8 on 8 sets: 20 steps = 8 + 8 + 4, two carried and one flush; 12 steps = 8 + a tail of 4, carried; 9 steps =
  // a run and one step: the run's graph updates are flushed before the step
  {
    std::vector<StepSpans> a, b, c;
    for (int i = 0; i < 20; ++i) a.push_back(spans_of(i % 8, i % 8, i % 8));
    for (int i = 0; i < 12; ++i) b.push_back(spans_of(i % 8, i % 8, i % 8));
    for (int i = 0; i < 9; ++i) c.push_back(spans_of(i % 8, i % 8, i % 8));
    const Result ra = check(a, 8, true, true), rb = check(b, 8, true, true), rc = check(c, 8, true, true);
    if (ra.runs != 3 || ra.carried != 2 || ra.flushed != 1 || rb.runs != 2 || rb.carried != 1 || rb.flushed != 1 || rc.runs != 2 || rc.carried != 0 || rc.flushed != 1 ||
        ra.unordered || rb.unordered || rc.unordered) {
      std::printf("FAIL known loops: %d/%d/%d %d/%d/%d %d/%d/%d\n", ra.runs, ra.carried, ra.flushed, rb.runs, rb.carried, rb.flushed, rc.runs, rc.carried, rc.flushed);
      ++fails;
    }
    // the negative control: with ONE partial-row area the carried graph updates read the rows the carrying run's tiles write
    if (!check(a, 8, true, false).unordered || !check(b, 8, true, false).unordered) { std::printf("FAIL: one partial-row area was not flagged\n"); ++fails; }
    if (check(c, 8, true, false).unordered) { std::printf("FAIL: one partial-row area flagged where nothing is carried\n"); ++fails; }
  }
  if (fails) return 1;
  std::printf("deferred ok\n");
  return 0;
}
"""


def test_carrying_runs_order_every_conflicting_pair(tmp_path):
    src = tmp_path / "deferred.cpp"
    src.write_text(SCHEDULE)
    exe = tmp_path / "deferred"
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "deferred ok" in out.stdout


def _resources(stderr):
    """kernel -> {sgpr, vgpr, scratch} from -Rpass-analysis=kernel-resource-usage remarks"""
    out = {}
    for blk in re.split(r"remark: Function Name: ", stderr)[1:]:
        name = blk.split()[0]
        g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))
        out[name] = dict(sgpr=g("TotalSGPRs"), vgpr=g("VGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"))
    return out


def _key(de, dn, dg, oe, on):
    return "".join(f"Li{v}E" for v in (de, dn, dg, oe, on, 2))


# the width sets and graph-count forms with a carrying kernel (gnx_narrow.hip: GNX_NARROW_CARRY_DIMS), as the mangled names spell them
CARRY = {(_key(*d), g) for d in ((10, 5, 0, 3, 4), (3, 4, 5, 3, 4), (10, 5, 3, 3, 4), (0, 2, 0, 2, 2), (4, 3, 2, 3, 4)) for g in "01"}


def test_carrying_kernels_resource_audit():
    """Every k_block_wave_carry instantiation, compiled as build.py compiles gnx_narrow.hip: no scratch, at most 80 scalar registers (the
    eighth workgroup per CU), no more vector registers than the chained kernel of the same set and form; exactly the listed instantiations,
    fp32 rows only."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    cmd = [HIPCC, "-x", "hip", "-c", "--cuda-device-only", "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, os.path.join(CSRC, "gnx_narrow.hip")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stderr[-3000:]
    res = _resources(p.stderr)
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
