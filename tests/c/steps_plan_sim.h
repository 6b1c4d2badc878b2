// Happens-before simulator of gnx_block_forward_steps' schedule, shared by tests/test_steps_{hazard,runs,deferred}_cpu.py.  It drives the
// library's own planner (gnx_step_hazard.h: StepsPlanner — the code steps_schedule issues from) over a loop of steps given as spans, and
// builds the graph of what its operations put in flight: launches are nodes on two streams (stream order), plus the waits the plan adds
// through the ring of four run events and the fork / join events.  An ACTIVITY is a step's edge + node update (kind 0: reads ef, nf, gf;
// writes ef_out, nf_out and the partial rows in one area of its workspace) or its graph update (kind 1: reads gf and those partial rows;
// writes gf_out), wherever the plan put it: behind its own block launch, at the front of the next one-step launch on its stream, at the
// front of the next run's block launch, or in a flush.  Every two activities of different steps whose bytes conflict must be ordered,
// whatever the streams' relative progress.  Plain C++, no HIP.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gnx_step_hazard.h"

namespace sim {
using namespace gnx;

static char mem[1 << 20];
// A buffer set: three 64-byte inputs, three 64-byte outputs.  A workspace is 64 bytes: area B (the head of the agg area) its bytes [0, 16),
// area A (the block's own partial rows) its bytes [32, 48).  shift 32: a workspace that overlaps its neighbour without being the same one
// (its area B is the neighbour's area A).
inline StepSpans spans_of(int in_set, int out_set, int ws_set, int shift = 0) {
  StepSpans s;
  for (int t = 0; t < 3; ++t) s.rd[t] = byte_span(mem + in_set * 1024 + t * 64, 64);
  for (int t = 0; t < 3; ++t) s.wr[t] = byte_span(mem + out_set * 1024 + 512 + t * 64, 64);
  s.wr[3] = byte_span(mem + 200 * 1024 + ws_set * 64 + shift, 64);
  return s;
}
// dims -> dims: the inputs of a step are the outputs of src_out_set
inline StepSpans spans_chain(int src_out_set, int out_set, int ws_set) {
  StepSpans s = spans_of(0, out_set, ws_set);
  for (int t = 0; t < 3; ++t) s.rd[t] = byte_span(mem + src_out_set * 1024 + 512 + t * 64, 64);
  return s;
}
using Loop = std::vector<StepSpans>;
inline Loop rotation(int K, int nsets) {
  Loop sp;
  for (int i = 0; i < K; ++i) sp.push_back(spans_of(i % nsets, i % nsets, i % nsets));
  return sp;
}

struct Act { int step, kind, area; };
inline ByteSpan part(const StepSpans& s, int area) {
  ByteSpan p;
  p.lo = s.wr[3].lo + (area ? 0 : 32);
  p.hi = p.lo + 16;
  return p;
}
inline bool acts_conflict(const Loop& sp, const Act& a, const Act& b) {
  struct Bytes { std::vector<ByteSpan> rd, wr; };
  auto bytes_of = [&](const Act& c) {
    const StepSpans& s = sp[c.step];
    return c.kind == 0 ? Bytes{{s.rd[0], s.rd[1], s.rd[2]}, {s.wr[0], s.wr[1], part(s, c.area)}} : Bytes{{s.rd[2], part(s, c.area)}, {s.wr[2]}};
  };
  const Bytes x = bytes_of(a), y = bytes_of(b);
  for (const ByteSpan& w : x.wr) {
    for (const ByteSpan& r : y.rd) if (spans_overlap(w, r)) return true;
    for (const ByteSpan& v : y.wr) if (spans_overlap(w, v)) return true;
  }
  for (const ByteSpan& w : y.wr)
    for (const ByteSpan& r : x.rd) if (spans_overlap(w, r)) return true;
  return false;
}

struct Config {
  int run_max = 8;
  bool two = true;     // two streams
  bool defer = true;   // the carry switch; the carrying kernel exists for every run
  bool chain = true;   // a one-step launch leaves its graph update pending (else that update is inside its own launch)
  // mutations of the plan, the negative controls:
  bool drop_wait3 = false;  // the wait for run j - 3 is not issued
  bool one_area = false;    // every run writes partial-row area A
};
struct Result {
  int unordered = 0;        // conflicting activities that nothing orders; a step without exactly one of each, in order, on one area
  int unordered_steps = 0;  // ... by the rule for whole steps (steps_conflict), which holds where nothing is carried
  int in_run = 0;           // conflicting steps inside one run
  int differs = 0;          // the runs are not the greedy windows; at a run maximum of 1, the plan is not the single-step schedule
  int runs = 0, multi = 0, longest = 0, carried = 0, flushed = 0, ops_max = 0;
};

inline Result check(const Loop& sp, const Config& cf) {
  const long long K = (long long)sp.size();
  Result res;
  std::vector<std::vector<Act>> nodes;
  std::vector<std::vector<int>> deps;  // edges into a node
  int last[2] = {-1, -1}, event[4] = {-1, -1, -1, -1};
  std::vector<int> extra[2];  // what a stream has been made to wait for: edges into its next node
  auto add = [&](int stream, std::vector<Act> acts) {
    std::vector<int> d;
    d.swap(extra[stream]);
    if (last[stream] >= 0) d.push_back(last[stream]);
    nodes.push_back(acts);
    deps.push_back(d);
    last[stream] = (int)nodes.size() - 1;
  };
  auto wait = [&](int stream, int node) { if (node >= 0) extra[stream].push_back(node); };
  auto acts_of = [](long long first, int n, int kind, int area) {
    std::vector<Act> v;
    for (int a = 0; a < n; ++a) v.push_back({(int)first + a, kind, area});
    return v;
  };
  auto apply = [&](StepsPlan pl) {
    if (pl.n > res.ops_max) res.ops_max = pl.n;
    for (int z = 0; z < pl.n; ++z) {
      StepsOp op = pl.op[z];
      if (cf.one_area) op.area = 0;
      const int k = op.stream;
      switch (op.kind) {
        case kOpFlushRun:
          add(k, acts_of(op.step, op.n, 1, op.area));
          event[op.run & 3] = last[k];
          ++res.flushed;
          break;
        case kOpFlushStep: add(k, {{(int)op.step, 1, 0}}); break;
        case kOpWaitRun: if (!cf.drop_wait3) wait(k, event[op.run & 3]); break;
        case kOpBehindOther: wait(k, last[k ^ 1]); break;
        case kOpLaunchStep: {
          std::vector<Act> acts = {{(int)op.step, 0, 0}};
          if (op.ride >= 0) acts.push_back({(int)op.ride, 1, 0});
          if (!cf.chain) acts.push_back({(int)op.step, 1, 0});
          add(k, acts);
          break;
        }
        case kOpLaunchRun: {
          std::vector<Act> acts = acts_of(op.step, op.n, 0, op.area);
          if (op.form == kRunCarry) {
            for (const Act& g : acts_of(op.ride, op.ride_n, 1, cf.one_area ? 0 : op.area ^ 1)) acts.push_back(g);
            ++res.carried;
          }
          add(k, acts);
          if (op.form == kRunWhole) add(k, acts_of(op.step, op.n, 1, op.area));
          break;
        }
        case kOpRecordRun: event[op.run & 3] = last[k]; break;
        case kOpJoin: wait(0, last[1]); break;
      }
    }
  };
  StepsPlanner planner(cf.two, cf.defer, cf.run_max, K);
  bool prev_behind = false;
  while (planner.first < K) {
    const long long i = planner.first, j = planner.j;
    const RunSpans cur = group_run(sp.data(), K, i, cf.run_max);
    if (cur.n < 1 || cur.n > cf.run_max || cur.n > kRunMax) { ++res.differs; break; }
    for (int a = 0; a < cur.n; ++a) {
      for (int t = 0; t < 4; ++t) if (!spans_identical(cur.step[a].wr[t], sp[i + a].wr[t])) ++res.differs;  // the run is steps i .. i + n - 1, in order
      for (int b = a + 1; b < cur.n; ++b) if (steps_conflict(cur.step[a], cur.step[b])) ++res.in_run;
    }
    // a run is the greedy window if it is full or the end of the loop cut it at four steps or more; else one step — restated here, and
    // the planner's own window functions agree
    {
      int len = 1;
      for (; len < cf.run_max && i + len < K; ++len) {
        bool clash = false;
        for (int a = 0; a < len; ++a) clash = clash || steps_conflict(sp[i + a], sp[i + len]);
        if (clash) break;
      }
      const bool is_run = len >= 2 && (len == cf.run_max || (i + len == K && len >= 4));
      if (cur.n != (is_run ? len : 1) || planner.is_run(len) != is_run) ++res.differs;
      RunSpans win;
      for (win.n = 0; win.n < len; ++win.n) win.step[win.n] = sp[i + win.n];
      if (i + len < K && planner.takes(win, sp[i + len])) ++res.differs;
    }
    ++res.runs;
    res.multi += cur.n > 1;
    if (cur.n > res.longest) res.longest = cur.n;
    const StepsPlan pl = planner.next(cur, planner.may_defer(cur), false);
    if (cf.run_max == 1) {
      // a run maximum of 1 is the schedule of single steps: step i is run i on stream i & 1 (one stream: 0); its pending graph update
      // is flushed ahead of step i + 2 exactly if the two conflict, and step i goes behind the other stream exactly if it conflicts with
      // step i - 1 or i - 3; no operation of a run of several steps
      auto clash = [&](long long d) { return i >= d && steps_conflict(sp[i], sp[i - d]); };
      // (its pending update is gone already where step i - 1 went behind the other stream, which flushed it)
      bool own = false, other = false, behind = false, waits = false, alien = cur.n != 1 || j != i;
      for (int z = 0; z < pl.n; ++z) {
        const StepsOp& op = pl.op[z];
        const int k = cf.two ? (int)(i & 1) : 0;
        if (op.kind == kOpFlushStep) (op.stream == k ? own : other) = true;
        else if (op.kind == kOpBehindOther) behind = true;
        else if (op.kind == kOpWaitRun) waits = op.run == i - 3;
        else if (op.kind != kOpLaunchStep && op.kind != kOpRecordRun) alien = true;
        if (op.kind != kOpFlushStep && op.stream != k) alien = true;
      }
      if (alien) ++res.differs;
      if (cf.two && (own != (cf.chain && clash(2) && !prev_behind) || behind != (clash(1) || clash(3)) || other != (behind && cf.chain && i >= 1) || waits != (i >= 3))) ++res.differs;
      if (!cf.two && (own != (cf.chain && clash(1)) || other || behind || waits)) ++res.differs;
      prev_behind = behind;
    }
    apply(pl);
    planner.done(pl, cur, pl.n, cf.chain);
  }
  apply(planner.close());

  const int n = (int)nodes.size();
  std::vector<std::vector<char>> r(n, std::vector<char>(n, 0));  // r[a][b]: a ends before b starts
  for (int b = 0; b < n; ++b)
    for (int a : deps[b]) {
      r[a][b] = 1;
      for (int x = 0; x < n; ++x) if (r[x][a]) r[x][b] = 1;
    }
  for (int a = 0; a < n; ++a)
    for (int b = a; b < n; ++b) {
      if (a != b && (r[a][b] || r[b][a])) continue;
      for (const Act& s : nodes[a])
        for (const Act& t : nodes[b]) {
          if (s.step == t.step) continue;
          if (acts_conflict(sp, s, t)) ++res.unordered;
          if (steps_conflict(sp[s.step], sp[t.step])) ++res.unordered_steps;
        }
    }
  // every step has both activities, once each, the graph update behind the edge + node update (or in its launch: a whole step) and on
  // the area that one wrote
  std::vector<int> at[2] = {std::vector<int>(K, -1), std::vector<int>(K, -1)}, area[2] = {std::vector<int>(K, -1), std::vector<int>(K, -1)};
  for (int a = 0; a < n; ++a)
    for (const Act& s : nodes[a]) {
      if (at[s.kind][s.step] >= 0) ++res.unordered;
      at[s.kind][s.step] = a;
      area[s.kind][s.step] = s.area;
    }
  for (long long s = 0; s < K; ++s) {
    const bool whole = !cf.chain && at[0][s] >= 0 && at[0][s] == at[1][s];
    if (at[0][s] < 0 || at[1][s] < 0 || !(whole || r[at[0][s]][at[1][s]]) || area[0][s] != area[1][s]) ++res.unordered;
  }
  return res;
}

}  // namespace sim
