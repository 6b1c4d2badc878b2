// Host-side hazard rule of gnx_block_forward_steps' two-stream schedule (gnx_forward.hip): may two steps of the loop run at the same time?
// Conservative and by address range only: step i's writes (ef_out, nf_out, gf_out, workspace) must not overlap anything step j reads or
// writes (ef, nf, gf, ef_out, nf_out, gf_out, workspace), and the same the other way round.  The weights are read by every step and
// written by none.  Plain C++ (no HIP): tests/test_steps_hazard_cpu.py compiles it on its own.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gnx {

struct ByteSpan {  // [lo, hi); empty when lo == hi
  uintptr_t lo = 0, hi = 0;
};

inline ByteSpan byte_span(const void* p, size_t bytes) {
  ByteSpan s;
  if (p && bytes) { s.lo = reinterpret_cast<uintptr_t>(p); s.hi = s.lo + bytes; }
  return s;
}

inline bool spans_overlap(ByteSpan a, ByteSpan b) { return a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi; }

struct StepSpans {
  ByteSpan rd[3];  // ef, nf, gf
  ByteSpan wr[4];  // ef_out, nf_out, gf_out, workspace
};

// The spans of one step of R replicas: rows[t] rows (E, N, G) of the inputs in_w[t] wide and of the outputs out_w[t] wide, elem bytes per
// feature (4: fp32, 2: bf16), and the part of the workspace the block's kernels use (ws_extent: the workspace query's figure for this call).
inline StepSpans step_spans_of(const void* const in[3], const void* const out[3], const void* ws, size_t ws_bytes, const long long rows[3],
                               const int in_w[3], const int out_w[3], long long R, size_t elem, size_t ws_extent) {
  const size_t f = elem * (size_t)R;
  StepSpans sp;
  for (int t = 0; t < 3; ++t) {
    sp.rd[t] = byte_span(in[t], f * (size_t)rows[t] * (size_t)in_w[t]);
    sp.wr[t] = byte_span(out[t], f * (size_t)rows[t] * (size_t)out_w[t]);
  }
  sp.wr[3] = byte_span(ws, ws_bytes < ws_extent ? ws_bytes : ws_extent);
  return sp;
}

// true: the two steps must not be in flight together
inline bool steps_conflict(const StepSpans& x, const StepSpans& y) {
  for (const ByteSpan& w : x.wr) {
    for (const ByteSpan& r : y.rd) if (spans_overlap(w, r)) return true;
    for (const ByteSpan& v : y.wr) if (spans_overlap(w, v)) return true;
  }
  for (const ByteSpan& w : y.wr)
    for (const ByteSpan& r : x.rd) if (spans_overlap(w, r)) return true;
  return false;
}

// The two-stream schedule of gnx_block_forward_steps: step i runs on stream i & 1 (even steps on the caller's stream, odd steps on the side
// stream); the chained graph update of step i rides at the front of step i + 2's launch (the next on its stream); and step i's launch waits
// for step i - 3's launch to end (an event per step).  That wait is what bounds the streams' skew: launches i and j can then run together
// only when |i - j| == 1, so step i (its launch and, two launches later, its graph update) is in flight together with steps i +- 1 and
// i +- 3 only, whatever the order in which the two streams (or a captured graph's two branches) make progress.  The rest is this:
struct StepOrder {
  bool flush_own = false;    // step i - 2's pending graph update runs as its own launch before step i's (it must not ride in step i's)
  bool after_other = false;  // step i waits for everything issued on the other stream, step i - 1's pending graph update flushed first
};
// recent[d - 1]: the spans of step i - d, for d = 1 .. min(i, 3)
inline StepOrder step_order(const StepSpans& cur, const StepSpans* recent, long long i) {
  StepOrder o;
  o.flush_own = i >= 2 && steps_conflict(cur, recent[1]);
  o.after_other = (i >= 1 && steps_conflict(cur, recent[0])) || (i >= 3 && steps_conflict(cur, recent[2]));
  return o;
}

// ---- runs: neighbouring steps that share ONE launch (k_block_wave_run: gridDim.y = the run's steps) ----
// A run is consecutive steps no two of which conflict: inside a launch nothing orders one slot's workgroups against another's.  The window
// grows greedily from the run's first step; it becomes a run if it is FULL — run_max steps (<= kRunMax) — or if the end of the loop cut it
// and it still has kRunTailMin steps.  Else the step is a run of its own: what a shared launch gains grows with its length
// (profiles/steps_runs_c2.md: eight steps per launch gain 6 % on the 1M-edge graph, four nothing, two lose 5 % against single steps on two
// streams), so a window that a CONFLICT cuts short (fewer buffer sets in rotation than run_max, a shared workspace, dims -> dims) keeps the
// schedule of single steps, which overlaps them on the two streams, and so does a short rest of the loop.
// The unit of the two-stream schedule above is the run: read "step" as "run" throughout — run j on stream j & 1, behind run j - 3's event,
// ordered against runs j - 1, j - 2, j - 3 by run_order.  A run of ONE step is issued exactly as a step was (chained, its graph update pending
// until the next launch on its stream); a run of several is two launches, its graph updates right behind its block launch, nothing pending.
constexpr int kRunMax = 8;      // slots of the kernel-argument table
constexpr int kRunTailMin = 4;  // the shortest run that is not full: the last steps of a loop

struct RunSpans {
  int n = 0;
  StepSpans step[kRunMax];
};

inline bool run_conflicts_step(const RunSpans& r, const StepSpans& s) {
  for (int a = 0; a < r.n; ++a)
    if (steps_conflict(r.step[a], s)) return true;
  return false;
}

// two runs conflict if any pair of their steps does
inline bool runs_conflict(const RunSpans& x, const RunSpans& y) {
  for (int b = 0; b < y.n; ++b)
    if (run_conflicts_step(x, y.step[b])) return true;
  return false;
}

// Greedy growth of the window: does the next step join?  (The caller also asks that the step is valid and that the run form takes the call.)
inline bool run_takes(const RunSpans& run, const StepSpans& next, int run_max) {
  return run.n >= 1 && run.n < run_max && run.n < kRunMax && !run_conflicts_step(run, next);
}

// a window of n steps that begins at step `first` of n_steps: is it a run?
inline bool window_is_run(int n, long long first, long long n_steps, int run_max) {
  return n >= 2 && (n == run_max || (first + n == n_steps && n >= kRunTailMin));
}

// the run that starts at step `first` of spans[0 .. n_steps)
inline RunSpans group_run(const StepSpans* spans, long long n_steps, long long first, int run_max) {
  RunSpans run;
  if (first >= n_steps) return run;
  run.step[run.n++] = spans[first];
  while (first + run.n < n_steps && run_takes(run, spans[first + run.n], run_max)) { run.step[run.n] = spans[first + run.n]; ++run.n; }
  if (!window_is_run(run.n, first, n_steps, run_max)) run.n = 1;
  return run;
}

// step_order on runs.  recent[d - 1]: run j - d, for d = 1 .. min(j, 3).  With runs of one step these are step_order's decisions.
inline StepOrder run_order(const RunSpans& cur, const RunSpans* recent, long long j) {
  StepOrder o;
  o.flush_own = j >= 2 && runs_conflict(cur, recent[1]);
  o.after_other = (j >= 1 && runs_conflict(cur, recent[0])) || (j >= 3 && runs_conflict(cur, recent[2]));
  return o;
}

// ---- a run that carries the graph updates of the run before it (k_block_wave_carry: front workgroups of ITS block launch) ----
// Run `prev` is issued as its block launch alone and its graph updates wait; if the next run conflicts with it — so that it would be ordered
// behind it anyway — and every conflict is of a kind that stream order plus two partial-row areas resolves, the next run goes on prev's
// stream and its launch carries them.  What then runs at the same time is prev's graph updates (they read prev's gf and the partial rows
// in prev's workspaces, they write prev's gf_out) and cur's edge + node updates (they read cur's inputs, they write cur's ef_out, nf_out
// and the partial rows in cur's workspaces).  Between a step x of cur and a step y of prev these overlaps are harmless:
//   x's ef_out / nf_out with y's ef_out / nf_out — write after write, ordered by the two block launches;
//   x's gf_out with y's gf_out — y's update runs in cur's launch, x's in a later one;
//   x's workspace with y's, if they are THE SAME workspace — cur writes the partial-row area that prev did not (steps_schedule).
// Every other overlap that makes the two steps conflict (steps_conflict) keeps today's order: prev's graph updates as a launch of their
// own, then cur.  Among them the ones that would race — cur reading what prev's update writes (dims -> dims: gf' fed back), cur's ef_out /
// nf_out over prev's gf, gf_out or workspace, workspaces that overlap without being the same — and, conservatively, all the rest.
inline bool spans_identical(ByteSpan a, ByteSpan b) { return a.lo == b.lo && a.hi == b.hi; }

// may step x (of the later run) be in a launch whose front finishes step y's graph update?  (No overlap at all: yes.)
inline bool step_defers(const StepSpans& x, const StepSpans& y) {
  for (int t = 0; t < 4; ++t) {
    for (const ByteSpan& r : y.rd) if (spans_overlap(x.wr[t], r)) return false;
    for (int u = 0; u < 4; ++u) {
      if (!spans_overlap(x.wr[t], y.wr[u])) continue;
      const bool rows = t < 2 && u < 2, gf_out = t == 2 && u == 2, ws = t == 3 && u == 3 && spans_identical(x.wr[3], y.wr[3]);
      if (!rows && !gf_out && !ws) return false;
    }
  }
  for (const ByteSpan& w : y.wr)
    for (const ByteSpan& r : x.rd) if (spans_overlap(w, r)) return false;
  return true;
}

// does run `cur` carry the graph updates of run `prev`, the run right before it?  (The caller also asks that the kernel exists for the call
// and that the second partial-row area fits.)
inline bool run_defers(const RunSpans& cur, const RunSpans& prev) {
  if (cur.n < 2 || prev.n < 2 || !runs_conflict(cur, prev)) return false;
  for (int a = 0; a < cur.n; ++a)
    for (int b = 0; b < prev.n; ++b)
      if (!step_defers(cur.step[a], prev.step[b])) return false;
  return true;
}

// The two-stream schedule with carrying runs.  A carrying run stays on the stream of the run it follows, so the runs no longer alternate
// between the streams, which is what run_order and the wait for run j - 3 assume.  A run is REGULAR if it and the three before it all sit
// on the stream of their parity (j & 1): then the schedule is today's, decision for decision.  Any other run (a carrying run, or one with a
// carrying run among the three before it) is ordered behind EVERYTHING issued before it on both streams — it costs nothing where it
// happens: a carrying run conflicts with its predecessor and waits for it anyway.  With that, when launch j starts every launch up to
// j - 4 has ended, as before: an irregular run waits for all of them; a regular one waits for run j - 3 on the other stream and follows
// run j - 2 on its own, and every older run is in front of one of the two in stream order.
struct RunPlace {
  int stream = 0;        // the stream run j is issued on
  bool regular = true;   // run_order's decisions hold; else the run waits for everything issued so far
};
// recent_stream[d - 1]: the stream of run j - d, d = 1 .. min(j, 3); carries: run j carries run j - 1's graph updates
inline RunPlace run_place(long long j, bool carries, const int* recent_stream) {
  RunPlace p;
  p.stream = carries ? recent_stream[0] : (int)(j & 1);
  p.regular = p.stream == (int)(j & 1);
  for (int d = 1; d <= 3 && d <= j; ++d) p.regular = p.regular && recent_stream[d - 1] == (int)((j - d) & 1);
  return p;
}

}  // namespace gnx
