// The host-side schedule of gnx_block_forward_steps (gnx_forward.hip: steps_schedule issues what is planned here).  Plain C++, no HIP and no
// heap: tests/c/steps_plan_sim.h compiles this header on its own and the CPU tests check the operations StepsPlanner returns.
//
// Hazard rule, conservative and by address range only: two steps may be in flight together only if nothing one writes (ef_out, nf_out,
// gf_out, workspace) overlaps anything the other reads or writes (ef, nf, gf, ef_out, nf_out, gf_out, workspace).  The weights are read by
// every step and written by none.
//
// The schedule.  Its unit is the RUN: run_max neighbouring steps no two of which conflict, or the last four or more of the loop, issued as
// one block launch with a slot per step; any other step is a run of its own, a chained step whose graph update stays pending and rides at
// the front of the next one-step launch on its stream.  On two streams run j goes to stream j & 1 (even: the caller's) and waits for the
// event of run j - 3, so that only runs up to three apart are in flight together; conflicts among those are ordered by run_order.  A run
// of several steps whose graph updates the next run can carry (run_defers) is its block launch alone; the carrying run stays on its stream
// and writes the other partial-row area (run_place orders it, and the three runs after it, behind everything issued so far).  What is not
// carried is flushed before anything of the next run is issued.  StepsPlanner at the end of this header composes these decisions.
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

// Two streams: run j on stream j & 1; a one-step run's chained graph update rides at the front of run j + 2's launch if that is one step
// too (the next on its stream); and run j's launch waits for run j - 3's to end (an event per run).  That wait is what bounds the streams'
// skew: launches i and j can then run together only when |i - j| == 1, so run j (its launch and, two launches later, a pending graph
// update) is in flight together with runs j +- 1 and j +- 3 only, whatever the order in which the two streams (or a captured graph's two
// branches) make progress.  The rest is this:
struct StepOrder {
  bool flush_own = false;    // run j - 2's pending graph update runs as its own launch before run j's (it must not ride in run j's)
  bool after_other = false;  // run j waits for everything issued on the other stream, run j - 1's pending graph update flushed first
};

// ---- runs: neighbouring steps that share ONE launch (k_block_wave_run: gridDim.y = the run's steps) ----
// A run is consecutive steps no two of which conflict: inside a launch nothing orders one slot's workgroups against another's.  The window
// grows greedily from the run's first step; it becomes a run if it is FULL — run_max steps (<= kRunMax) — or if the end of the loop cut it
// and it still has kRunTailMin steps.  Else the step is a run of its own: what a shared launch gains grows with its length
// (profiles/steps_runs_c2.md: eight steps per launch gain 6 % on the 1M-edge graph, four nothing, two lose 5 % against single steps on two
// streams), so a window that a CONFLICT cuts short (fewer buffer sets in rotation than run_max, a shared workspace, dims -> dims) keeps the
// schedule of single steps, which overlaps them on the two streams, and so does a short rest of the loop.
// A run of several steps that no run carries is two launches, its graph updates right behind its block launch, nothing pending.
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

// recent[d - 1]: run j - d, for d = 1 .. min(j, 3).  With runs of one step these are the decisions of the schedule of single steps.
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
//   x's workspace with y's, if they are THE SAME workspace — cur writes the partial-row area that prev did not (StepsPlanner).
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

// ---- the schedule composed: one run in, its operations out ----
// An operation is one thing steps_schedule issues.  `stream` is the stream it goes to (0: the caller's, 1: the side stream); run r's event
// is the r & 3rd of the ring of four.
enum StepsOpKind : unsigned char {
  kOpFlushRun,     // the graph updates of the deferred run `run` (steps step .. step + n - 1, partial rows in `area`), then its event again
  kOpFlushStep,    // the pending graph update of `step` as a launch of its own
  kOpWaitRun,      // wait for the event of run `run` (j - 3)
  kOpBehindOther,  // behind everything on the other stream: record fork (from stream 0) or join (from stream 1) there, wait here
  kOpLaunchStep,   // `step` as a chained step; `ride`: the pending step whose graph update rides at its front, or -1
  kOpLaunchRun,    // steps step .. step + n - 1 in one launch of form `form`, their partial rows in `area`
  kOpRecordRun,    // record the event of run `run`
  kOpJoin,         // the end of the call: record join on the side stream, the caller's stream waits for it
};
enum RunForm : unsigned char {
  kRunWhole,  // block launch and graph updates right behind it
  kRunBlock,  // the block launch alone: the graph updates are deferred
  kRunCarry,  // ... and its front finishes the graph updates of the deferred run, steps ride .. ride + ride_n - 1 (area ^ 1)
};
struct StepsOp {
  StepsOpKind kind = kOpJoin;
  unsigned char stream = 0, form = kRunWhole, area = 0;
  int n = 1, ride_n = 0;
  long long step = -1, ride = -1, run = 0;
};
struct StepsPlan {
  static constexpr int kMax = 8;  // a run: at most seven (two flushes, two waits and the flush between them, a launch, an event)
  int n = 0;
  StepsOp op[kMax];
  StepsOp& add(StepsOpKind kind, int stream, long long step = -1, int steps = 1, long long run = 0, int area = 0) {
    StepsOp& o = op[n++];
    o.kind = kind, o.stream = (unsigned char)stream, o.step = step, o.n = steps, o.run = run, o.area = (unsigned char)area;
    return o;
  }
};

// The loop's state that is no HIP object.  Per run: grow the window (takes, is_run; the caller validates its steps), next() for the run's
// operations in issue order, done() with how many of them were issued — all of them, or the ones before the one that failed — then, once,
// close() for the flushes and the join that end the call on every path.
struct StepsPlanner {
  // the call
  bool two = false;        // two streams, else every run on the caller's
  bool can_carry = false;  // a run may carry its predecessor's graph updates at all (two streams, fp32 rows, area B fits, the switch on)
  int run_max = 1;
  long long n_steps = 0;
  // the loop
  long long j = 0, first = 0;      // the next run and its first step
  RunSpans recent[3];              // runs j - 1, j - 2, j - 3
  int rstream[3] = {0, 0, 0};      // ... and the streams they went to
  long long pend[2] = {-1, -1};    // the one-step run whose graph update is pending on each stream
  struct Deferred {                // the last run of several steps while its graph updates wait (run j - 1, never older)
    bool has = false;
    int stream = 0, n = 0, area = 0;
    long long step = 0, run = 0;
    void flush(StepsPlan& pl) const { pl.add(kOpFlushRun, stream, step, n, run, area); }
  } held;

  StepsPlanner(bool two_streams, bool carry, int max, long long steps) : two(two_streams), can_carry(two_streams && carry), run_max(max), n_steps(steps) {}

  bool takes(const RunSpans& win, const StepSpans& next_step) const { return run_takes(win, next_step, run_max); }
  bool is_run(int n) const { return window_is_run(n, first, n_steps, run_max); }
  // the caller then asks whether the carrying kernel exists for the call
  bool may_defer(const RunSpans& cur) const { return can_carry && cur.n > 1; }

  // carry_kernel: may_defer(cur) and the kernel exists.  aliases_pending (one stream): the step's workspace or gf_out is, as a pointer, the
  // one of pend[0] — not the spans' business: a step with a bad workspace has an empty span and must still find nothing pending.
  StepsPlan next(const RunSpans& cur, bool carry_kernel, bool aliases_pending) const {
    StepsPlan pl;
    // does this run carry the deferred graph updates of the run before it?  Else they are flushed first, as if never deferred.
    const bool carries = held.has && carry_kernel && run_defers(cur, recent[0]);
    if (held.has && !carries) held.flush(pl);
    const RunPlace place = two ? run_place(j, carries, rstream) : RunPlace{};
    const int k = place.stream, o = k ^ 1;
    StepOrder ord;
    // one stream: a run whose buffers overlap its predecessor's cannot start before that one's graph update has run
    if (!two) ord.flush_own = pend[0] >= 0 && (aliases_pending || runs_conflict(cur, recent[0]));
    else if (place.regular) ord = run_order(cur, recent, j);
    else ord.flush_own = ord.after_other = true;  // (run_place: behind everything issued so far)
    // a launch of several steps has no front for a pending update to ride in
    const bool flush_own = pend[k] >= 0 && (ord.flush_own || cur.n > 1);
    if (flush_own) pl.add(kOpFlushStep, k, pend[k]);
    if (two && j >= 3) pl.add(kOpWaitRun, k, -1, 1, j - 3);
    if (ord.after_other) {
      if (pend[o] >= 0) pl.add(kOpFlushStep, o, pend[o]);
      pl.add(kOpBehindOther, k);
    }
    StepsOp& l = pl.add(cur.n > 1 ? kOpLaunchRun : kOpLaunchStep, k, first, cur.n, j, carries ? held.area ^ 1 : 0);
    if (cur.n == 1) l.ride = flush_own ? -1 : pend[k];
    else if (carries) l.form = kRunCarry, l.ride = held.step, l.ride_n = held.n;
    else if (carry_kernel) l.form = kRunBlock;
    // (event j & 3 was last recorded for run j - 4, and the wait on that record — run j - 1's — is already planned)
    if (two) pl.add(kOpRecordRun, k, -1, 1, j);
    return pl;
  }

  // issued == pl.n: the run is out.  Else operation `issued` failed and nothing after it was issued: a flush that fails is not pending any
  // more, a carrying launch that fails carried nothing, a step that fails leaves what was pending as it was.  took: the one-step launch
  // left its graph update pending (known only once it returns).
  void done(const StepsPlan& pl, const RunSpans& cur, int issued, bool took) {
    for (int z = 0; z < pl.n && z <= issued; ++z) {
      const StepsOp& op = pl.op[z];
      const bool ok = z < issued;
      if (op.kind == kOpFlushRun) held.has = false;
      if (op.kind == kOpFlushStep) pend[op.stream] = -1;
      if (op.kind == kOpLaunchStep && ok) pend[op.stream] = took ? op.step : -1;
      if (op.kind == kOpLaunchRun) {
        if (op.form == kRunCarry) held.has = false;
        if (ok && op.form != kRunWhole) held = Deferred{true, op.stream, op.n, op.area, op.step, op.run};
      }
    }
    if (issued < pl.n) return;
    recent[2] = recent[1]; recent[1] = recent[0]; recent[0] = cur;
    rstream[2] = rstream[1]; rstream[1] = rstream[0]; rstream[0] = pl.op[pl.n - 1].stream;
    first += cur.n;
    ++j;
  }

  // what is still deferred or pending, then the join: all of it is issued whatever fails
  StepsPlan close() const {
    StepsPlan pl;
    if (held.has) held.flush(pl);
    for (int k = 0; k < 2; ++k)
      if (pend[k] >= 0) pl.add(kOpFlushStep, k, pend[k]);
    if (two) pl.add(kOpJoin, 0);
    return pl;
  }
};

}  // namespace gnx
