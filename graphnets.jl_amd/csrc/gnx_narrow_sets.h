// Which ahead-of-time kernel forms of the fused narrow block exist for a width set (de, dn, dg) => (oe, on) — og is free: the graph update is
// its own small kernel.  The ONE table: narrow_set_dispatch (gnx_narrow_launch.h) instantiates exactly what a row's mask names, and every
// "does this form apply" predicate of gnx_narrow.hip reads narrow_forms / narrow_cap_ok.  Any other narrow width set is specialised at run
// time (gnx_jit.cpp).  Plain C++, no HIP: tests/test_narrow_sets_cpu.py compiles this header on its own and derives from it the kernel
// names the two translation units must produce.
#pragma once

namespace gnx {

enum : unsigned {
  NF_PLAIN = 1,    // k_block_wave at EPT 1, 2 and (narrow_cap_ok) 4, its PACK form, its chained form (gnx_block_forward_chained), k_graph_t
  NF_RUN1 = 2,     // k_block_wave_run / k_graph_run, one graph: a run of hazard-free steps of gnx_block_forward_steps in one launch
  NF_RUNG = 4,     // ... several graphs
  NF_CARRY1 = 8,   // k_block_wave_carry, one graph: a run whose launch carries the graph updates of the run before it
  NF_CARRYG = 16,  // ... several graphs
  NF_LN = 32,      // LayerNorm on load (the block of a GNCore: block(gn1(x)) straight from x), at the default wave-tile size only
  NF_FFE = 64,     // k_block_wave_ffe: the core's edge FeedForward + residual in the edge lanes, at the default wave-tile size only
};

template <int DE_, int DN_, int DG_, int OE_, int ON_, unsigned FORMS>
struct NarrowSet {
  static constexpr int DE = DE_, DN = DN_, DG = DG_, OE = OE_, ON = ON_;
  static constexpr unsigned forms = FORMS;
  static_assert(OE_ + ON_ > 0, "the graph update of the fused path needs at least one of ef' / nf'");
  static constexpr bool is(int de, int dn, int dg, int oe, int on) { return de == DE_ && dn == DN_ && dg == DG_ && oe == OE_ && on == ON_; }
};
template <class... S>
struct NarrowSetList {};

// A run kernel (NF_RUN*) exists where it keeps the limits that make the form worth having — at most 80 scalar registers (the eighth
// workgroup per CU), no scratch, no more vector registers than the chained kernel of the set (tests/test_steps_runs_cpu.py); a carrying
// kernel (NF_CARRY*) where it keeps the run kernel's limits (tests/test_steps_deferred_cpu.py).  A set or form without one keeps one
// chained launch per step, or two launches per run.
constexpr unsigned NF_RUNS = NF_PLAIN | NF_RUN1 | NF_RUNG, NF_CARRIES = NF_RUNS | NF_CARRY1 | NF_CARRYG;

// fp32 rows
using NarrowSetsF32 = NarrowSetList<
    NarrowSet<10, 5, 0, 3, 4, NF_CARRIES>,  // README ex.1 / the headline batch (BASELINE configs[1])
    NarrowSet<3, 4, 5, 3, 4, NF_CARRIES>,   // README ex.1's outputs: dims to dims (the recurrent loop x_{i+1} = block(x_i))
    NarrowSet<10, 5, 3, 3, 4, NF_CARRIES>,
    NarrowSet<0, 2, 0, 2, 2, NF_CARRIES>,
    NarrowSet<2, 2, 2, 2, 2, NF_RUNS>,  // its carrying kernel takes 55 vector registers in both forms, its chained kernel 54
    NarrowSet<4, 3, 2, 3, 4, NF_CARRIES>,
    // the three wide sets are over 100 scalar and vector registers in every form — three or four workgroups per CU whatever the
    // schedule — and keep one launch per step
    NarrowSet<8, 8, 8, 16, 8, NF_PLAIN>,
    NarrowSet<10, 5, 3, 10, 5, NF_PLAIN | NF_LN | NF_FFE>,  // README ex.3's core widths
    NarrowSet<10, 5, 0, 10, 5, NF_PLAIN>>;

// bf16 rows (gnx_narrow_bf16.hip)
using NarrowSetsBF16 = NarrowSetList<
    // no run kernel for several graphs: it needs 54 vector registers, as the plain bf16 kernel does, against the 52 of the set's chained kernel
    NarrowSet<10, 5, 0, 3, 4, NF_PLAIN | NF_RUN1>,
    NarrowSet<3, 4, 5, 3, 4, NF_RUNS>,  // a set with dg > 0 (the chained graph update reads a bf16 gf) that also maps dims to dims
    NarrowSet<10, 5, 3, 10, 5, NF_LN | NF_FFE>>;  // the block of a bf16 GNCore only: bf16 rows in, fp32 intermediates out

template <class... S>
constexpr unsigned narrow_forms_in(NarrowSetList<S...>, int de, int dn, int dg, int oe, int on) {
  unsigned m = 0;
  ((S::is(de, dn, dg, oe, on) ? (void)(m = S::forms) : (void)0), ...);
  return m;
}

// the forms of a width set; 0: not listed
constexpr unsigned narrow_forms(int de, int dn, int dg, int oe, int on, bool bf16) {
  return bf16 ? narrow_forms_in(NarrowSetsBF16{}, de, dn, dg, oe, on) : narrow_forms_in(NarrowSetsF32{}, de, dn, dg, oe, on);
}

// The wave-tile rule: the plain kernel's edges per lane are cap / 64 — 1, 2, or 4 while a lane's four input rows stay within 64 floats.
// (Every other form exists at cap 128 alone.)
constexpr bool narrow_cap_ok(int de, int dn, int cap) { return cap == 64 || cap == 128 || (cap == 256 && (de + dn) * 4 <= 64); }

}  // namespace gnx
