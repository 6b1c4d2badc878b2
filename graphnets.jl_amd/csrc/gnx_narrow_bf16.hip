// The fused narrow kernels with bfloat16 feature rows (k_block_wave<..., BF16 = true>, its chained form k_block_wave<..., CHAIN, BF16>,
// k_graph_t<C, ONEG, true>, the run form k_block_wave_run / k_graph_run of several steps in one launch) for the ahead-of-time width sets; gnx_narrow.hip routes gnx_block_forward_typed and the bf16 steps of
// gnx_block_forward_steps_typed here, every other narrow width set is specialised at run time (gnx_jit.cpp).  Also the block of a bf16
// GNCore at README ex.3's widths (k_block_wave<..., LN, ..., BF16>, k_block_wave_ffe<..., BF16>: bf16 rows in, fp32 intermediates out).
// A translation unit of its own because build.py compiles it without the SLP vectoriser (-fno-slp-vectorize; gnx_jit.cpp passes the same
// option for a bf16 key): with it, every widened value feeds a v_pk_fma_f32 as the low half of a register pair of its own, and the README
// ex.1 kernel needs 70 instead of 58 VGPRs — 7 instead of 8 waves per SIMD.  Scalar FMAs compute the same bits.
#include "gnx_launchers.h"
#include "gnx_narrow_launch.h"
#include "gnx_wave_kernel.h"

namespace gnx {

// README ex.1 / the headline batch (BASELINE configs[1]); README ex.1's outputs (3,4,5) => (3,4,5): a set with dg > 0 (the chained graph
// update reads a bf16 gf) that also maps dims to dims (the recurrent loop x_{i+1} = block(x_i))
#define GNX_NARROW_DIMS_BF16(X) \
  X(10, 5, 0, 3, 4)             \
  X(3, 4, 5, 3, 4)

// an ahead-of-time bf16 kernel exists for these widths at the handle's wave-tile size (launch_fused's EPT)
bool narrow_bf16_aot(const gnx_graphs* h, const BlockArgs& a) {
#define GNX_CASE(DE, DN, DG, OE, ON)                                     \
  if (a.de == DE && a.dn == DN && a.dg == DG && a.oe == OE && a.on == ON) \
    return h->wtile_e_cap == 64 || h->wtile_e_cap == 128 || (h->wtile_e_cap == 256 && (DE + DN) * 4 <= 64);
  GNX_NARROW_DIMS_BF16(GNX_CASE)
#undef GNX_CASE
  return false;
}

// the block on bf16 rows — whole (phase 3), or only the graph update from partial rows a chained launch left (phase 2: a flush of
// gnx_block_forward_steps_typed); 1: no ahead-of-time kernel for these widths
int32_t launch_fused_bf16(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, int phase) {
#define GNX_CASE(DE, DN, DG, OE, ON) \
  if (a.de == DE && a.dn == DN && a.dg == DG && a.oe == OE && a.on == ON) return launch_fused<DE, DN, DG, OE, ON, true>(h, a, R, s, phase);
  GNX_NARROW_DIMS_BF16(GNX_CASE)
#undef GNX_CASE
  return 1;
}

// the chained form (gnx_narrow.hip: launch_block_narrow_chained) on bf16 rows: this call's edge + node update with the previous call's
// graph update at the front of the launch; 1: no ahead-of-time kernel for these widths
int32_t launch_chained_bf16(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s) {
#define GNX_CASE(DE, DN, DG, OE, ON)                                                                                               \
  if (a.de == DE && a.dn == DN && a.dg == DG && a.oe == OE && a.on == ON) {                                                         \
    if constexpr (OE + ON > 0) {                                                                                                   \
      return h->G == 1 ? launch_wave_g<DE, DN, DG, OE, ON, 2, false, true, false, true, true>(h, a, R, s, 1)                        \
                       : launch_wave_g<DE, DN, DG, OE, ON, 2, false, false, false, true, true>(h, a, R, s, 1);                      \
    }                                                                                                                              \
  }
  GNX_NARROW_DIMS_BF16(GNX_CASE)
#undef GNX_CASE
  return 1;
}

// ---- the block of a bf16 GNCore (gnx_core_forward_typed): LayerNorm on load of bf16 rows, fp32 out ----
// README ex.3's core widths at the default wave-tile size: the set gnx_narrow.hip's ln_aot has ahead of time for fp32 rows.
bool narrow_bf16_ln_aot(const gnx_graphs* h, const BlockArgs& a) {
  return a.n_wtiles > 0 && a.E > 0 && a.de == 10 && a.dn == 5 && a.dg == 3 && a.oe == 10 && a.on == 5 && h->wtile_e_cap == 128;
}
// gn1 applied to the bf16 rows as they are loaded; the block's outputs are the core's intermediates and leave as fp32 (a.nf_out, a.gf_out and —
// without the FeedForward in the edge lanes — a.ef_out are fp32 staging).  a.ffe_w1 set: the edge lanes finish the core's edge rows and
// store them, rounded once, as bf16 (a.ef_out is then the caller's).  1: not these widths.
int32_t launch_ln_bf16(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, int phase) {
  if (!narrow_bf16_ln_aot(h, a)) return 1;
  if (a.ffe_w1)
    return h->G == 1 ? launch_wave_g<10, 5, 3, 10, 5, 2, true, true, true, false, true>(h, a, R, s, phase)
                     : launch_wave_g<10, 5, 3, 10, 5, 2, true, false, true, false, true>(h, a, R, s, phase);
  return launch_wave_t<10, 5, 3, 10, 5, 2, true, true>(h, a, R, s, phase);
}

// A run of steps in one launch (gnx_narrow.hip: launch_block_narrow_run) on bf16 rows.  (DE, DN, DG, OE, ON, SEVERAL): SEVERAL — the set
// has a run kernel for batches of several graphs too.  (10,5,0)=>(3,4,5) has not: that kernel needs 54 vector registers, as the plain bf16
// kernel does, against the 52 of the set's chained kernel — the limit a run kernel keeps (tests/test_steps_runs_cpu.py); such a batch keeps
// one chained launch per step.
#define GNX_NARROW_RUN_DIMS_BF16(X) \
  X(10, 5, 0, 3, 4, false)          \
  X(3, 4, 5, 3, 4, true)
bool narrow_bf16_run(const gnx_graphs* h, const BlockArgs& a) {
#define GNX_CASE(DE, DN, DG, OE, ON, SEVERAL) \
  if (a.de == DE && a.dn == DN && a.dg == DG && a.oe == OE && a.on == ON) return h->G == 1 || SEVERAL;
  GNX_NARROW_RUN_DIMS_BF16(GNX_CASE)
#undef GNX_CASE
  return false;
}
// 1: no run kernel for these widths and this batch
int32_t launch_run_bf16(const gnx_graphs* h, const BlockArgs& a, const RunTable& t, int Z, hipStream_t s) {
#define GNX_CASE(DE, DN, DG, OE, ON, SEVERAL)                                                                \
  if (a.de == DE && a.dn == DN && a.dg == DG && a.oe == OE && a.on == ON) {                                   \
    if (h->G == 1) return launch_wave_run<DE, DN, DG, OE, ON, true, true>(h, a, t, Z, s);                     \
    if constexpr (SEVERAL) return launch_wave_run<DE, DN, DG, OE, ON, false, true>(h, a, t, Z, s);            \
  }
  GNX_NARROW_RUN_DIMS_BF16(GNX_CASE)
#undef GNX_CASE
  return 1;
}

}  // namespace gnx
