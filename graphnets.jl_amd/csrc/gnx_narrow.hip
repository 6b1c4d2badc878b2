// Fused GNBlock path for narrow feature widths (README-sized dims): ONE launch does the edge update, the
// edge->node segmented sum, the node update and the per-tile partial sums of the graph update; a second tiny launch
// finishes the graph update.  The kernels themselves live in gnx_wave_kernel.h (self-contained device code).
//
// Why it can be fused: the reference's edge order is CSC order (src/pad.jl:30 — sorted by destination), so the
// in-edges of a node range [n0, n1) are the contiguous edge range [colptr[n0], colptr[n1]).  A wavefront that owns
// a node tile therefore owns every edge that aggregates into it: ef' never has to be re-read from HBM, the
// edge->node sum (nodefninput.jl:3) needs no atomics, and its order is fixed.
//
// Widths are template parameters (fully unrolled FMAs, weights as scalar operands).  launch_block_narrow() first
// looks the width set up in the ahead-of-time list below; any other width set with every width <= 32 (and <= 1024 weights) is specialised
// at run time (gnx_jit.cpp: hiprtc on the same header text) — the analogue of Julia compiling a GNBlock for its own
// dims on first use.  1 ("not applicable") sends the caller on to the MFMA / generic kernels.
#include <cstdlib>

#include "gnx_launchers.h"
#include "gnx_narrow_launch.h"
#include "gnx_wave_kernel.h"

namespace gnx {

// Instantiated width sets.  (de, dn, dg) => (oe, on); og is free (the graph update is its own small kernel).
#define GNX_NARROW_DIMS(X) \
  X(10, 5, 0, 3, 4)        \
  X(3, 4, 5, 3, 4)         \
  X(10, 5, 3, 3, 4)        \
  X(0, 2, 0, 2, 2)         \
  X(2, 2, 2, 2, 2)         \
  X(4, 3, 2, 3, 4)         \
  X(8, 8, 8, 16, 8)        \
  X(10, 5, 3, 10, 5)       \
  X(10, 5, 0, 10, 5)
// (with bfloat16 features: the list in gnx_narrow_bf16.hip, narrow_bf16_aot)
static bool narrow_aot_listed(const BlockArgs& a) {
#define GNX_CASE(DE, DN, DG, OE, ON) \
  if (a.de == DE && a.dn == DN && a.dg == DG && a.oe == OE && a.on == ON) return true;
  GNX_NARROW_DIMS(GNX_CASE)
#undef GNX_CASE
  return false;
}

// edges per lane of the run-time specialised kernel at the handle's wave-tile size (1, 2 or 4); 0: no such kernel for that size
static int jit_ept(const gnx_graphs* h) {
  const int ept = h->wtile_e_cap / 64;
  return ept * 64 == h->wtile_e_cap && (ept == 1 || ept == 2 || ept == 4) ? ept : 0;
}

// Same launch geometry as launch_wave_t, kernels specialised at run time (gnx_jit.cpp) for this width set.
static int32_t launch_wave_jit(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, int phase, bool bf16 = false) {
  const int ept = jit_ept(h);
  if (!ept) return 1;
  hipFunction_t fb = nullptr, fg = nullptr;
  const int32_t rc = jit_get(a, ept, s, &fb, &fg, bf16);
  if (rc) return rc;
  const int C = a.oe + a.on;
  BlockArgs aa = a;
  int n_rows = partial_rows(h);
  void* params[] = {&aa, &n_rows};
  if (phase & 1) {
    ProfScope ps("k_block_wave", s);
    GNX_HIP(module_launch(fb, (unsigned)((a.n_wtiles + 3) / 4), (unsigned)R, 1, kThreads, 1, 1, 0, s, params));
  }
  if ((phase & 2) && a.og > 0) {
    const int threads = graph_update_threads(h);
    const size_t lds = sizeof(float) * (size_t)graph_update_lds_floats(C, a.dg, a.og, threads);
    ProfScope ps("k_graph_t", s);
    GNX_HIP(module_launch(fg, (unsigned)a.G, (unsigned)R, 1, threads, 1, 1, (unsigned)lds, s, params));
  }
  return GNX_OK;
}

// compiles + loads the run-time specialised kernels of this width set ahead of the first forward (called from
// gnx_block_workspace_bytes, which every caller runs before a forward and never inside a stream capture)
void warm_block_narrow(const gnx_graphs* h, const gnx_block_params* p, bool bf16) {
  const BlockArgs a = block_probe(h, p);  // (a.G selects the one-graph / several-graphs variant of the kernel)
  static const bool jit_all = getenv("GNX_JIT_ALL") != nullptr;  // (diagnostic: specialise even the ahead-of-time width sets; read once)
  if (!jit_all && (bf16 ? narrow_bf16_aot(h, a) : narrow_aot_listed(a))) return;
  if (h->n_wtiles() == 0 || h->E == 0) return;
  hipFunction_t fb, fg;
  (void)jit_get(a, h->wtile_e_cap / 64, nullptr, &fb, &fg, bf16);
}

static bool wants_ln(const BlockArgs& a) { return a.ln_g[0] || a.ln_g[1] || a.ln_g[2]; }

// LayerNorm-on-load variant (GNCore: block(gn1(x)) straight from x): ahead of time for the README ex.3 core widths at the
// default wave-tile size, any other eligible width set through the run-time specialiser.
static bool ln_aot(const gnx_graphs* h, const BlockArgs& a) {
  return a.de == 10 && a.dn == 5 && a.dg == 3 && a.oe == 10 && a.on == 5 && h->wtile_e_cap == 128;
}

// Can the fused kernel run this width set (with LayerNorm on load if a.ln_g is set) right now?  Compiles the run-time
// specialised kernel if needed — except while `s` is being captured.  The GNCore forward asks before it decides to skip the
// separate gn1 kernels.
bool block_narrow_ready(const gnx_graphs* h, const BlockArgs& a, hipStream_t s) {
  if (a.n_wtiles == 0 || a.E == 0) return false;
  if (wants_ln(a)) {
    if (ln_aot(h, a)) return true;
  } else if (narrow_aot_listed(a)) {
    return h->wtile_e_cap == 64 || h->wtile_e_cap == 128 || h->wtile_e_cap == 256;
  }
  const int ept = jit_ept(h);
  hipFunction_t fb, fg;
  return ept && jit_get(a, ept, s, &fb, &fg) == GNX_OK;
}

// gnx_block_forward_chained: can the previous call's graph update ride at the front of this call's block kernel?  The two-launch form of
// an ahead-of-time width set at the default wave-tile size, graph function small enough for the kernel's LDS, <= 256 partial rows per
// graph (one wavefront per graph) or one graph.  (Batches that take the pack form run their graph update inside the kernel already.)
// bf16 features: the same rule, restricted to the bf16 ahead-of-time list (gnx_narrow_bf16.hip).
static bool pack_form(const gnx_graphs* h, const BlockArgs& a) { return h->G > 1 && h->n_packs > 0 && a.packs && a.og > 0 && !getenv("GNX_NO_PACK"); }
bool block_narrow_chain_applies(const gnx_graphs* h, const BlockArgs& a, bool bf16) {
  if (a.n_wtiles == 0 || a.E == 0 || a.og <= 0 || h->wtile_e_cap != 128 || wants_ln(a) || a.ffe_w1 || pack_form(h, a)) return false;
  const int C = a.oe + a.on;
  if (C <= 0) return false;
  const int wsl = wave_slice_floats(a.oe, 2);
  if (h->G == 1) { if (graph_update_lds_floats(C, a.dg, a.og, graph_update_threads(h)) > 4 * wsl) return false; }
  else if (h->max_wtiles_per_graph > 256 || graph_update_lds_floats(C, a.dg, a.og, 64) > wsl) return false;
  return narrow_aot_listed(a) && (!bf16 || narrow_bf16_aot(h, a));
}
// the edge + node update of THIS call with a.prev_* (the previous call's pending graph update) at the front of the same launch
int32_t launch_block_narrow_chained(const gnx_graphs* h, const BlockArgs& a0, int64_t R, hipStream_t s, bool bf16) {
  BlockArgs a = a0;
  a.prev_blocks = a.prev_partials ? (h->G == 1 ? 1 : (int)((h->G + 3) / 4)) : 0;
  if (bf16) {  // ... on bf16 rows (gnx_block_forward_steps_typed): gnx_narrow_bf16.hip
    const int32_t rc = launch_chained_bf16(h, a, R, s);
    return rc == 1 ? fail(GNX_ERR_INVALID_ARG, "internal: chained bf16 launch for a width set without that kernel") : rc;
  }
#define GNX_CASE(DE, DN, DG, OE, ON)                                                                                               \
  if (a.de == DE && a.dn == DN && a.dg == DG && a.oe == OE && a.on == ON) {                                                         \
    if constexpr (OE + ON > 0) {                                                                                                   \
      return h->G == 1 ? launch_wave_g<DE, DN, DG, OE, ON, 2, false, true, false, true>(h, a, R, s, 1)                              \
                       : launch_wave_g<DE, DN, DG, OE, ON, 2, false, false, false, true>(h, a, R, s, 1);                            \
    }                                                                                                                              \
  }
  GNX_NARROW_DIMS(GNX_CASE)
#undef GNX_CASE
  return fail(GNX_ERR_INVALID_ARG, "internal: chained launch for a width set without that kernel");
}

// A run of Z >= 2 neighbouring, hazard-free steps of gnx_block_forward_steps in one launch (k_block_wave_run) plus one for their graph
// updates: the batches that chain (block_narrow_chain_applies), whose steps would otherwise be Z chained launches, at the width sets whose
// run kernel keeps the limits that make the form worth having — at most 80 scalar registers (the eighth workgroup per CU), no scratch, no
// more vector registers than the chained kernel of the set (tests/test_steps_runs_cpu.py).  The three wide sets of GNX_NARROW_DIMS
// ((8,8,8)=>(16,8), (10,5,3)=>(10,5), (10,5,0)=>(10,5)) are over 100 scalar and vector registers in every form — three or four workgroups per
// CU whatever the schedule — and keep one launch per step.
#define GNX_NARROW_RUN_DIMS(X) \
  X(10, 5, 0, 3, 4)            \
  X(3, 4, 5, 3, 4)             \
  X(10, 5, 3, 3, 4)            \
  X(0, 2, 0, 2, 2)             \
  X(2, 2, 2, 2, 2)             \
  X(4, 3, 2, 3, 4)
bool block_narrow_run_applies(const gnx_graphs* h, const BlockArgs& a, bool bf16) {
  if (!block_narrow_chain_applies(h, a, bf16)) return false;
  if (bf16) return narrow_bf16_run(h, a);
#define GNX_CASE(DE, DN, DG, OE, ON) \
  if (a.de == DE && a.dn == DN && a.dg == DG && a.oe == OE && a.on == ON) return true;
  GNX_NARROW_RUN_DIMS(GNX_CASE)
#undef GNX_CASE
  return false;
}
int32_t launch_block_narrow_run(const gnx_graphs* h, const BlockArgs& a, const RunTable& t, int Z, hipStream_t s, bool bf16, int phase) {
  if (bf16) {  // ... on bf16 rows: gnx_narrow_bf16.hip (always both launches)
    if (phase != 3) return fail(GNX_ERR_INVALID_ARG, "internal: a bf16 run is issued whole");
    const int32_t rc = launch_run_bf16(h, a, t, Z, s);
    return rc == 1 ? fail(GNX_ERR_INVALID_ARG, "internal: bf16 run launch for a width set without that kernel") : rc;
  }
#define GNX_CASE(DE, DN, DG, OE, ON)                                                                                               \
  if (a.de == DE && a.dn == DN && a.dg == DG && a.oe == OE && a.on == ON) {                                                         \
    if constexpr (OE + ON > 0) {                                                                                                   \
      return h->G == 1 ? launch_wave_run<DE, DN, DG, OE, ON, true>(h, a, t, Z, s, phase) : launch_wave_run<DE, DN, DG, OE, ON, false>(h, a, t, Z, s, phase); \
    }                                                                                                                              \
  }
  GNX_NARROW_RUN_DIMS(GNX_CASE)
#undef GNX_CASE
  return fail(GNX_ERR_INVALID_ARG, "internal: run launch for a width set without that kernel");
}

// A run whose block launch carries the graph updates of the run before it (k_block_wave_carry; fp32 rows): the run sets whose carrying
// kernel keeps the run kernel's limits — no scratch, at most 80 scalar registers, no more vector registers than the chained kernel of the
// set (tests/test_steps_deferred_cpu.py) — in the one-graph form (X1) and the several-graphs form (XG).  A set or form without one keeps the
// two launches per run: of GNX_NARROW_RUN_DIMS, (2,2,2)=>(2,2) — its carrying kernel takes 55 vector registers in both forms, its chained
// kernel 54.
#define GNX_NARROW_CARRY_DIMS(X1, XG) \
  X1(10, 5, 0, 3, 4) XG(10, 5, 0, 3, 4) \
  X1(3, 4, 5, 3, 4) XG(3, 4, 5, 3, 4)   \
  X1(10, 5, 3, 3, 4) XG(10, 5, 3, 3, 4) \
  X1(0, 2, 0, 2, 2) XG(0, 2, 0, 2, 2)   \
  X1(4, 3, 2, 3, 4) XG(4, 3, 2, 3, 4)
bool block_narrow_carry_applies(const gnx_graphs* h, const BlockArgs& a) {
  if (!block_narrow_run_applies(h, a, false)) return false;
#define GNX_CASE1(DE, DN, DG, OE, ON) \
  if (h->G == 1 && a.de == DE && a.dn == DN && a.dg == DG && a.oe == OE && a.on == ON) return true;
#define GNX_CASEG(DE, DN, DG, OE, ON) \
  if (h->G != 1 && a.de == DE && a.dn == DN && a.dg == DG && a.oe == OE && a.on == ON) return true;
  GNX_NARROW_CARRY_DIMS(GNX_CASE1, GNX_CASEG)
#undef GNX_CASE1
#undef GNX_CASEG
  return false;
}
int32_t launch_block_narrow_carry(const gnx_graphs* h, const BlockArgs& a, const RunTable& t, int Z, const PrevTable& prev, hipStream_t s) {
#define GNX_CASE1(DE, DN, DG, OE, ON) \
  if (h->G == 1 && a.de == DE && a.dn == DN && a.dg == DG && a.oe == OE && a.on == ON) return launch_wave_carry<DE, DN, DG, OE, ON, true>(h, a, t, Z, prev, s);
#define GNX_CASEG(DE, DN, DG, OE, ON) \
  if (h->G != 1 && a.de == DE && a.dn == DN && a.dg == DG && a.oe == OE && a.on == ON) return launch_wave_carry<DE, DN, DG, OE, ON, false>(h, a, t, Z, prev, s);
  GNX_NARROW_CARRY_DIMS(GNX_CASE1, GNX_CASEG)
#undef GNX_CASE1
#undef GNX_CASEG
  return fail(GNX_ERR_INVALID_ARG, "internal: carrying run launch for a width set without that kernel");
}

// the edge FeedForward + residual of a narrow GNCore inside the block kernel (k_block_wave<..., FFE>): ahead-of-time widths, identity / relu
// activations.  GNX_FLAG_NO_FFE keeps the FeedForward in k_core_post3.
bool block_narrow_ffe_applies(const gnx_graphs* h, const BlockArgs& a, int act1, int act2) {
  return ln_aot(h, a) && a.ln_g[0] && act1 <= GNX_ACT_RELU && act2 <= GNX_ACT_RELU && a.act_e <= GNX_ACT_RELU && h->max_in_degree <= h->wtile_e_cap &&
         !form(GNX_FLAG_NO_FFE);  // (max_in_degree: every wave tile is ONE chunk of edges — the kernel runs the FeedForward once, at its end)
}

// Which fused kernel launch_block_narrow runs for a call without LayerNorm on load: the run-time specialised kernel first under GNX_JIT_ALL,
// an ahead-of-time width set at a wave-tile size it has, else the specialised kernel (never compiled while `s` is being captured); none:
// the caller goes on to the matrix-core / generic kernels.  The ONE place this is decided: launch_block_narrow dispatches on it and
// block_narrow_takes (gnx_block_forward_steps: two streams only on this path) asks it.
enum NarrowRoute { NR_NONE, NR_AOT, NR_JIT };
static NarrowRoute narrow_route(const gnx_graphs* h, const BlockArgs& a, hipStream_t s, bool bf16 = false) {
  if (a.n_wtiles == 0 || a.E == 0 || wants_ln(a)) return NR_NONE;
  auto jit_ok = [&]() {
    const int ept = jit_ept(h);
    hipFunction_t fb, fg;
    return ept && jit_get(a, ept, s, &fb, &fg, bf16) == GNX_OK;
  };
  static const bool jit_all = getenv("GNX_JIT_ALL") != nullptr;  // testing: run-time specialise even the listed width sets
  if (jit_all && jit_ok()) return NR_JIT;
  if (bf16) {
    if (narrow_bf16_aot(h, a)) return NR_AOT;
  } else if (narrow_aot_listed(a)) {
    return h->wtile_e_cap == 64 || h->wtile_e_cap == 128 || (h->wtile_e_cap == 256 && (a.de + a.dn) * 4 <= 64) ? NR_AOT : NR_NONE;  // (launch_fused's EPT)
  }
  return jit_ok() ? NR_JIT : NR_NONE;
}

bool block_narrow_takes(const gnx_graphs* h, const BlockArgs& a, hipStream_t s, bool bf16) { return narrow_route(h, a, s, bf16) != NR_NONE; }

// 1: no fused kernel takes these widths.  bf16 features (gnx_block_forward_typed): the native kernels (on 1 the caller converts around the
// fp32 forward); LayerNorm on load only as the block of a bf16 core (launch_ln_bf16: bf16 rows in, fp32 out); phase 2 alone is the flush of
// a chained bf16 step (ahead-of-time widths only).
int32_t launch_block_narrow(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, int phase, bool bf16) {
  if (a.n_wtiles == 0 || a.E == 0) return 1;
  if (wants_ln(a)) {  // only reached after block_narrow_ready(): a miss here would silently drop the LayerNorm
    if (bf16) {       // the block of a bf16 core (gnx_core_forward_typed's native path: ahead-of-time widths only): gnx_narrow_bf16.hip
      const int32_t rc = launch_ln_bf16(h, a, R, s, phase);
      return rc == 1 ? fail(GNX_ERR_INVALID_ARG, "internal: LayerNorm-on-load on bf16 rows for a width set without that kernel") : rc;
    }
    if (a.ffe_w1) {   // (set by gnx_core_forward only after block_narrow_ffe_applies())
      if (!ln_aot(h, a)) return fail(GNX_ERR_INVALID_ARG, "internal: FeedForward-in-the-edge-lanes requested for a width set without that kernel");
      return h->G == 1 ? launch_wave_g<10, 5, 3, 10, 5, 2, true, true, true>(h, a, R, s, phase) : launch_wave_g<10, 5, 3, 10, 5, 2, true, false, true>(h, a, R, s, phase);
    }
    if (ln_aot(h, a)) return launch_wave_t<10, 5, 3, 10, 5, 2, true>(h, a, R, s, phase);
    const int32_t rc = launch_wave_jit(h, a, R, s, phase);
    return rc == 1 ? fail(GNX_ERR_INVALID_ARG, "internal: LayerNorm-on-load requested but the fused kernel is not available") : rc;
  }
  const NarrowRoute route = narrow_route(h, a, s, bf16);
  if (route == NR_NONE) return 1;
  if (route == NR_JIT) return launch_wave_jit(h, a, R, s, phase, bf16);  // compiled on first use (gnx_block_workspace_bytes)
  if (bf16) {
    const int32_t rc = launch_fused_bf16(h, a, R, s, phase);
    return rc == 1 ? fail(GNX_ERR_INVALID_ARG, "internal: ahead-of-time bf16 route for a width set without that kernel") : rc;
  }
  // 16-B vector copies assume fp32-aligned buffers (always true for fp32 arrays); nothing else is required
#define GNX_CASE(DE, DN, DG, OE, ON) \
  if (a.de == DE && a.dn == DN && a.dg == DG && a.oe == OE && a.on == ON) return launch_fused<DE, DN, DG, OE, ON>(h, a, R, s, phase);
  GNX_NARROW_DIMS(GNX_CASE)
#undef GNX_CASE
  return fail(GNX_ERR_INVALID_ARG, "internal: ahead-of-time route for a width set without that kernel");
}

}  // namespace gnx
