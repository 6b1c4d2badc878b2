// Fused GNBlock path for narrow feature widths (README-sized dims): ONE launch does the edge update, the
// edge->node segmented sum, the node update and the per-tile partial sums of the graph update; a second tiny launch
// finishes the graph update.  The kernels themselves live in gnx_wave_kernel.h (self-contained device code).
//
// Why it can be fused: the reference's edge order is CSC order (src/pad.jl:30 — sorted by destination), so the
// in-edges of a node range [n0, n1) are the contiguous edge range [colptr[n0], colptr[n1]).  A wavefront that owns
// a node tile therefore owns every edge that aggregates into it: ef' never has to be re-read from HBM, the
// edge->node sum (nodefninput.jl:3) needs no atomics, and its order is fixed.
//
// Widths are template parameters (fully unrolled FMAs, weights as scalar operands).  Which ahead-of-time forms a width set has is ONE
// table, gnx_narrow_sets.h: every predicate here reads narrow_forms / narrow_cap_ok and adds only the conditions that are its own, every
// launcher goes through narrow_set_dispatch (gnx_narrow_launch.h), the table's one expansion site.  launch_block_narrow() first
// looks the width set up there; any other width set with every width <= 32 (and <= 1024 weights) is specialised
// at run time (gnx_jit.cpp: hiprtc on the same header text) — the analogue of Julia compiling a GNBlock for its own
// dims on first use.  1 ("not applicable") sends the caller on to the MFMA / generic kernels.
#include <cstdlib>

#include "gnx_launchers.h"
#include "gnx_narrow_launch.h"
#include "gnx_wave_kernel.h"

namespace gnx {

static int32_t or_internal(int32_t rc, const char* msg) { return rc == 1 ? fail(GNX_ERR_INVALID_ARG, msg) : rc; }  // (a launcher's "no such kernel")

// an ahead-of-time plain kernel exists for these widths at the handle's wave-tile size
static bool plain_aot(const gnx_graphs* h, const BlockArgs& a, bool bf16) {
  return (narrow_forms(a, bf16) & NF_PLAIN) && narrow_cap_ok(a.de, a.dn, h->wtile_e_cap);
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
  if (!jit_all && plain_aot(h, a, bf16)) return;
  if (h->n_wtiles() == 0 || h->E == 0) return;
  hipFunction_t fb, fg;
  (void)jit_get(a, h->wtile_e_cap / 64, nullptr, &fb, &fg, bf16);
}

static bool wants_ln(const BlockArgs& a) { return a.ln_g[0] || a.ln_g[1] || a.ln_g[2]; }

// Can the fused kernel run this width set (with LayerNorm on load if a.ln_g is set) right now?  Compiles the run-time
// specialised kernel if needed — except while `s` is being captured.  The GNCore forward asks before it decides to skip the
// separate gn1 kernels.
bool block_narrow_ready(const gnx_graphs* h, const BlockArgs& a, hipStream_t s) {
  if (a.n_wtiles == 0 || a.E == 0) return false;
  if (wants_ln(a) ? narrow_ln_aot(h, a, false) : plain_aot(h, a, false)) return true;
  const int ept = jit_ept(h);
  hipFunction_t fb, fg;
  return ept && jit_get(a, ept, s, &fb, &fg) == GNX_OK;
}

// gnx_block_forward_chained: can the previous call's graph update ride at the front of this call's block kernel?  The two-launch form of
// an ahead-of-time width set at the default wave-tile size, graph function small enough for the kernel's LDS, <= 256 partial rows per
// graph (one wavefront per graph) or one graph.  (Batches that take the pack form run their graph update inside the kernel already.)
// bf16 features: the same rule on the bf16 rows of the table.
static bool pack_form(const gnx_graphs* h, const BlockArgs& a) { return h->G > 1 && h->n_packs > 0 && a.packs && a.og > 0 && !getenv("GNX_NO_PACK"); }
bool block_narrow_chain_applies(const gnx_graphs* h, const BlockArgs& a, bool bf16) {
  if (a.n_wtiles == 0 || a.E == 0 || a.og <= 0 || h->wtile_e_cap != 128 || wants_ln(a) || a.ffe_w1 || pack_form(h, a)) return false;
  const int C = a.oe + a.on;
  if (C <= 0) return false;
  const int wsl = wave_slice_floats(a.oe, 2);
  if (h->G == 1) { if (graph_update_lds_floats(C, a.dg, a.og, graph_update_threads(h)) > 4 * wsl) return false; }
  else if (h->max_wtiles_per_graph > 256 || graph_update_lds_floats(C, a.dg, a.og, 64) > wsl) return false;
  return narrow_forms(a, bf16) & NF_PLAIN;
}
// the edge + node update of THIS call with a.prev_* (the previous call's pending graph update) at the front of the same launch
int32_t launch_block_narrow_chained(const gnx_graphs* h, const BlockArgs& a0, int64_t R, hipStream_t s, bool bf16) {
  BlockArgs a = a0;
  a.prev_blocks = a.prev_partials ? (h->G == 1 ? 1 : (int)((h->G + 3) / 4)) : 0;
  if (bf16)  // ... on bf16 rows (gnx_block_forward_steps_typed): gnx_narrow_bf16.hip
    return or_internal(launch_chained_bf16(h, a, R, s), "internal: chained bf16 launch for a width set without that kernel");
  return or_internal(launch_narrow_chained<false>(h, a, R, s), "internal: chained launch for a width set without that kernel");
}

// A run of Z >= 2 neighbouring, hazard-free steps of gnx_block_forward_steps in one launch (k_block_wave_run) plus one for their graph
// updates: the batches that chain (block_narrow_chain_applies), whose steps would otherwise be Z chained launches, at the width sets with a
// run kernel for the batch's form (NF_RUN1: one graph, NF_RUNG: several).
bool block_narrow_run_applies(const gnx_graphs* h, const BlockArgs& a, bool bf16) {
  return block_narrow_chain_applies(h, a, bf16) && (narrow_forms(a, bf16) & (h->G == 1 ? NF_RUN1 : NF_RUNG));
}
int32_t launch_block_narrow_run(const gnx_graphs* h, const BlockArgs& a, const RunTable& t, int Z, hipStream_t s, bool bf16, int phase) {
  if (bf16) {  // ... on bf16 rows: gnx_narrow_bf16.hip (always both launches)
    if (phase != 3) return fail(GNX_ERR_INVALID_ARG, "internal: a bf16 run is issued whole");
    return or_internal(launch_run_bf16(h, a, t, Z, s), "internal: bf16 run launch for a width set without that kernel");
  }
  return or_internal(launch_narrow_run<false>(h, a, t, Z, s, phase), "internal: run launch for a width set without that kernel");
}

// A run whose block launch carries the graph updates of the run before it (k_block_wave_carry; fp32 rows): the run sets with a carrying
// kernel for the batch's form (NF_CARRY1 / NF_CARRYG).  A set or form without one keeps the two launches per run.
bool block_narrow_carry_applies(const gnx_graphs* h, const BlockArgs& a) {
  return block_narrow_run_applies(h, a, false) && (narrow_forms(a, false) & (h->G == 1 ? NF_CARRY1 : NF_CARRYG));
}
int32_t launch_block_narrow_carry(const gnx_graphs* h, const BlockArgs& a, const RunTable& t, int Z, const PrevTable& prev, hipStream_t s) {
  const int32_t rc = narrow_set_dispatch<false>(a, [&](auto set) -> int32_t {
    using S = decltype(set);
    if (h->G == 1) {
      if constexpr (S::forms & NF_CARRY1) return launch_wave_carry<S::DE, S::DN, S::DG, S::OE, S::ON, true>(h, a, t, Z, prev, s);
    } else {
      if constexpr (S::forms & NF_CARRYG) return launch_wave_carry<S::DE, S::DN, S::DG, S::OE, S::ON, false>(h, a, t, Z, prev, s);
    }
    return 1;
  });
  return or_internal(rc, "internal: carrying run launch for a width set without that kernel");
}

// the edge FeedForward + residual of a narrow GNCore inside the block kernel (k_block_wave<..., FFE>): the sets with NF_FFE, identity / relu
// activations.  GNX_FLAG_NO_FFE keeps the FeedForward in k_core_post3.
bool block_narrow_ffe_applies(const gnx_graphs* h, const BlockArgs& a, int act1, int act2) {
  return (narrow_forms(a, false) & NF_FFE) && h->wtile_e_cap == 128 && a.ln_g[0] && act1 <= GNX_ACT_RELU && act2 <= GNX_ACT_RELU && a.act_e <= GNX_ACT_RELU &&
         h->max_in_degree <= h->wtile_e_cap &&  // (every wave tile is ONE chunk of edges — the kernel runs the FeedForward once, at its end)
         !form(GNX_FLAG_NO_FFE);
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
  if (plain_aot(h, a, bf16)) return NR_AOT;
  return jit_ok() ? NR_JIT : NR_NONE;
}

bool block_narrow_takes(const gnx_graphs* h, const BlockArgs& a, hipStream_t s, bool bf16) { return narrow_route(h, a, s, bf16) != NR_NONE; }

// 1: no fused kernel takes these widths.  bf16 features (gnx_block_forward_typed): the native kernels (on 1 the caller converts around the
// fp32 forward); LayerNorm on load only as the block of a bf16 core (launch_ln_bf16: bf16 rows in, fp32 out); phase 2 alone is the flush of
// a chained bf16 step (ahead-of-time widths only).
int32_t launch_block_narrow(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, int phase, bool bf16) {
  if (a.n_wtiles == 0 || a.E == 0) return 1;
  if (wants_ln(a)) {  // only reached after block_narrow_ready(): a miss here would silently drop the LayerNorm
    if (bf16)         // the block of a bf16 core (gnx_core_forward_typed's native path: ahead-of-time widths only): gnx_narrow_bf16.hip
      return or_internal(launch_ln_bf16(h, a, R, s, phase), "internal: LayerNorm-on-load on bf16 rows for a width set without that kernel");
    if (a.ffe_w1)     // (set by gnx_core_forward only after block_narrow_ffe_applies())
      return or_internal(launch_narrow_ln<false>(h, a, R, s, phase), "internal: FeedForward-in-the-edge-lanes requested for a width set without that kernel");
    if (narrow_ln_aot(h, a, false)) return launch_narrow_ln<false>(h, a, R, s, phase);
    return or_internal(launch_wave_jit(h, a, R, s, phase), "internal: LayerNorm-on-load requested but the fused kernel is not available");
  }
  const NarrowRoute route = narrow_route(h, a, s, bf16);
  if (route == NR_NONE) return 1;
  if (route == NR_JIT) return launch_wave_jit(h, a, R, s, phase, bf16);  // compiled on first use (gnx_block_workspace_bytes)
  if (bf16) return or_internal(launch_fused_bf16(h, a, R, s, phase), "internal: ahead-of-time bf16 route for a width set without that kernel");
  // 16-B vector copies assume fp32-aligned buffers (always true for fp32 arrays); nothing else is required
  return or_internal(launch_narrow_plain<false>(h, a, R, s, phase), "internal: ahead-of-time route for a width set without that kernel");
}

}  // namespace gnx
