// Launchers of the fused narrow kernels (gnx_wave_kernel.h) for a width set known at compile time, and — at the end — the ONE place the
// table of gnx_narrow_sets.h is expanded: narrow_set_dispatch and the four launchers by form on top of it.  Shared by gnx_narrow.hip (fp32
// features: BF16 = false) and gnx_narrow_bf16.hip (bfloat16 features, a translation unit of its own: see there).
#pragma once
#include <cstdlib>

#include "gnx_device.h"
#include "gnx_narrow_sets.h"
#include "gnx_wave_kernel.h"

namespace gnx {

// Rows of the partial-sum table per replica: one per workgroup (one graph) or one per wave tile (several graphs).
static int partial_rows(const gnx_graphs* h) { return (int)(h->G == 1 ? (h->n_wtiles() + 3) / 4 : h->n_wtiles()); }

// Threads of the graph update: one wavefront per graph while a graph has <= 256 partial rows (the usual heterogeneous batch:
// C3 has ~16 rows per graph, C5 ~3), else 256, and 1024 from 1024 rows on (C2: 2032 rows, two per thread in flight at once).
static int graph_update_threads(const gnx_graphs* h) {
  return graph_update_threads_for_rows(h->G == 1 ? (h->n_wtiles() + 3) / 4 : h->max_wtiles_per_graph);
}

// LN with BF16 (gnx_wave_kernel.h: OUT32): bf16 rows in, the block's own outputs — ef' / nf' / gf' — out as fp32 (the block of a bf16 core)
template <int DE, int DN, int DG, int OE, int ON, int EPT, bool LN, bool ONEG, bool FFE = false, bool CHAIN = false, bool BF16 = false>
static int32_t launch_wave_g(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, int phase) {
  constexpr int C = OE + ON;
  const int n_rows = partial_rows(h);
  const unsigned grid = (unsigned)((a.n_wtiles + 3) / 4) + (CHAIN ? (unsigned)a.prev_blocks : 0u);
  if (phase & 1) {
    ProfScope ps("k_block_wave", s);
#ifdef GNX_WAVE_STAMPS_BUILD  // diagnostic build: GNX_WAVE_STAMPS_DUMP=<file> writes [wave tile][8] shader-clock stamps of every (eager) launch
    static unsigned long long* d_dbg = nullptr;
    static size_t dbg_cap = 0;
    const char* dump = getenv("GNX_WAVE_STAMPS_DUMP");
    if (dump) {
      if (dbg_cap < (size_t)a.n_wtiles) { if (d_dbg) (void)hipFree(d_dbg); dbg_cap = (size_t)a.n_wtiles; (void)hipMalloc((void**)&d_dbg, dbg_cap * 64); }
      (void)hipMemsetAsync(d_dbg, 0, (size_t)a.n_wtiles * 64, s);
      (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_wave_dbg), &d_dbg, sizeof(d_dbg), 0, hipMemcpyHostToDevice, s);
    }
#endif
    if constexpr (FFE) GNX_LAUNCH((k_block_wave_ffe<DE, DN, DG, OE, ON, EPT, ONEG, BF16>), dim3(grid, (unsigned)R), dim3(kThreads), 0, s, a, n_rows);
    else GNX_LAUNCH((k_block_wave<DE, DN, DG, OE, ON, EPT, LN, ONEG, false, false, CHAIN, BF16>), dim3(grid, (unsigned)R), dim3(kThreads), 0, s, a, n_rows);
    GNX_HIP(hipGetLastError());
#ifdef GNX_WAVE_STAMPS_BUILD
    if (dump) {
      (void)hipStreamSynchronize(s);
      std::vector<unsigned long long> hs((size_t)a.n_wtiles * 8);
      (void)hipMemcpy(hs.data(), d_dbg, hs.size() * 8, hipMemcpyDeviceToHost);
      if (FILE* f = fopen(dump, "wb")) { fwrite(hs.data(), 8, hs.size(), f); fclose(f); }
    }
#endif
  }
  if ((phase & 2) && a.og > 0) {
    if constexpr (C > 0) {
      const int threads = graph_update_threads(h);
      const size_t lds = sizeof(float) * (size_t)graph_update_lds_floats(C, a.dg, a.og, threads);
      ProfScope ps("k_graph_t", s);
      GNX_LAUNCH((k_graph_t<C, ONEG, BF16, BF16 && !LN>), dim3((unsigned)a.G, (unsigned)R), dim3(threads), lds, s, a, n_rows);
      GNX_HIP(hipGetLastError());
    }
  }
  return GNX_OK;
}

// A run of Z steps of gnx_block_forward_steps (a.ef ... a.partials unused: the slots of `t`): every slot's edge + node update in one launch
// (k_block_wave_run, slot-major: x fastest), then every slot's graph update in a second one right behind it, with k_graph_t's thread count.
// phase: GNX_PHASE_EDGE_NODE alone leaves the graph updates to a later launch (the next run's front, or this function with GNX_PHASE_GRAPH).
template <int DE, int DN, int DG, int OE, int ON, bool ONEG, bool BF16 = false>
static int32_t launch_wave_run(const gnx_graphs* h, const BlockArgs& a, const RunTable& t, int Z, hipStream_t s, int phase = 3) {
  constexpr int C = OE + ON;
  if (Z < 1 || Z > kRunSlots) return fail(GNX_ERR_INVALID_ARG, "internal: a run of more steps than the table has slots");
  const int n_rows = partial_rows(h);
  if (phase & 1) {
    ProfScope ps("k_block_wave", s);
    GNX_LAUNCH((k_block_wave_run<DE, DN, DG, OE, ON, 2, ONEG, BF16>), dim3((unsigned)((a.n_wtiles + 3) / 4), (unsigned)Z), dim3(kThreads), 0, s, a, t, n_rows);
    GNX_HIP(hipGetLastError());
  }
  if ((phase & 2) && a.og > 0) {
    const int threads = graph_update_threads(h);
    const size_t lds = sizeof(float) * (size_t)graph_update_lds_floats(C, a.dg, a.og, threads);
    ProfScope ps("k_graph_t", s);
    GNX_LAUNCH((k_graph_run<C, ONEG, BF16>), dim3((unsigned)a.G, (unsigned)Z), dim3(threads), lds, s, a, t, n_rows);
    GNX_HIP(hipGetLastError());
  }
  return GNX_OK;
}

// A run of Z steps whose launch also carries the graph updates of the run before it (k_block_wave_carry; fp32 rows) in a.prev_blocks front
// workgroups per row.  The block launch only: this run's own graph updates are pending afterwards.
template <int DE, int DN, int DG, int OE, int ON, bool ONEG>
static int32_t launch_wave_carry(const gnx_graphs* h, const BlockArgs& a0, const RunTable& t, int Z, const PrevTable& prev0, hipStream_t s) {
  if (Z < 1 || Z > kRunSlots || prev0.n < 1 || prev0.n > kRunSlots) return fail(GNX_ERR_INVALID_ARG, "internal: a run of more steps than the table has slots");
  BlockArgs a = a0;
  PrevTable prev = prev0;
  prev.per_slot = h->G == 1 ? 1 : (int)((h->G + 3) / 4);
  // The front (gnx_wave_kernel.h: CHAIN with RUN).  One graph: the previous run's slot x in the x-th workgroup behind the tiles of row 0.
  // Several graphs: per_slot workgroups per slot in front of the tiles, slots y, y + Z, ... in row y.  Rounded up to a multiple of 8 (the
  // workgroups beyond return at once): workgroup x + gridDim.x * y goes to XCD (x + gridDim.x * y) % 8, so a front that is no multiple of
  // 8 would shift a tile's XCD from slot to slot; with it the slots of a tile meet in one L2, as in k_block_wave_run.
  a.prev_blocks = ((h->G == 1 ? prev.n : prev.per_slot * ((prev.n + Z - 1) / Z)) + 7) / 8 * 8;
  const int n_rows = partial_rows(h);
  ProfScope ps("k_block_wave", s);
  GNX_LAUNCH((k_block_wave_carry<DE, DN, DG, OE, ON, 2, ONEG>), dim3((unsigned)((a.n_wtiles + 3) / 4) + (unsigned)a.prev_blocks, (unsigned)Z), dim3(kThreads), 0, s, a, t,
             prev, n_rows);
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

// Batches of small graphs (every graph <= 8 wave tiles: the handle has a pack table): ONE launch — 512-thread workgroups that own whole
// graphs run the graph update themselves (k_block_wave<..., PACK>).  Only for the whole block in one call (phase 3): a caller that
// splits off the graph update, or a narrow GNCore that runs it inside its FeedForward launch, reads the partial rows of the two-launch form.
// GNX_FLAG_NO_PACK keeps the two launches.
template <int DE, int DN, int DG, int OE, int ON, int EPT, bool BF16 = false>
static bool launch_wave_pack(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, int phase, int32_t* rc) {
  constexpr int C = OE + ON;
  if constexpr (EPT != 2 || C == 0) return false;
  else {
    if (h->G <= 1 || h->n_packs <= 0 || !a.packs || phase != 3 || a.og <= 0 || form(GNX_FLAG_NO_PACK)) return false;
    ProfScope ps("k_block_wave", s);
    GNX_LAUNCH((k_block_wave<DE, DN, DG, OE, ON, EPT, false, false, true, false, false, BF16>), dim3((unsigned)h->n_packs, (unsigned)R), dim3(kPackThreads), 0, s, a, 0);
    const hipError_t e = hipGetLastError();
    *rc = e == hipSuccess ? GNX_OK : hip_fail(e, "k_block_wave<PACK>");
    return true;
  }
}

template <int DE, int DN, int DG, int OE, int ON, int EPT, bool LN = false, bool BF16 = false>
static int32_t launch_wave_t(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, int phase) {
  if constexpr (!LN) {
    int32_t rc = GNX_OK;
    if (launch_wave_pack<DE, DN, DG, OE, ON, EPT, BF16>(h, a, R, s, phase, &rc)) return rc;
  }
  return h->G == 1 ? launch_wave_g<DE, DN, DG, OE, ON, EPT, LN, true, false, false, BF16>(h, a, R, s, phase)
                   : launch_wave_g<DE, DN, DG, OE, ON, EPT, LN, false, false, false, BF16>(h, a, R, s, phase);
}

template <int DE, int DN, int DG, int OE, int ON, bool BF16 = false>
static int32_t launch_fused(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, int phase) {
  // the kernel's EPT must match the handle's wave-tile edge cap (GNX_WTILE_E at handle creation: 64, 128 or 256)
  if (h->wtile_e_cap == 64) return launch_wave_t<DE, DN, DG, OE, ON, 1, false, BF16>(h, a, R, s, phase);
  if (h->wtile_e_cap == 128) return launch_wave_t<DE, DN, DG, OE, ON, 2, false, BF16>(h, a, R, s, phase);
  if (h->wtile_e_cap == 256) {
    if constexpr (narrow_cap_ok(DE, DN, 256)) return launch_wave_t<DE, DN, DG, OE, ON, 4, false, BF16>(h, a, R, s, phase);
  }
  return 1;
}

// ---- the table's one expansion site ----
// f(S{}) for the row S of the element type's list (gnx_narrow_sets.h) with a's widths: S::DE .. S::ON and S::forms are constants, so f picks
// its instantiation with `if constexpr (S::forms & NF_...)` and a form a row lacks is never compiled.  1: no row (or f had no kernel).
template <class F, class... S>
static int32_t narrow_set_dispatch_in(NarrowSetList<S...>, const BlockArgs& a, F&& f) {
  int32_t rc = 1;
  (void)((S::is(a.de, a.dn, a.dg, a.oe, a.on) && ((rc = f(S{})), true)) || ...);
  return rc;
}
template <bool BF16, class F>
static int32_t narrow_set_dispatch(const BlockArgs& a, F&& f) {
  if constexpr (BF16) return narrow_set_dispatch_in(NarrowSetsBF16{}, a, f);
  else return narrow_set_dispatch_in(NarrowSetsF32{}, a, f);
}

// The launchers by form; each returns 1 where the set, or the set at this batch or wave-tile size, has no such kernel.
// NF_PLAIN: the block — whole (phase 3), one launch of the two, or only the graph update from partial rows a chained launch left.
template <bool BF16>
static int32_t launch_narrow_plain(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, int phase) {
  return narrow_set_dispatch<BF16>(a, [&](auto set) -> int32_t {
    using S = decltype(set);
    if constexpr (S::forms & NF_PLAIN) return launch_fused<S::DE, S::DN, S::DG, S::OE, S::ON, BF16>(h, a, R, s, phase);
    return 1;
  });
}
// NF_PLAIN, chained: this call's edge + node update with a.prev_* (the previous call's pending graph update) at the front of the launch.
template <bool BF16>
static int32_t launch_narrow_chained(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s) {
  return narrow_set_dispatch<BF16>(a, [&](auto set) -> int32_t {
    using S = decltype(set);
    if constexpr (S::forms & NF_PLAIN)
      return h->G == 1 ? launch_wave_g<S::DE, S::DN, S::DG, S::OE, S::ON, 2, false, true, false, true, BF16>(h, a, R, s, 1)
                       : launch_wave_g<S::DE, S::DN, S::DG, S::OE, S::ON, 2, false, false, false, true, BF16>(h, a, R, s, 1);
    return 1;
  });
}
// NF_RUN1 / NF_RUNG: a run of Z steps in one launch plus one for their graph updates.
template <bool BF16>
static int32_t launch_narrow_run(const gnx_graphs* h, const BlockArgs& a, const RunTable& t, int Z, hipStream_t s, int phase) {
  return narrow_set_dispatch<BF16>(a, [&](auto set) -> int32_t {
    using S = decltype(set);
    if (h->G == 1) {
      if constexpr (S::forms & NF_RUN1) return launch_wave_run<S::DE, S::DN, S::DG, S::OE, S::ON, true, BF16>(h, a, t, Z, s, phase);
    } else {
      if constexpr (S::forms & NF_RUNG) return launch_wave_run<S::DE, S::DN, S::DG, S::OE, S::ON, false, BF16>(h, a, t, Z, s, phase);
    }
    return 1;
  });
}
// NF_LN / NF_FFE (a.ffe_w1 set): LayerNorm on load — with BF16 the block of a bf16 core: gn1 applied to the bf16 rows as they are loaded, the
// block's outputs leave as fp32 (a.nf_out, a.gf_out and, without the FeedForward in the edge lanes, a.ef_out are fp32 staging); with
// a.ffe_w1 the edge lanes finish the core's edge rows and store them, rounded once, as bf16 (a.ef_out is then the caller's).
template <bool BF16>
static int32_t launch_narrow_ln(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, int phase) {
  if (h->wtile_e_cap != 128) return 1;
  return narrow_set_dispatch<BF16>(a, [&](auto set) -> int32_t {
    using S = decltype(set);
    if (a.ffe_w1) {
      if constexpr (S::forms & NF_FFE)
        return h->G == 1 ? launch_wave_g<S::DE, S::DN, S::DG, S::OE, S::ON, 2, true, true, true, false, BF16>(h, a, R, s, phase)
                         : launch_wave_g<S::DE, S::DN, S::DG, S::OE, S::ON, 2, true, false, true, false, BF16>(h, a, R, s, phase);
    } else {
      if constexpr (S::forms & NF_LN) return launch_wave_t<S::DE, S::DN, S::DG, S::OE, S::ON, 2, true, BF16>(h, a, R, s, phase);
    }
    return 1;
  });
}

}  // namespace gnx
