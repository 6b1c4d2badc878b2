// The pullback of a GNBlock with Chain update functions at narrow widths in the wave form (gnx_chain_block_backward_wave, gnx_backward.hip; the
// rule and the LDS plan: chain_bw_wave_takes / chain_bw_wave_shape, gnx_chain_plan.h).  A wave tile owns a contiguous node range of one graph
// (<= 64 nodes) and EVERY in-edge of those nodes (<= wtile_e_cap, one chunk: the rule), so what the narrow pullback sends through memory between
// its launches — the recomputed ef' and nf', ef' again per node, the node rows' input-gradient columns [0, oe) and their gather per edge —
// stays inside one wavefront's LDS.
//
//   k_chain_wave_partials<W>  : (a block with a graph function) k_chain_wave's forward (gnx_chain_wave.hip: its text, its summation orders)
//                               without the stores of ef' and nf': only partials[r][tile][oe + on], the tile's column sums, reach memory.
//   k_chain_graph_rows_wave   : one workgroup per graph and replica with k_chain_graph_wave's geometry and summation order; writes the graph
//                               function's input row [sum ef' ; sum nf' ; gf[g]] into Xg.  The graph level then runs as k_chain_mlp_bw<., SRC_ROWS>.
//   k_chain_wave_bw<W>        : ONE WAVEFRONT PER WAVE TILE, the node function's and the edge function's pullbacks.  Per workgroup: both
//                               functions' parameters in LDS behind the one workgroup barrier (chain_stage_params).  Per wave: a tape of 64 rows
//                               (ld floats each, ld odd: a lane's own row falls into its own bank), P_e + P_n accumulators, a slice [cap][oe | 1].
//     (a) lanes as EDGES        per chunk of 64: [ef ; nf[src] ; nf[dst] ; gf[g]] through the edge function (chain_layer_fw); ef' into the slice only.
//     (b) lanes as NODES        the in-edges' rows summed from the slice in CSC order, nf[n] and gf[g] appended; forward onto the tape; the last
//                               delta from g_nf_out + dXg[g][oe : oe + on]; back through the layers in registers (k_chain_mlp_bw's arithmetic),
//                               chain_bw_dw_phase per layer into the node accumulators.  Columns [oe, Kn) of the row's input gradient go to the
//                               workspace as [R N][dn + dg] (add_cols / colsum_graphs read them); columns [0, oe) overwrite the slice as row
//                               `lane` — they never reach memory.
//     (c) lanes as EDGES again  per chunk: the input row again, forward onto the tape; the last delta from g_ef_out + dXg[g][0 : oe] + the slice
//                               row dst - n0; back; the parameter-gradient phase into the edge accumulators; d_ef stored directly, the
//                               2 dn + dg node and graph columns into the compact dXe (k_bw_dnf and the d_gf column sums read it).
//     (d) finish                the workgroup's waves add their accumulators in wave order: one partial row per workgroup and layer, which
//                               k_bw_dw_final finishes (nwg = ceil(wave tiles / waves) per replica).
// No atomics; every accumulator starts at 0 and every sum has one fixed order: the bits do not depend on what the workspace held.  A last-layer
// gelu differentiates from its pre-activation.  Every global access is one dword (4-byte aligned buffers are enough); offsets are size_t.
// Register arrays are indexed by unrolled constants only: no instantiation uses scratch (profiles/chain_bw_wave_resources.json).
// k_chain_wave_partials and k_chain_wave_bw are one text with their bf16 twins (gnx_chain_bw_wave_kernel.h, which this file compiles with
// BF16 = false); k_chain_graph_rows_wave reads fp32 rows for both.
#define GNX_CHAIN_BW_WAVE_NAME(x) x  // k_chain_wave_partials, k_chain_wave_bw, launch_chain_wave_partials, launch_chain_wave_bw
#define GNX_CHAIN_BW_WAVE_BF16 false
#include "gnx_chain_bw_wave_kernel.h"

namespace gnx {

// ---- (2) the graph function's input rows from the partial rows ----
struct ChainGraphRowsArgs {
  const float* partials;  // [R][n_wtiles][C]
  const float* gf;        // [R][G][dg]
  float* xg;              // [R][G][C + dg]
  const int* wtile_off;   // [G + 1]
  int n_wtiles, C, dg, G;
};

__global__ __launch_bounds__(1024) void k_chain_graph_rows_wave(ChainGraphRowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_red[];  // [T] per-thread sums
  const int T = blockDim.x, tid = threadIdx.x, C = a.C;
  const int g = blockIdx.x;
  const size_t r = blockIdx.y;
  const int S = (T / C) * C;  // threads that add: thread t keeps column t % C
  const size_t n = (size_t)(a.wtile_off[g + 1] - a.wtile_off[g]) * C;
  const float* __restrict__ p = a.partials + (r * (size_t)a.n_wtiles + a.wtile_off[g]) * (size_t)C;
  float acc = 0.f;
  if (tid < S) {
    size_t i = tid;
    for (; i + 3 * (size_t)S < n; i += 4 * (size_t)S) {  // four loads in flight, added in element order
      const float x0 = p[i], x1 = p[i + S], x2 = p[i + 2 * (size_t)S], x3 = p[i + 3 * (size_t)S];
      acc += x0; acc += x1; acc += x2; acc += x3;
    }
    for (; i < n; i += S) acc += p[i];
  }
  s_red[tid] = acc;
  __syncthreads();
  float* __restrict__ o = a.xg + (r * (size_t)a.G + g) * (size_t)(C + a.dg);
  if (tid < C) {
    float s = 0.f;
    for (int q = tid; q < S; q += C) s += s_red[q];
    o[tid] = s;
  } else if (tid < C + a.dg) {
    o[tid] = a.gf[(r * (size_t)a.G + g) * a.dg + (tid - C)];
  }
}

int32_t launch_chain_graph_rows_wave(const gnx_graphs* h, const ChainShape& sh, const float* partials, const float* gf, float* xg, int64_t R, hipStream_t s) {
  ChainGraphRowsArgs a{partials, gf, xg, h->d_wtile_off, (int)h->n_wtiles(), sh.ow[0] + sh.ow[1], sh.dg, (int)h->G};
  const int threads = std::max(graph_update_threads_for_rows(h->max_wtiles_per_graph), (a.C + a.dg + 63) / 64 * 64);
  GNX_LAUNCH(k_chain_graph_rows_wave, dim3((unsigned)h->G, (unsigned)R), dim3(threads), sizeof(float) * threads, s, a);
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
