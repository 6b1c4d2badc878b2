// GNBlock with Chain update functions at narrow widths, the edge and the node function in ONE kernel (gnx_chain_block_forward_wave, gnx_chain.cpp;
// the rule: chain_wave_takes, gnx_chain_plan.h).
//
//   k_chain_wave<W>       : ONE WAVEFRONT PER WAVE TILE — a contiguous node range of one graph (<= 64 nodes) and its contiguous in-edges
//                           (<= wtile_e_cap: the rule admits a batch only when every tile is one such chunk).  A workgroup is `waves` (4 or 2)
//                           independent waves; the one workgroup barrier stands behind the staging of both functions' parameters in LDS
//                           (chain_stage_params: the edge function's, the node function's behind them), read as uniform ds_read_b128 broadcasts.
//     lanes as EDGES        el = lane, lane + 64, ... < ne: the lane builds [ef[e] ; nf[src] ; nf[dst] ; gf[g]] in registers (g from the tile
//                           record: no search), runs every layer (chain_layer_fw: k_chain_mlp's arithmetic, so ef' keeps the bits of
//                           gnx_chain_block_forward_narrow), stores the row to ef_out AND to the wave's LDS slice [cap][stride].
//                           stride = oe | 1 (odd): lanes that read or write 64 different rows at one column fall into different banks —
//                           an odd stride is coprime to the bank count.
//     lanes as NODES        lane n < nn sums its in-edges' rows from LDS sequentially in CSC order (the adds of chain_input_row<., SRC_NODE>: the
//                           same bits), appends nf[n] and gf[g], runs the node function's layers and stores nf'.
//     the partial row       (a block with a graph function) [column sums of the tile's ef' ; of its nf']: each lane adds its own rows in edge
//                           order (re-read from LDS, when the edge registers are free), the node lanes hold one row each; one fixed tree per
//                           column (wave_sum: DPP + 4 readlanes); lane k stores column k of partials[r][tile][oe + on].  No atomics.
//   k_chain_graph_wave<W> : the graph function from the partial rows, one workgroup per graph (and replica) with k_graph_t's geometry (64 threads
//                           while every graph has <= 256 partial rows, 256 above, 1024 from 1024 rows on).  The graph's rows are one contiguous
//                           run of floats: thread t < S = (T / C) C adds the elements t, t + S, ... (one column, four loads in flight), the
//                           S / C per-thread sums of a column are added in thread order by thread c.  Wave 0 then holds
//                           [sum ef' ; sum nf' ; gf[g]] in registers, runs the graph function's layers from LDS and stores gf'.
//
// W in {8, 16, 32}: ONE register width per launch, the smallest that covers the input and layer widths of the functions the kernel runs (three
// instantiations per kernel, not nine): the edge and the node phase follow each other in one wave, so the kernel's registers are those of the
// wider phase under either scheme, and a layer's products are skipped by groups of four behind wave-uniform tests — a narrow function in a
// wide instantiation pays branches, not products (profiles/chain_wave_resources.json).  The bits do not depend on W: the padding is exactly 0.
// Every global access is one dword: feature pointers may be 4-byte aligned only.  Offsets are size_t.
#include "gnx_chain_mlp.h"

namespace gnx {

struct ChainWaveArgs {
  ChainMlpArgs e, n;  // the edge / node function: layers, K and the feature pointers (e: ef, nf, gf of widths d0, d1, d2; n.d0 = oe)
  const Tile* wtiles;
  int n_wtiles, waves, cap, stride;  // waves per workgroup; the LDS slice of a wave: [cap][stride] floats
  int par_e, par_all;                // floats of the edge function's / of both functions' staged parameters
  float *ef_out, *nf_out;
  float* partials;                   // [R][n_wtiles][oe + on], or nullptr (no graph function)
  int oe, on;
};

template <int W>
__global__ __launch_bounds__(256) void k_chain_wave(ChainWaveArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const int NT = 64 * a.waves;
  chain_stage_params(a.e, s_mem, NT);
  chain_stage_params(a.n, s_mem + a.par_e, NT);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wt = blockIdx.x * a.waves + wave;
  if (wt >= a.n_wtiles) return;  // wave-uniform
  const size_t r = blockIdx.y;
  const Tile t = a.wtiles[wt];
  const int ne = t.e1 - t.e0, nn = t.n1 - t.n0, oe = a.oe, on = a.on, stride = a.stride;
  float* __restrict__ s_ef = s_mem + a.par_all + wave * (a.cap * stride);
  const float* __restrict__ gfr = a.e.a2 + (r * (size_t)a.e.G + t.g) * a.e.d2;

  // ---- lanes as edges ----
  for (int base = 0; base < ne; base += 64) {  // (wave-uniform trips: every lane runs the layers, a lane beyond the tile on a zero row)
    const int el = base + lane;
    const bool live = el < ne;
    float cur[W];
#pragma unroll
    for (int k = 0; k < W; ++k) cur[k] = 0.f;
    if (live) {
      const int e = t.e0 + el;
      if (a.e.d0 > 0) chain_load_seg<W>(a.e.a0 + (r * (size_t)a.e.E + e) * a.e.d0, 0, a.e.d0, cur);
      if (a.e.d1 > 0) {
        chain_load_seg<W>(a.e.a1 + (r * (size_t)a.e.N + a.e.rowval[e]) * a.e.d1, a.e.d0, a.e.d1, cur);
        chain_load_seg<W>(a.e.a1 + (r * (size_t)a.e.N + a.e.edge_dst[e]) * a.e.d1, a.e.d0 + a.e.d1, a.e.d1, cur);
      }
      if (a.e.d2 > 0) chain_load_seg<W>(gfr, a.e.d0 + 2 * a.e.d1, a.e.d2, cur);
    }
    int off = 0, kin = a.e.K;
#pragma unroll 1
    for (int l = 0; l < a.e.n_layers; ++l) {
      off = chain_layer_fw<W>(s_mem, off, kin, a.e.layer[l].width, a.e.layer[l].op, cur);
      kin = a.e.layer[l].width;
    }
    if (live) {
      float* __restrict__ o = a.ef_out + (r * (size_t)a.e.E + (t.e0 + el)) * (size_t)oe;
      float* __restrict__ so = s_ef + el * stride;
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (k < oe) { o[k] = cur[k]; so[k] = cur[k]; }
    }
  }
  // the slice is read by other lanes of this wave than wrote it: LDS operations of one wave execute in order
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  // ---- the partial row's edge half: own rows in edge order, one tree per column ----
  float* __restrict__ prow = a.partials ? a.partials + (r * (size_t)a.n_wtiles + wt) * (size_t)(oe + on) : nullptr;
  if (prow) {
    float pe[W];
#pragma unroll
    for (int k = 0; k < W; ++k) pe[k] = 0.f;
    for (int base = 0; base < ne; base += 64) {
      const int el = base + lane;
      if (el < ne) {
        const float* __restrict__ so = s_ef + el * stride;
#pragma unroll
        for (int k = 0; k < W; ++k)
          if (k < oe) pe[k] += so[k];
      }
    }
    float mine = 0.f;
#pragma unroll
    for (int k = 0; k < W; ++k)
      if (k < oe) { const float tot = wave_sum(pe[k]); mine = lane == k ? tot : mine; }
    if (lane < oe) prow[lane] = mine;
  }

  // ---- lanes as nodes ----
  const bool live = lane < nn;
  const int node = t.n0 + lane;
  float cur[W];
#pragma unroll
  for (int k = 0; k < W; ++k) cur[k] = 0.f;
  if (live) {
    const int c1 = a.n.colptr[node + 1] - t.e0;
    for (int i = a.n.colptr[node] - t.e0; i < c1; ++i) {
      const float* __restrict__ so = s_ef + i * stride;
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (k < oe) cur[k] += so[k];
    }
    if (a.n.d1 > 0) chain_load_seg<W>(a.n.a1 + (r * (size_t)a.n.N + node) * a.n.d1, oe, a.n.d1, cur);
    if (a.n.d2 > 0) chain_load_seg<W>(gfr, oe + a.n.d1, a.n.d2, cur);
  }
  int off = a.par_e, kin = a.n.K;
#pragma unroll 1
  for (int l = 0; l < a.n.n_layers; ++l) {
    off = chain_layer_fw<W>(s_mem, off, kin, a.n.layer[l].width, a.n.layer[l].op, cur);
    kin = a.n.layer[l].width;
  }
  if (live) {
    float* __restrict__ o = a.nf_out + (r * (size_t)a.n.N + node) * (size_t)on;
#pragma unroll
    for (int k = 0; k < W; ++k)
      if (k < on) o[k] = cur[k];
  }
  if (prow) {
    float mine = 0.f;
#pragma unroll
    for (int k = 0; k < W; ++k)
      if (k < on) { const float tot = wave_sum(live ? cur[k] : 0.f); mine = lane == k ? tot : mine; }
    if (lane < on) prow[oe + lane] = mine;
  }
}

struct ChainGraphWaveArgs {
  ChainMlpArgs f;          // the graph function: layers and K = oe + on + dg
  const float* partials;   // [R][n_wtiles][C]
  const float* gf;         // [R][G][dg]
  float* gf_out;           // [R][G][og]
  const int* wtile_off;    // [G + 1]
  int n_wtiles, C, dg, og, G, par;  // par: floats of the staged parameters
};

template <int W>
__global__ __launch_bounds__(1024) void k_chain_graph_wave(ChainGraphWaveArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const int T = blockDim.x, tid = threadIdx.x, C = a.C;
  float* __restrict__ s_red = s_mem + a.par;  // [T] per-thread sums, then [C + dg] the function's input row
  float* __restrict__ s_x = s_red + T;
  chain_stage_params(a.f, s_mem, T);
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
  if (tid < C) {
    float s = 0.f;
    for (int q = tid; q < S; q += C) s += s_red[q];
    s_x[tid] = s;
  } else if (tid < C + a.dg) {
    s_x[tid] = a.gf[(r * (size_t)a.G + g) * a.dg + (tid - C)];
  }
  __syncthreads();
  if (tid >= 64) return;
  float cur[W];
#pragma unroll
  for (int k = 0; k < W; ++k) cur[k] = k < a.f.K ? s_x[k] : 0.f;
  int off = 0, kin = a.f.K;
#pragma unroll 1
  for (int l = 0; l < a.f.n_layers; ++l) {
    off = chain_layer_fw<W>(s_mem, off, kin, a.f.layer[l].width, a.f.layer[l].op, cur);
    kin = a.f.layer[l].width;
  }
  if (tid == 0) {
    float* __restrict__ o = a.gf_out + (r * (size_t)a.G + g) * (size_t)a.og;
#pragma unroll
    for (int k = 0; k < W; ++k)
      if (k < a.og) o[k] = cur[k];
  }
}

// The edge + node launch and (a block with a graph function) the finishing launch.  The caller asked chain_wave_takes; `partials`: R n_wtiles
// (oe + on) floats of the workspace.  The profiler names are the narrow entry's: the block launch reports as the edge function's, the
// finishing launch as the graph function's.
int32_t launch_chain_wave(const gnx_graphs* h, const gnx_chain_block_params& p, const ChainShape& sh, const float* ef, const float* nf, const float* gf, float* ef_out,
                          float* nf_out, float* gf_out, float* partials, int64_t R, hipStream_t s) {
  const int oe = sh.ow[0], on = sh.ow[1], og = sh.ow[2];
  ChainWaveArgs a{};
  int we, wn;
  size_t rows;
  if (int32_t rc = chain_mlp_prologue(h, 0, p.edgefn, ef, p.de, nf, p.dn, gf, p.dg, CHAIN_RULE_FW, "launch_chain_wave", s, a.e, &we, &rows)) return rc;
  if (int32_t rc = chain_mlp_prologue(h, 1, p.nodefn, ef_out, oe, nf, p.dn, gf, p.dg, CHAIN_RULE_FW, "launch_chain_wave", s, a.n, &wn, &rows)) return rc;
  a.waves = chain_wave_waves(sh, h->wtile_e_cap);
  if (a.waves < 2 || h->max_in_degree > h->wtile_e_cap) return fail(GNX_ERR_INVALID_ARG, "launch_chain_wave: the block is outside the wave rule");
  a.wtiles = h->d_wtiles; a.n_wtiles = (int)h->n_wtiles();
  a.cap = h->wtile_e_cap; a.stride = chain_wave_stride(oe);
  a.par_e = (int)chain_narrow_lds_floats(p.edgefn, sh.k0[0]);
  a.par_all = a.par_e + (int)chain_narrow_lds_floats(p.nodefn, sh.k0[1]);
  a.ef_out = ef_out; a.nf_out = nf_out; a.partials = og > 0 ? partials : nullptr;
  a.oe = oe; a.on = on;
  {
    const dim3 grid((unsigned)((a.n_wtiles + a.waves - 1) / a.waves), (unsigned)R);
    const size_t lds = sizeof(float) * ((size_t)a.par_all + (size_t)a.waves * a.cap * a.stride);
    ProfScope ps("k_rows_gemm_chain_e", s);
    const int w = std::max(we, wn);
    if (w <= 8) GNX_LAUNCH((k_chain_wave<8>), grid, dim3(64 * a.waves), lds, s, a);
    else if (w <= 16) GNX_LAUNCH((k_chain_wave<16>), grid, dim3(64 * a.waves), lds, s, a);
    else GNX_LAUNCH((k_chain_wave<32>), grid, dim3(64 * a.waves), lds, s, a);
    GNX_HIP(hipGetLastError());
  }
  if (og <= 0) return GNX_OK;
  ChainGraphWaveArgs b{};
  int wg;
  if (int32_t rc = chain_mlp_prologue(h, 2, p.graphfn, partials, sh.k0[2], nullptr, 0, nullptr, 0, CHAIN_RULE_FW, "launch_chain_wave", s, b.f, &wg, &rows)) return rc;
  b.partials = partials; b.gf = gf; b.gf_out = gf_out; b.wtile_off = h->d_wtile_off;
  b.n_wtiles = a.n_wtiles; b.C = oe + on; b.dg = p.dg; b.og = og; b.G = (int)h->G;
  b.par = (int)chain_narrow_lds_floats(p.graphfn, sh.k0[2]);
  const int threads = graph_update_threads_for_rows(h->max_wtiles_per_graph);
  const size_t lds = sizeof(float) * ((size_t)b.par + threads + 64);
  ProfScope ps("k_rows_gemm_chain_g", s);
  const dim3 grid((unsigned)h->G, (unsigned)R);
  if (wg <= 8) GNX_LAUNCH((k_chain_graph_wave<8>), grid, dim3(threads), lds, s, b);
  else if (wg <= 16) GNX_LAUNCH((k_chain_graph_wave<16>), grid, dim3(threads), lds, s, b);
  else GNX_LAUNCH((k_chain_graph_wave<32>), grid, dim3(threads), lds, s, b);
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
