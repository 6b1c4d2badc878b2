// The edge level of the GNBlock backward at narrow widths, in one kernel (gnx_block_backward_fused, gnx_block_backward_narrow).  Self-contained
// device code like gnx_wave_kernel.h: included by gnx_backward_narrow.hip for the ahead-of-time instantiations AND part of the source text
// gnx_jit.cpp compiles at run time (any other eligible width set), so it depends on gnx_device.h / gnx_wave_kernel.h only.
//
// The generic edge level (gnx_backward.hip, where the matrix cores do not take it) materialises Xe [R*E][Ke], writes delta_e [R*E][oe], writes
// all of dXe [R*E][Ke] with d_ef on top of it, and reads Xe and delta_e again for the weight gradient.  Here a wavefront owns one wave tile of
// the handle — a contiguous, dst-sorted edge range of one graph (Tile, gnx_device.h) — and walks it 64 edges at a time, one edge per lane:
// the edge's input row, its delta and its dXe row live in registers; the ef columns of dXe go to d_ef and nowhere else, the other columns to
// a compact tensor dXe_c [R*E][2*dn + dg] that k_bw_dnf and the d_gf column sums read; Xe and delta_e never reach memory.  The weight and
// bias gradient: the wave parks the chunk's rows in its own LDS slice and lane l adds the chunk's edges in edge order for the pairs
// p = k * OE + j (k == Ke: the bias) of its slots, p = l and — where P = OE (Ke + 1) exceeds 64 — p = l + 64, one accumulator per slot that
// lives across the chunks of the tile; a workgroup adds its four waves in wave order and writes one row partial[r][workgroup][P] in the pair
// order of k_bw_dw_partial, which k_bw_dw_final finishes.  No atomics, every sum in a fixed order.
//
// delta and dXe are computed by the operations of k_bw_delta (kind 2) and k_bw_dx in their order, so d_ef and dXe_c carry the bits of the
// generic form; only the weight / bias gradient is summed in another order.
//
// Element type (BF16: GNX_ELEM_BF16): ef, nf, gf, g_ef_out, ef_out and d_ef hold bfloat16 — declared float in BwEdgeWave like the feature
// pointers of BlockArgs.  A bf16 element is widened on load (exact) and d_ef is rounded to nearest even once on store; dXg, dXn, We, dXe_c,
// the LDS rows, the partial rows and every instruction between load and store are the fp32 kernel's.  One form for every address: fp32
// tensors by dword accesses, bf16 tensors by one 16-bit access per element of the lane's own row (ld_feat / st_feat, as the generic typed
// kernels) — a lane never touches the other half of a dword, so rows that start in the middle of one need no special case.
// The body is one template; the fp32 kernel keeps its name and its four width parameters, the bf16 kernel is k_bw_edge_wave_bf16.
#pragma once
#include "gnx_device.h"
#include "gnx_wave_kernel.h"  // ld_feat / st_feat, feat

namespace gnx {

struct BwEdgeWave {
  const float *ef, *nf, *gf;       // the forward's inputs, replica 0
  const float *g_ef_out, *ef_out;  // upstream gradient of the edges (or nullptr) and the forward's edge output
  const float* dXg; int Kg;        // the graph level's dX rows [R][G][Kg] (edge columns first) or nullptr
  const float* dXn; int Kn;        // the node level's dX rows [R][N][Kn] (edge columns first) or nullptr
  const float* We; int act;
  float* d_ef;     // [R][E][de] or nullptr
  float* dXe_c;    // [R][E][2 dn + dg]: the columns of dXe behind the ef segment, or nullptr
  float* partial;  // [R][bw_edge_wave_rows][oe (Ke + 1)] or nullptr (neither dWe nor dbe wanted)
  const Tile* wtiles; int n_wtiles;
  const int *rowval, *edge_dst;
  int N, E, G;
};

// one element of a typed row
__device__ __forceinline__ float ld_row(const float* p, size_t i) { return p[i]; }
__device__ __forceinline__ float ld_row(const bf16_t* p, size_t i) { return bf16_lo(p[i]); }

template <int DE, int DN, int DG, int OE, bool BF16>
__device__ __forceinline__ void bw_edge_wave(BwEdgeWave a) {
  constexpr int KE = DE + 2 * DN + DG, CW = 2 * DN + DG, P = OE * (KE + 1);
  constexpr int PS = (P + 63) / 64;  // pair slots of a lane: lane l sums the pairs l and (PS == 2) l + 64
  constexpr int LD = (OE + KE) | 1;  // odd row length: the lanes' row writes fall on 64 different banks
  static_assert(PS <= 2, "at most two (k, j) pairs per lane");
  static_assert(KE > 0 && OE > 0, "an edge function with inputs and outputs");
  __shared__ float s_rows[4][64 * LD];  // per wave: [edge of the chunk][Xe row ; delta row]
  __shared__ float s_acc[4][64 * PS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wt = blockIdx.x * 4 + wave;
  const size_t r = blockIdx.y;
  int pk[PS], pj[PS];  // the pairs this lane sums (slot q: lane + 64 q < P)
#pragma unroll
  for (int q = 0; q < PS; ++q) { pk[q] = (lane + 64 * q) / OE; pj[q] = (lane + 64 * q) % OE; }
  float w[KE * OE];  // read before the kernel's first store: uniform, scalar loads
#pragma unroll
  for (int i = 0; i < KE * OE; ++i) w[i] = a.We[i];
  float wacc[PS];
#pragma unroll
  for (int q = 0; q < PS; ++q) wacc[q] = 0.f;
  if (wt < a.n_wtiles) {  // wave-uniform
    const Tile t = a.wtiles[wt];
    float* const rows = s_rows[wave];
    const auto* const ef = feat<BF16>(a.ef) + r * (size_t)a.E * DE;  // (float or bf16_t rows)
    const auto* const nf = feat<BF16>(a.nf) + r * (size_t)a.N * DN;
    const auto* const gfr = feat<BF16>(a.gf) + (r * (size_t)a.G + t.g) * DG;
    const float* const dxg = a.dXg ? a.dXg + (r * (size_t)a.G + t.g) * a.Kg : nullptr;
    for (int c0 = t.e0; c0 < t.e1; c0 += 64) {
      const int cnt = min(64, t.e1 - c0);
      const bool live = lane < cnt;
      const int e = c0 + (live ? lane : cnt - 1);  // clamped: unconditional loads, guarded stores
      const size_t re = r * (size_t)a.E + e;
      const int src = a.rowval[e], dst = a.edge_dst[e];
      float x[KE], d[OE];
#pragma unroll
      for (int k = 0; k < DE; ++k) x[k] = ld_row(ef, (size_t)e * DE + k);
#pragma unroll
      for (int k = 0; k < DN; ++k) x[DE + k] = ld_row(nf, (size_t)src * DN + k);
#pragma unroll
      for (int k = 0; k < DN; ++k) x[DE + DN + k] = ld_row(nf, (size_t)dst * DN + k);
#pragma unroll
      for (int k = 0; k < DG; ++k) x[DE + 2 * DN + k] = ld_row(gfr, k);
#pragma unroll
      for (int j = 0; j < OE; ++j) {  // k_bw_delta, kind 2
        float g = a.g_ef_out ? ld_feat<BF16>(a.g_ef_out, re * OE + j) : 0.f;
        if (dxg) g += dxg[j];
        if (a.dXn) g += a.dXn[(r * (size_t)a.N + dst) * a.Kn + j];
        d[j] = g * act_grad_from_out(ld_feat<BF16>(a.ef_out, re * OE + j), a.act);
      }
#pragma unroll
      for (int k = 0; k < KE; ++k) {  // k_bw_dx
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < OE; ++j) acc = fmaf(w[k * OE + j], d[j], acc);
        if (k < DE) { if (a.d_ef && live) st_feat<BF16>(a.d_ef, re * DE + k, acc); }
        else if (a.dXe_c && live) a.dXe_c[re * CW + (k - DE)] = acc;
      }
      if (a.partial) {  // uniform
#pragma unroll
        for (int k = 0; k < KE; ++k) rows[lane * LD + k] = x[k];
#pragma unroll
        for (int j = 0; j < OE; ++j) rows[lane * LD + KE + j] = d[j];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < PS; ++q) {
          if (lane + 64 * q < P) {
            const int kk = pk[q] < KE ? pk[q] : KE - 1;
#pragma unroll 8
            for (int i = 0; i < cnt; ++i) {
              const float xv = pk[q] < KE ? rows[i * LD + kk] : 1.f;
              wacc[q] = fmaf(rows[i * LD + KE + pj[q]], xv, wacc[q]);
            }
          }
        }
        __builtin_amdgcn_wave_barrier();  // the next chunk's rows overwrite these
      }
    }
  }
  if (a.partial) {
#pragma unroll
    for (int q = 0; q < PS; ++q) s_acc[wave][lane + 64 * q] = wacc[q];
    __syncthreads();
    if (threadIdx.x < P) {
      const float v = ((s_acc[0][threadIdx.x] + s_acc[1][threadIdx.x]) + s_acc[2][threadIdx.x]) + s_acc[3][threadIdx.x];
      a.partial[(r * gridDim.x + blockIdx.x) * (size_t)P + threadIdx.x] = v;
    }
  }
}

template <int DE, int DN, int DG, int OE>
__global__ __launch_bounds__(256) void k_bw_edge_wave(BwEdgeWave a) { bw_edge_wave<DE, DN, DG, OE, false>(a); }
template <int DE, int DN, int DG, int OE>
__global__ __launch_bounds__(256) void k_bw_edge_wave_bf16(BwEdgeWave a) { bw_edge_wave<DE, DN, DG, OE, true>(a); }

}  // namespace gnx
