// The two wave-per-tile kernels of the Chain pullback, one text for both element types: k_chain_wave_partials / k_chain_wave_bw
// (gnx_chain_bw_wave.hip, fp32 features) and k_chain_wave_partials_bf16 / k_chain_wave_bw_bf16 (gnx_chain_bw_wave_bf16.hip, bfloat16 features),
// with their launchers.  Each of the two files defines GNX_CHAIN_BW_WAVE_NAME(x) (x itself / x##_bf16: the names of the kernels and launchers) and
// GNX_CHAIN_BW_WAVE_BF16 (false / true) and includes this header once.  The kernels are the text itself and not __device__ functions two kernels
// call (as in gnx_chain_bw_kernel.h): the fp32 instantiations keep the device code they had in a file of their own
// (profiles/chain_bw_wave_resources.json).  The geometry, the LDS plan and the phases (a) - (d) stand at the head of gnx_chain_bw_wave.hip.
//
// The two element types differ in loads and stores alone, all behind overloads and `if constexpr`:
//   read as bf16     ef, nf[src], nf[dst], nf[n], gf[g] (chain_load_seg_bf16: one 16-bit load per element, widened exactly by a shift), and the
//                    upstream gradients g_ef_out / g_nf_out (one 16-bit load per element);
//   written as bf16  d_ef: rounded to nearest even once (to_bf16), one 16-bit store per element from the lane that holds the row — not staged
//                    through LDS: the tape is live until the chunk's parameter-gradient phase has read it.
// A bf16 buffer is 4-byte aligned (the entry checks); rows of odd width and replicas of an odd rows * d start 2-byte aligned, and nothing more is
// assumed: no dword of a feature row is read, none is read, modified and written back, no byte outside a tensor is touched.
// Everything that stays inside the call is fp32 in both: the slice, the tape, the accumulators, dXg, the compact dXn and dXe, the partial rows.
// The arithmetic — chain_layer_fw, chain_wave_bw_rows — is one text without an element type, every sum in its fixed order: the bf16 kernels
// compute, operation for operation, what the fp32 kernels compute on the widened tensors.
// The bf16 pointers are declared float in the records and launchers, as in ChainMlpArgs.
#pragma once
#include "gnx_chain_mlp.h"

#if !defined(GNX_CHAIN_BW_WAVE_NAME) || !defined(GNX_CHAIN_BW_WAVE_BF16)
#error "define GNX_CHAIN_BW_WAVE_NAME and GNX_CHAIN_BW_WAVE_BF16 before including gnx_chain_bw_wave_kernel.h"
#endif

namespace gnx {

// ---- (1) the tiles' partial rows ----
struct ChainWavePartialArgs {
  ChainMlpArgs e, n;  // as ChainWaveArgs (n.d0 = oe; n.a0 unused: ef' lives in the slice)
  const Tile* wtiles;
  int n_wtiles, waves, cap, stride, par_e, par_all, oe, on;
  float* partials;    // [R][n_wtiles][oe + on]
};

// chain_load_seg by the element type of the rows, and one element of an upstream gradient widened
template <int W>
__device__ __forceinline__ void chain_wave_seg(const float* __restrict__ p, int at, int w, float (&cur)[W]) { chain_load_seg<W>(p, at, w, cur); }
template <int W>
__device__ __forceinline__ void chain_wave_seg(const bf16_t* __restrict__ p, int at, int w, float (&cur)[W]) { chain_load_seg_bf16<W>(p, at, w, cur); }
__device__ __forceinline__ float chain_wave_elem(float x) { return x; }
__device__ __forceinline__ float chain_wave_elem(bf16_t x) { return bf16_lo(x); }

template <int W>
__global__ __launch_bounds__(256) void GNX_CHAIN_BW_WAVE_NAME(k_chain_wave_partials)(ChainWavePartialArgs a) {
  constexpr bool BF16 = GNX_CHAIN_BW_WAVE_BF16;
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
  const typename ElemOf<BF16>::T* __restrict__ gfr = feat<BF16>(a.e.a2) + (r * (size_t)a.e.G + t.g) * a.e.d2;
  for (int base = 0; base < ne; base += 64) {
    const int el = base + lane;
    const bool live = el < ne;
    float cur[W];
#pragma unroll
    for (int k = 0; k < W; ++k) cur[k] = 0.f;
    if (live) {
      const int e = t.e0 + el;
      if (a.e.d0 > 0) chain_wave_seg<W>(feat<BF16>(a.e.a0) + (r * (size_t)a.e.E + e) * a.e.d0, 0, a.e.d0, cur);
      if (a.e.d1 > 0) {
        chain_wave_seg<W>(feat<BF16>(a.e.a1) + (r * (size_t)a.e.N + a.e.rowval[e]) * a.e.d1, a.e.d0, a.e.d1, cur);
        chain_wave_seg<W>(feat<BF16>(a.e.a1) + (r * (size_t)a.e.N + a.e.edge_dst[e]) * a.e.d1, a.e.d0 + a.e.d1, a.e.d1, cur);
      }
      if (a.e.d2 > 0) chain_wave_seg<W>(gfr, a.e.d0 + 2 * a.e.d1, a.e.d2, cur);
    }
    int off = 0, kin = a.e.K;
#pragma unroll 1
    for (int l = 0; l < a.e.n_layers; ++l) {
      off = chain_layer_fw<W>(s_mem, off, kin, a.e.layer[l].width, a.e.layer[l].op, cur);
      kin = a.e.layer[l].width;
    }
    if (live) {
      float* __restrict__ so = s_ef + el * stride;
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (k < oe) so[k] = cur[k];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float* __restrict__ prow = a.partials + (r * (size_t)a.n_wtiles + wt) * (size_t)(oe + on);
  {
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
    if (a.n.d1 > 0) chain_wave_seg<W>(feat<BF16>(a.n.a1) + (r * (size_t)a.n.N + node) * a.n.d1, oe, a.n.d1, cur);
    if (a.n.d2 > 0) chain_wave_seg<W>(gfr, oe + a.n.d1, a.n.d2, cur);
  }
  int off = a.par_e, kin = a.n.K;
#pragma unroll 1
  for (int l = 0; l < a.n.n_layers; ++l) {
    off = chain_layer_fw<W>(s_mem, off, kin, a.n.layer[l].width, a.n.layer[l].op, cur);
    kin = a.n.layer[l].width;
  }
  float mine = 0.f;
#pragma unroll
  for (int k = 0; k < W; ++k)
    if (k < on) { const float tot = wave_sum(live ? cur[k] : 0.f); mine = lane == k ? tot : mine; }
  if (lane < on) prow[oe + lane] = mine;
}

// ---- (3) the node and the edge function's pullbacks ----
struct ChainWaveBwArgs {
  ChainMlpArgs e, n;
  ChainBwNarrowShape she, shn;
  const Tile* wtiles;
  int n_wtiles, waves, cap, stride, ld, par_e, par_all, per_wave, oe, on;
  const float *g_ef, *g_nf;  // upstream gradients [R][E][oe] / [R][N][on], or nullptr
  const float* dxg; int kg;  // dXg [R][G][kg]: columns [0, oe) reach the edges, [oe, oe + on) the nodes; or nullptr
  float* d_ef;               // [R][E][de] or nullptr
  float* dxe;                // [R][E][2 dn + dg]: columns [de, Ke) of the edge rows' input gradient, or nullptr
  float* dxn;                // [R][N][dn + dg]: columns [oe, Kn) of the node rows' input gradient, or nullptr
  float *part_e, *part_n;    // the partial rows of the edge / node function (layer l at part + part_off[l] * R * nwg), or nullptr (no gradient wanted)
};

// The way forward onto the tape and back of `cnt` rows the wave holds, one per lane (lanes at or beyond cnt on rows of zeros): k_chain_mlp_bw's
// body.  cur: the input row on entry, the row's input gradient on return.  up(k): the gradient arriving at output column k < ow.
// accs: the function's accumulators, or nullptr.  pbase: where the function's staged parameters start in s_mem.
template <int W, class Up>
__device__ __forceinline__ void chain_wave_bw_rows(const float* s_mem, int pbase, const ChainMlpArgs& f, const ChainBwNarrowShape& sh, float* tape, int ld, float* accs,
                                                   int cnt, int lane, float (&cur)[W], Up up) {
  constexpr int SMAX = chain_bw_smax(W);
  const int nl = f.n_layers, ow = f.layer[nl - 1].width;
  float* const my = tape + lane * ld;
#pragma unroll
  for (int k = 0; k < W; ++k)
    if (k < f.K) my[k] = cur[k];
  {
    int kin = f.K;
#pragma unroll 1
    for (int l = 0; l < nl; ++l) {
      const int width = f.layer[l].width, op = f.layer[l].op;
      if (l == nl - 1 && op == GNX_ACT_GELU) (void)chain_layer_fw<W>(s_mem, pbase + sh.par_off[l], kin, width, GNX_ACT_IDENTITY, cur);  // its pre-activation is all the way back reads
      else (void)chain_layer_fw<W>(s_mem, pbase + sh.par_off[l], kin, width, op, cur);
      if (l < nl - 1) {
#pragma unroll
        for (int k = 0; k < W; ++k)
          if (k < width) my[sh.tape_out[l] + k] = cur[k];
      }
      kin = width;
    }
  }
  // ---- delta of the last layer: (upstream + the shares of the levels above) .* act' ----
  float d[W];
  {
    const int op = f.layer[nl - 1].op, act = op < 5 ? op : GNX_ACT_IDENTITY;
#pragma unroll
    for (int k = 0; k < W; ++k) d[k] = k < ow ? up(k) * act_grad_bw(cur[k], act) : 0.f;
  }
  // ---- back through the layers ----
#pragma unroll 1
  for (int l = nl - 1; l >= 0; --l) {
    const int width = f.layer[l].width, op = f.layer[l].op;
    const int kin = l > 0 ? f.layer[l - 1].width : f.K, xs = l > 0 ? sh.tape_out[l - 1] : 0;
    const float* __restrict__ sp = s_mem + pbase + sh.par_off[l];
    float gin[W];
#pragma unroll
    for (int k = 0; k < W; ++k) gin[k] = 0.f;
    if (op < 5) {
      if (accs) {
#pragma unroll
        for (int k = 0; k < W; ++k)
          if (k < width) my[sh.dslot + k] = d[k];
        __builtin_amdgcn_wave_barrier();
        chain_bw_dw_phase<SMAX>(tape, ld, cnt, xs, sh.dslot, width, kin, accs + sh.part_off[l], lane);
        __builtin_amdgcn_wave_barrier();  // (the next layer's deltas overwrite these)
      }
      const int OP = ceil4(width);
#pragma unroll
      for (int k = 0; k < W; ++k) {
        if (k < kin) {
          float acc = 0.f;
#pragma unroll
          for (int j0 = 0; j0 < W; j0 += 4) {
            if (j0 < width) {
              const float4 wv = *reinterpret_cast<const float4*>(sp + k * OP + j0);  // (the padding of W and of d is 0)
              acc = fmaf(wv.x, d[j0], acc); acc = fmaf(wv.y, d[j0 + 1], acc); acc = fmaf(wv.z, d[j0 + 2], acc); acc = fmaf(wv.w, d[j0 + 3], acc);
            }
          }
          gin[k] = acc;
        }
      }
    } else {
      // k_ln_backward with one norm: x from the tape, the statistics again, dx = (dxh - mean(dxh)) / sden - c * coef, dxh = dy .* gamma
      float c[W];
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < W; ++k) { c[k] = k < width ? my[xs + k] : 0.f; s += c[k]; }
      const float mu = s / (float)width;
      float v = 0.f;
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (k < width) { c[k] -= mu; v = fmaf(c[k], c[k], v); }
      v /= (float)width;
      const float sigma = sqrtf(v);
      const float sden = op == 5 ? sigma + kChainLnEps : sqrtf(v + kChainLnEps);
      const float q = op == 5 ? sigma * sden * sden : sden * sden * sden;
      float sum_dxh = 0.f, sum_dxh_c = 0.f;
#pragma unroll
      for (int k0 = 0; k0 < W; k0 += 4) {
        if (k0 < width) {
          const float4 g4 = *reinterpret_cast<const float4*>(sp + k0);
          const float gg[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float dxh = d[k0 + u] * gg[u];  // (0 in the padding)
            gin[k0 + u] = dxh;
            sum_dxh += dxh;
            sum_dxh_c = fmaf(dxh, c[k0 + u], sum_dxh_c);
          }
        }
      }
      if (accs) {  // [dy ; dy .* xhat] behind the tape: lane j < width sums dgamma[j], lane width + j sums dbeta[j]
#pragma unroll
        for (int k = 0; k < W; ++k)
          if (k < width) { my[sh.dslot + k] = d[k]; my[sh.dslot + width + k] = d[k] * (c[k] / sden); }
        __builtin_amdgcn_wave_barrier();
        if (lane < 2 * width) {
          float* const ap = accs + sh.part_off[l] + lane;
          const int slot = sh.dslot + (lane < width ? width + lane : lane - width);
          float acc = *ap;
          for (int i = 0; i < cnt; ++i) acc += tape[i * ld + slot];
          *ap = acc;
        }
        __builtin_amdgcn_wave_barrier();
      }
      const float mean_dxh = sum_dxh / (float)width;
      const float coef = q > 0.f ? sum_dxh_c / ((float)width * q) : 0.f;
#pragma unroll
      for (int k = 0; k < W; ++k) gin[k] = k < width ? (gin[k] - mean_dxh) / sden - c[k] * coef : 0.f;
    }
    if (l > 0) {  // delta of layer l - 1 from the gradient w.r.t. its output
      const int pop = f.layer[l - 1].op;
      if (pop >= 5 || pop == GNX_ACT_IDENTITY) {
#pragma unroll
        for (int k = 0; k < W; ++k) d[k] = gin[k];
      } else {
        float y[W];
        if (pop == GNX_ACT_GELU) {  // its pre-activation, from its input on the tape
          const int kin1 = l > 1 ? f.layer[l - 2].width : f.K, xs1 = l > 1 ? sh.tape_out[l - 2] : 0;
#pragma unroll
          for (int k = 0; k < W; ++k) y[k] = k < kin1 ? my[xs1 + k] : 0.f;
          (void)chain_layer_fw<W>(s_mem, pbase + sh.par_off[l - 1], kin1, kin, GNX_ACT_IDENTITY, y);
        } else {
#pragma unroll
          for (int k = 0; k < W; ++k) y[k] = k < kin ? my[xs + k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < W; ++k) d[k] = k < kin ? gin[k] * act_grad_bw(y[k], pop) : 0.f;
      }
    } else {
#pragma unroll
      for (int k = 0; k < W; ++k) cur[k] = gin[k];
    }
  }
}

__device__ __forceinline__ void chain_wave_lds_turn() {  // the wave's LDS rows change hands between lanes: LDS operations of one wave execute in order
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int W>
__global__ __launch_bounds__(256) void GNX_CHAIN_BW_WAVE_NAME(k_chain_wave_bw)(ChainWaveBwArgs a) {
  constexpr bool BF16 = GNX_CHAIN_BW_WAVE_BF16;
  typedef typename ElemOf<BF16>::T elem_t;
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const int NT = blockDim.x, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ld = a.ld, Pe = a.she.P, Pn = a.shn.P, oe = a.oe, on = a.on, stride = a.stride;
  float* const tape = s_mem + a.par_all + wave * a.per_wave;  // this wave's rows, its accumulators (edge, node), its slice
  float* const acc_e = tape + 64 * ld;
  float* const acc_n = acc_e + Pe;
  float* const slice = acc_n + Pn;
  chain_stage_params(a.e, s_mem, NT);
  chain_stage_params(a.n, s_mem + a.par_e, NT);
  for (int p = lane; p < Pe + Pn; p += 64) acc_e[p] = 0.f;
  __syncthreads();
  const size_t r = blockIdx.y;
  const int wt = blockIdx.x * a.waves + wave;
  if (wt < a.n_wtiles) {  // wave-uniform
    const Tile t = a.wtiles[wt];
    const int ne = t.e1 - t.e0, nn = t.n1 - t.n0;
    const elem_t* __restrict__ gfr = feat<BF16>(a.e.a2) + (r * (size_t)a.e.G + t.g) * a.e.d2;
    const float* __restrict__ xg = a.dxg ? a.dxg + (r * (size_t)a.e.G + t.g) * (size_t)a.kg : nullptr;
    // the edge function's input row of edge e0 + el, zeros beyond the tile
    auto edge_row = [&](int el, float (&cur)[W]) __attribute__((always_inline)) {
#pragma unroll
      for (int k = 0; k < W; ++k) cur[k] = 0.f;
      if (el < ne) {
        const int e = t.e0 + el;
        if (a.e.d0 > 0) chain_wave_seg<W>(feat<BF16>(a.e.a0) + (r * (size_t)a.e.E + e) * a.e.d0, 0, a.e.d0, cur);
        if (a.e.d1 > 0) {
          chain_wave_seg<W>(feat<BF16>(a.e.a1) + (r * (size_t)a.e.N + a.e.rowval[e]) * a.e.d1, a.e.d0, a.e.d1, cur);
          chain_wave_seg<W>(feat<BF16>(a.e.a1) + (r * (size_t)a.e.N + a.e.edge_dst[e]) * a.e.d1, a.e.d0 + a.e.d1, a.e.d1, cur);
        }
        if (a.e.d2 > 0) chain_wave_seg<W>(gfr, a.e.d0 + 2 * a.e.d1, a.e.d2, cur);
      }
    };

    // ---- (a) lanes as edges: ef' into the slice ----
    for (int base = 0; base < ne; base += 64) {  // (wave-uniform trips)
      const int el = base + lane;
      float cur[W];
      edge_row(el, cur);
      int off = 0, kin = a.e.K;
#pragma unroll 1
      for (int l = 0; l < a.e.n_layers; ++l) {
        off = chain_layer_fw<W>(s_mem, off, kin, a.e.layer[l].width, a.e.layer[l].op, cur);
        kin = a.e.layer[l].width;
      }
      if (el < ne) {
        float* __restrict__ so = slice + el * stride;
#pragma unroll
        for (int k = 0; k < W; ++k)
          if (k < oe) so[k] = cur[k];
      }
    }
    chain_wave_lds_turn();

    // ---- (b) lanes as nodes ----
    {
      const bool live = lane < nn;
      const int node = t.n0 + lane;
      float cur[W];
#pragma unroll
      for (int k = 0; k < W; ++k) cur[k] = 0.f;
      if (live) {
        const int c1 = a.n.colptr[node + 1] - t.e0;
        for (int i = a.n.colptr[node] - t.e0; i < c1; ++i) {
          const float* __restrict__ so = slice + i * stride;
#pragma unroll
          for (int k = 0; k < W; ++k)
            if (k < oe) cur[k] += so[k];
        }
        if (a.n.d1 > 0) chain_wave_seg<W>(feat<BF16>(a.n.a1) + (r * (size_t)a.n.N + node) * a.n.d1, oe, a.n.d1, cur);
        if (a.n.d2 > 0) chain_wave_seg<W>(gfr, oe + a.n.d1, a.n.d2, cur);
      }
      const elem_t* __restrict__ gp = a.g_nf && live ? feat<BF16>(a.g_nf) + (r * (size_t)a.n.N + node) * (size_t)on : nullptr;
      const float* __restrict__ e1 = xg && live ? xg + oe : nullptr;
      chain_wave_bw_rows<W>(s_mem, a.par_e, a.n, a.shn, tape, ld, a.part_n ? acc_n : nullptr, nn, lane, cur, [&](int k) __attribute__((always_inline)) {
        float g = gp ? chain_wave_elem(gp[k]) : 0.f;
        if (e1) g += e1[k];
        return g;
      });
      if (live && a.dxn) {
        float* __restrict__ o = a.dxn + (r * (size_t)a.n.N + node) * (size_t)(a.n.K - oe);
#pragma unroll
        for (int k = 0; k < W; ++k)
          if (k >= oe && k < a.n.K) o[k - oe] = cur[k];
      }
      chain_wave_lds_turn();  // (every lane has summed its in-edges' rows long since: the slice changes its meaning here)
      if (live) {
        float* __restrict__ so = slice + lane * stride;
#pragma unroll
        for (int k = 0; k < W; ++k)
          if (k < oe) so[k] = cur[k];
      }
    }
    chain_wave_lds_turn();

    // ---- (c) lanes as edges again ----
    for (int base = 0; base < ne; base += 64) {
      const int el = base + lane;
      const bool live = el < ne;
      const int e = t.e0 + el;
      float cur[W];
      edge_row(el, cur);
      const elem_t* __restrict__ gp = a.g_ef && live ? feat<BF16>(a.g_ef) + (r * (size_t)a.e.E + e) * (size_t)oe : nullptr;
      const float* __restrict__ e1 = live ? xg : nullptr;
      const float* __restrict__ e2 = live ? slice + (a.e.edge_dst[e] - t.n0) * stride : nullptr;
      chain_wave_bw_rows<W>(s_mem, 0, a.e, a.she, tape, ld, a.part_e ? acc_e : nullptr, min(64, ne - base), lane, cur, [&](int k) __attribute__((always_inline)) {
        float g = gp ? chain_wave_elem(gp[k]) : 0.f;
        if (e1) g += e1[k];
        if (e2) g += e2[k];
        return g;
      });
      if (live) {
        const size_t at = r * (size_t)a.e.E + e;
        if (a.d_ef) {
          if constexpr (BF16) {  // rounded once, one 16-bit store per element from the lane that holds the row
            bf16_t* __restrict__ o = reinterpret_cast<bf16_t*>(a.d_ef) + at * (size_t)a.e.d0;
#pragma unroll
            for (int k = 0; k < W; ++k)
              if (k < a.e.d0) o[k] = to_bf16(cur[k]);
          } else {
            float* __restrict__ o = a.d_ef + at * (size_t)a.e.d0;
#pragma unroll
            for (int k = 0; k < W; ++k)
              if (k < a.e.d0) o[k] = cur[k];
          }
        }
        if (a.dxe) {
          float* __restrict__ o = a.dxe + at * (size_t)(a.e.K - a.e.d0);
#pragma unroll
          for (int k = 0; k < W; ++k)
            if (k >= a.e.d0 && k < a.e.K) o[k - a.e.d0] = cur[k];
        }
      }
      __builtin_amdgcn_wave_barrier();  // (the next chunk's rows overwrite the tape)
    }
  }
  if (!a.part_e && !a.part_n) return;  // uniform
  // ---- (d) one partial row per workgroup and layer, the waves added in wave order ----
  __syncthreads();
  const size_t wg = r * gridDim.x + blockIdx.x, nwg = (size_t)gridDim.x * gridDim.y;
  const float* const acc0 = s_mem + a.par_all + 64 * ld;
  for (int fn = 0; fn < 2; ++fn) {
    const ChainMlpArgs& f = fn ? a.n : a.e;
    const ChainBwNarrowShape& sh = fn ? a.shn : a.she;
    float* const part = fn ? a.part_n : a.part_e;
    if (!part) continue;
    const float* const accf = acc0 + (fn ? Pe : 0);
    int kin = f.K;
    for (int l = 0; l < f.n_layers; ++l) {
      const int width = f.layer[l].width;
      const int Pl = f.layer[l].op < 5 ? width * (kin + 1) : 2 * width, at = sh.part_off[l];
      float* __restrict__ out = part + (size_t)at * nwg + wg * (size_t)Pl;
      for (int p = threadIdx.x; p < Pl; p += NT) {
        float v = accf[at + p];
        for (int ww = 1; ww < a.waves; ++ww) v += accf[ww * a.per_wave + at + p];
        out[p] = v;
      }
      kin = width;
    }
  }
}

// ---- the launchers.  The caller (chain_backward_wave, gnx_backward.hip) asked chain_bw_wave_takes and opens the ProfScopes ----
inline int32_t chain_wave_fn_args(const gnx_graphs* h, const gnx_chain_block_params& p, const ChainShape& sh, const float* ef, const float* nf, const float* gf,
                                  ChainRule rule, const char* who, hipStream_t s, ChainMlpArgs& e, ChainMlpArgs& n, int* w) {
  int we, wn;
  size_t rows;
  if (int32_t rc = chain_mlp_prologue(h, 0, p.edgefn, ef, p.de, nf, p.dn, gf, p.dg, rule, who, s, e, &we, &rows)) return rc;
  if (int32_t rc = chain_mlp_prologue(h, 1, p.nodefn, nullptr, sh.ow[0], nf, p.dn, gf, p.dg, rule, who, s, n, &wn, &rows)) return rc;
  *w = std::max(we, wn);
  return GNX_OK;
}

int32_t GNX_CHAIN_BW_WAVE_NAME(launch_chain_wave_partials)(const gnx_graphs* h, const gnx_chain_block_params& p, const ChainShape& sh, const float* ef, const float* nf,
                                                           const float* gf, float* partials, int64_t R, hipStream_t s) {
  ChainWavePartialArgs a{};
  int w;
  if (int32_t rc = chain_wave_fn_args(h, p, sh, ef, nf, gf, CHAIN_RULE_FW, "launch_chain_wave_partials", s, a.e, a.n, &w)) return rc;
  a.waves = chain_wave_waves(sh, h->wtile_e_cap);
  if (a.waves < 2 || h->max_in_degree > h->wtile_e_cap) return fail(GNX_ERR_INVALID_ARG, "launch_chain_wave_partials: the block is outside the wave rule");
  a.wtiles = h->d_wtiles; a.n_wtiles = (int)h->n_wtiles();
  a.cap = h->wtile_e_cap; a.stride = chain_wave_stride(sh.ow[0]);
  a.par_e = (int)chain_narrow_lds_floats(p.edgefn, sh.k0[0]);
  a.par_all = a.par_e + (int)chain_narrow_lds_floats(p.nodefn, sh.k0[1]);
  a.oe = sh.ow[0]; a.on = sh.ow[1]; a.partials = partials;
  const dim3 grid((unsigned)((a.n_wtiles + a.waves - 1) / a.waves), (unsigned)R);
  const size_t lds = sizeof(float) * ((size_t)a.par_all + (size_t)a.waves * a.cap * a.stride);
  if (w <= 8) GNX_LAUNCH((GNX_CHAIN_BW_WAVE_NAME(k_chain_wave_partials)<8>), grid, dim3(64 * a.waves), lds, s, a);
  else if (w <= 16) GNX_LAUNCH((GNX_CHAIN_BW_WAVE_NAME(k_chain_wave_partials)<16>), grid, dim3(64 * a.waves), lds, s, a);
  else GNX_LAUNCH((GNX_CHAIN_BW_WAVE_NAME(k_chain_wave_partials)<32>), grid, dim3(64 * a.waves), lds, s, a);
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

int32_t GNX_CHAIN_BW_WAVE_NAME(launch_chain_wave_bw)(const gnx_graphs* h, const gnx_chain_block_params& p, const ChainShape& sh, const float* ef, const float* nf,
                                                     const float* gf, const ChainWaveBwIo& io, int64_t R, hipStream_t s) {
  ChainWaveBwArgs a{};
  int w;
  if (int32_t rc = chain_wave_fn_args(h, p, sh, ef, nf, gf, CHAIN_RULE_BW, "launch_chain_wave_bw", s, a.e, a.n, &w)) return rc;
  const ChainBwWaveShape ws = chain_bw_wave_shape(sh, h->wtile_e_cap, h->n_wtiles());
  if (ws.waves < 2 || h->max_in_degree > h->wtile_e_cap) return fail(GNX_ERR_INVALID_ARG, "launch_chain_wave_bw: the block is outside the wave rule");
  a.she = ws.e; a.shn = ws.n;
  a.wtiles = h->d_wtiles; a.n_wtiles = (int)h->n_wtiles();
  a.waves = ws.waves; a.cap = h->wtile_e_cap; a.stride = ws.stride; a.ld = ws.ld;
  a.par_e = ws.par_e; a.par_all = ws.par_all; a.per_wave = ws.per_wave;
  a.oe = sh.ow[0]; a.on = sh.ow[1];
  a.g_ef = io.g_ef; a.g_nf = io.g_nf; a.dxg = io.dxg; a.kg = io.kg;
  a.d_ef = io.d_ef; a.dxe = io.dxe; a.dxn = io.dxn; a.part_e = io.part_e; a.part_n = io.part_n;
  const dim3 grid((unsigned)ws.nwg, (unsigned)R), block(64 * ws.waves);
  const size_t lds = sizeof(float) * ((size_t)ws.par_all + (size_t)ws.waves * ws.per_wave);
  if (w <= 8) GNX_LAUNCH((GNX_CHAIN_BW_WAVE_NAME(k_chain_wave_bw)<8>), grid, block, lds, s, a);
  else if (w <= 16) GNX_LAUNCH((GNX_CHAIN_BW_WAVE_NAME(k_chain_wave_bw)<16>), grid, block, lds, s, a);
  else GNX_LAUNCH((GNX_CHAIN_BW_WAVE_NAME(k_chain_wave_bw)<32>), grid, block, lds, s, a);
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
