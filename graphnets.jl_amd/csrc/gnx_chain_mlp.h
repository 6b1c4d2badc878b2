// What the fused Chain update-function kernels share: k_chain_mlp (gnx_chain_narrow.hip, the forward) and k_chain_mlp_bw
// (gnx_chain_bw_narrow.hip, the pullback) stage a function's parameters in LDS and build a lane's input row with this code.  chain_layer_fw is
// the forward kernel's layer, operation for operation, as a function: the pullback's forward half runs it (and so carries the forward's bits);
// k_chain_mlp keeps its loop in place, because as a function call the same text costs its 32-wide instantiation 16 more registers.
#pragma once
#include <algorithm>
#include <type_traits>

#include "gnx_launchers.h"
#include "gnx_wave_kernel.h"  // act_row

namespace gnx {

enum : int { SRC_EDGE = 0, SRC_NODE = 1, SRC_ROWS = 2 };

struct ChainMlpLayer {
  const float* w;  // Dense: weight (out x in, column-major) / LayerNorm: gamma
  const float* b;  // Dense: bias or nullptr / LayerNorm: beta
  int width;       // output width
  int op;          // 0..4: Dense with activation GNX_ACT_*; 5 / 6: LayerNorm with 1 / (sigma + eps) / 1 / sqrt(sigma^2 + eps);
                   // 7: a Dropout entry of a training call (w = b = nullptr; the training kernels alone see it: gnx_chain_drop.h)
};

struct ChainMlpArgs {
  ChainMlpLayer layer[kChainMaxLayers];
  int n_layers, K;       // K: width of the function's input row
  const float *a0, *a1, *a2;  // EDGE: ef, nf, gf / NODE: ef', nf, gf / ROWS: the input rows, -, -
  int d0, d1, d2;        // their widths (EDGE: de, dn, dg; NODE: oe, dn, dg)
  int N, E, G;
  const int *colptr, *rowval, *edge_dst, *seg_off;  // seg_off: edge_off (EDGE) / node_off (NODE), [G + 1]
  float* out; int ow;    // [R][rows][ow]
  size_t rows;           // rows of the entity per replica
};

// cur[at .. at + w) = p[0 .. w): one dword load per element behind a uniform test
template <int WMAX>
__device__ __forceinline__ void chain_load_seg(const float* __restrict__ p, int at, int w, float (&cur)[WMAX]) {
#pragma unroll
  for (int k = 0; k < WMAX; ++k)
    if (k >= at && k < at + w) cur[k] = p[k - at];
}

// the function's parameters into s_par, zero-padded to groups of four: a Dense as [ceil4(k_in)][ceil4(width)] weights (element (j, k) at
// k * ceil4(width) + j) + ceil4(width) biases, a LayerNorm as gamma and beta.  All NT threads of the workgroup call it; the caller synchronises.
// TRAIN (the training kernels): a Dropout entry (op 7) stages nothing.
template <bool TRAIN = false>
__device__ __forceinline__ void chain_stage_params(const ChainMlpArgs& a, float* s_par, int NT) {
  int off = 0, kin = a.K;
  for (int l = 0; l < a.n_layers; ++l) {
    const ChainMlpLayer L = a.layer[l];
    if constexpr (TRAIN) { if (L.op == 7) continue; }  // (its width is kin)
    const int OP = ceil4(L.width);
    if (L.op < 5) {
      const int n = ceil4(kin) * OP;
      for (int i = threadIdx.x; i < n; i += NT) {
        const int k = i / OP, j = i - k * OP;
        s_par[off + i] = (k < kin && j < L.width) ? L.w[(size_t)k * L.width + j] : 0.f;
      }
      for (int j = threadIdx.x; j < OP; j += NT) s_par[off + n + j] = (j < L.width && L.b) ? L.b[j] : 0.f;
      off += n + OP;
    } else {
      for (int j = threadIdx.x; j < OP; j += NT) {
        s_par[off + j] = j < L.width ? L.w[j] : 0.f;
        s_par[off + OP + j] = j < L.width ? L.b[j] : 0.f;
      }
      off += 2 * OP;
    }
    kin = L.width;
  }
}
// (floats a layer takes in that layout: chain_layer_par_floats, gnx_chain_plan.h — ceil4 is defined there)

// the input row of `row` (replica r) of the function, entries at or beyond K exactly 0.f
template <int WMAX, int SRC>
__device__ __forceinline__ void chain_input_row(const ChainMlpArgs& a, size_t row, size_t r, float (&cur)[WMAX]) {
#pragma unroll
  for (int k = 0; k < WMAX; ++k) cur[k] = 0.f;
  if constexpr (SRC == SRC_EDGE) {
    const int e = (int)row;
    if (a.d0 > 0) chain_load_seg<WMAX>(a.a0 + (r * (size_t)a.E + e) * a.d0, 0, a.d0, cur);
    if (a.d1 > 0) {
      chain_load_seg<WMAX>(a.a1 + (r * (size_t)a.N + a.rowval[e]) * a.d1, a.d0, a.d1, cur);
      chain_load_seg<WMAX>(a.a1 + (r * (size_t)a.N + a.edge_dst[e]) * a.d1, a.d0 + a.d1, a.d1, cur);
    }
    if (a.d2 > 0) chain_load_seg<WMAX>(a.a2 + (r * (size_t)a.G + segment_of(a.seg_off, a.G, e)) * a.d2, a.d0 + 2 * a.d1, a.d2, cur);
  } else if constexpr (SRC == SRC_NODE) {
    const int n = (int)row;
    if (a.d0 > 0) {
      const int e1 = a.colptr[n + 1];
      for (int e = a.colptr[n]; e < e1; ++e) {
        const float* __restrict__ p = a.a0 + (r * (size_t)a.E + e) * a.d0;
#pragma unroll
        for (int k = 0; k < WMAX; ++k)
          if (k < a.d0) cur[k] += p[k];
      }
    }
    if (a.d1 > 0) chain_load_seg<WMAX>(a.a1 + (r * (size_t)a.N + n) * a.d1, a.d0, a.d1, cur);
    if (a.d2 > 0) chain_load_seg<WMAX>(a.a2 + (r * (size_t)a.G + segment_of(a.seg_off, a.G, n)) * a.d2, a.d0 + a.d1, a.d2, cur);
  } else {
    chain_load_seg<WMAX>(a.a0 + (r * a.rows + row) * (size_t)a.K, 0, a.K, cur);
  }
}

// ---- the same on bfloat16 feature rows (k_chain_mlp_bf16, k_chain_mlp_bw_bf16): which sources are bf16 stands at the head of their files ----
// cur[at .. at + w) = widened p[0 .. w): one 16-bit load per element behind a uniform test
template <int WMAX>
__device__ __forceinline__ void chain_load_seg_bf16(const bf16_t* __restrict__ p, int at, int w, float (&cur)[WMAX]) {
#pragma unroll
  for (int k = 0; k < WMAX; ++k)
    if (k >= at && k < at + w) cur[k] = bf16_lo(p[k - at]);
}

// chain_input_row on bf16 features; entries at or beyond K exactly 0.f
template <int WMAX, int SRC>
__device__ __forceinline__ void chain_input_row_bf16(const ChainMlpArgs& a, size_t row, size_t r, float (&cur)[WMAX]) {
  if constexpr (SRC == SRC_ROWS) {
    chain_input_row<WMAX, SRC_ROWS>(a, row, r, cur);
    return;
  }
#pragma unroll
  for (int k = 0; k < WMAX; ++k) cur[k] = 0.f;
  const bf16_t* __restrict__ b0 = reinterpret_cast<const bf16_t*>(a.a0);
  const bf16_t* __restrict__ b1 = reinterpret_cast<const bf16_t*>(a.a1);
  const bf16_t* __restrict__ b2 = reinterpret_cast<const bf16_t*>(a.a2);
  if constexpr (SRC == SRC_EDGE) {
    const int e = (int)row;
    if (a.d0 > 0) chain_load_seg_bf16<WMAX>(b0 + (r * (size_t)a.E + e) * a.d0, 0, a.d0, cur);
    if (a.d1 > 0) {
      chain_load_seg_bf16<WMAX>(b1 + (r * (size_t)a.N + a.rowval[e]) * a.d1, a.d0, a.d1, cur);
      chain_load_seg_bf16<WMAX>(b1 + (r * (size_t)a.N + a.edge_dst[e]) * a.d1, a.d0 + a.d1, a.d1, cur);
    }
    if (a.d2 > 0) chain_load_seg_bf16<WMAX>(b2 + (r * (size_t)a.G + segment_of(a.seg_off, a.G, e)) * a.d2, a.d0 + 2 * a.d1, a.d2, cur);
  } else {
    const int n = (int)row;
    if (a.d0 > 0) {  // the fp32 ef' of this call: chain_input_row's sequential adds in CSC order
      const int e1 = a.colptr[n + 1];
      for (int e = a.colptr[n]; e < e1; ++e) {
        const float* __restrict__ p = a.a0 + (r * (size_t)a.E + e) * a.d0;
#pragma unroll
        for (int k = 0; k < WMAX; ++k)
          if (k < a.d0) cur[k] += p[k];
      }
    }
    if (a.d1 > 0) chain_load_seg_bf16<WMAX>(b1 + (r * (size_t)a.N + n) * a.d1, a.d0, a.d1, cur);
    if (a.d2 > 0) chain_load_seg_bf16<WMAX>(b2 + (r * (size_t)a.G + segment_of(a.seg_off, a.G, n)) * a.d2, a.d0 + a.d1, a.d2, cur);
  }
}

// cur <- layer(cur): a Dense (op 0..4, its activation) or a LayerNorm (op 5 / 6) of k_in inputs and `width` outputs whose staged parameters
// start at s_par + off; returns the next layer's offset.  Products run as groups of 4 outputs x 4 inputs behind wave-uniform tests; entries at or beyond `width` end exactly 0.f.
template <int WMAX>
__device__ __forceinline__ int chain_layer_fw(const float* s_par, int off, int kin, int width, int op, float (&cur)[WMAX]) {
  const int OP = ceil4(width);
  if (op < 5) {
    float nxt[WMAX];
    const float* __restrict__ sw = s_par + off;
    const float* __restrict__ sb = sw + ceil4(kin) * OP;
#pragma unroll
    for (int j0 = 0; j0 < WMAX; j0 += 4) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      if (j0 < width) {
        const float4 bb = *reinterpret_cast<const float4*>(sb + j0);
        acc[0] = bb.x; acc[1] = bb.y; acc[2] = bb.z; acc[3] = bb.w;
#pragma unroll
        for (int k0 = 0; k0 < WMAX; k0 += 4) {
          if (k0 < kin) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
              const float4 w = *reinterpret_cast<const float4*>(sw + (k0 + kk) * OP + j0);
              acc[0] = fmaf(w.x, cur[k0 + kk], acc[0]); acc[1] = fmaf(w.y, cur[k0 + kk], acc[1]);
              acc[2] = fmaf(w.z, cur[k0 + kk], acc[2]); acc[3] = fmaf(w.w, cur[k0 + kk], acc[3]);
            }
          }
        }
        act_row<4>(acc, op);
      }
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) nxt[j0 + jj] = j0 + jj < width ? acc[jj] : 0.f;  // (sigmoid(0) != 0: the padding stays exactly 0)
    }
#pragma unroll
    for (int k = 0; k < WMAX; ++k) cur[k] = nxt[k];
    return off + ceil4(kin) * OP + OP;
  } else {
    // k_chain_layernorm's formula (gnx_chain.cpp), the sums taken by the lane in element order
    const float* __restrict__ sg = s_par + off;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < WMAX; ++k) s += cur[k];  // (the padding is 0)
    const float mu = s / (float)width;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < WMAX; ++k)
      if (k < width) { const float c = cur[k] - mu; v = fmaf(c, c, v); }
    v /= (float)width;
    const float inv = op == 5 ? 1.f / (sqrtf(v) + kChainLnEps) : 1.f / sqrtf(v + kChainLnEps);
#pragma unroll
    for (int k0 = 0; k0 < WMAX; k0 += 4) {
      if (k0 < width) {
        const float4 g = *reinterpret_cast<const float4*>(sg + k0);
        const float4 b = *reinterpret_cast<const float4*>(sg + OP + k0);
        const float gg[4] = {g.x, g.y, g.z, g.w}, bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) cur[k0 + kk] = k0 + kk < width ? fmaf(gg[kk], (cur[k0 + kk] - mu) * inv, bb[kk]) : 0.f;
      }
    }
    return off + 2 * OP;
  }
}

// d/dz of NNlib.gelu's tanh form 0.5 z (1 + tanh(c (z + 0.044715 z^3))): unlike relu / tanh / sigmoid it is not a function of the
// OUTPUT (gelu is not monotonic), so a gelu level differentiates from its pre-activation z = W x + b: act code 4 of act_grad_bw means "v holds z".
__device__ __forceinline__ float gelu_grad_pre(float z) {
  const float c = 0.7978845608028654f, k = 0.044715f;
  const float t = tanhf(c * (z + k * z * z * z));
  return 0.5f * (1.f + t) + 0.5f * z * (1.f - t * t) * c * (1.f + 3.f * k * z * z);
}
__device__ __forceinline__ float act_grad_bw(float v, int act) { return act == 4 ? gelu_grad_pre(v) : act_grad_from_out(v, act); }

// What the three fused launchers (launch_chain_narrow, _bf16, launch_chain_bw_narrow: `who`) do first: ask the rule, refuse a Dense without weights
// (the forward's launchers pass a layer of width 0, the pullback's does not: each keeps the set it took), fill the argument record's function
// part from the chain.  *wmax: the register width's lower bound (the largest of K and the layer widths); *rows: rows of the entity per replica.
inline int32_t chain_mlp_prologue(const gnx_graphs* h, int entity, const gnx_chain& c, const float* in0, int d0, const float* in1, int d1, const float* in2, int d2,
                                  ChainRule rule, const char* who, hipStream_t s, ChainMlpArgs& a, int* wmax, size_t* rows) {
  const int K = entity == 0 ? d0 + 2 * d1 + d2 : d0 + d1 + d2;
  *rows = entity == 0 ? (size_t)h->E : (entity == 1 ? (size_t)h->N : (size_t)h->G);
  if (!chain_rule_takes(rule, c, K, *rows)) return fail(GNX_ERR_INVALID_ARG, std::string(who) + ": the function is outside the fused rule");
  // the destination of every edge: a forward launch makes sure of the table itself, the pullback (chain_bw_run) has
  if (rule == CHAIN_RULE_FW && entity == 0) { if (int32_t rcw = gnx_ensure_wide_tables(h, s)) return rcw; }
  *wmax = K;
  int kin = K;
  for (int i = 0; i < c.n_layers; ++i) {
    const gnx_dense& l = c.layers[i];
    const bool drop = chain_layer_is_dropout(l);  // (a training launcher's chain: no parameters, op 7)
    if (!chain_layer_is_ln(l) && !drop && (rule == CHAIN_RULE_BW || c.widths[i] > 0) && kin > 0 && !l.weight) return fail(GNX_ERR_INVALID_ARG, "Chain: Dense weight is NULL");
    a.layer[i] = drop ? ChainMlpLayer{nullptr, nullptr, c.widths[i], 7} : ChainMlpLayer{l.weight, l.bias, c.widths[i], chain_layer_is_ln(l) ? 5 + chain_layer_ln_mode(l) : l.act};
    *wmax = std::max(*wmax, (int)c.widths[i]);
    kin = c.widths[i];
  }
  a.n_layers = c.n_layers; a.K = K;
  a.a0 = in0; a.a1 = in1; a.a2 = in2; a.d0 = d0; a.d1 = d1; a.d2 = d2;
  a.N = (int)h->N; a.E = (int)h->E; a.G = (int)h->G;
  a.colptr = h->d_colptr; a.rowval = h->d_rowval; a.edge_dst = h->d_edge_dst; a.seg_off = entity == 0 ? h->d_edge_off : h->d_node_off;
  a.rows = *rows;
  return GNX_OK;
}

// the WMAX x SRC switch of the three launchers: launch(WMAX, SRC) as integral constants, WMAX in {8, 16, 32} the smallest that covers wmax
template <int V> using ChainInt = std::integral_constant<int, V>;
template <class Launch>
inline void chain_mlp_dispatch(int wmax, int entity, Launch&& launch) {
  auto width = [&](auto src) { wmax <= 8 ? launch(ChainInt<8>{}, src) : wmax <= 16 ? launch(ChainInt<16>{}, src) : launch(ChainInt<32>{}, src); };
  entity == 0 ? width(ChainInt<SRC_EDGE>{}) : entity == 1 ? width(ChainInt<SRC_NODE>{}) : width(ChainInt<SRC_ROWS>{});
}

}  // namespace gnx
