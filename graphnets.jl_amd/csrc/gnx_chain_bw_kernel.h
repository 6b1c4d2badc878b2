// The fused Chain pullback kernel, one text for both element types: k_chain_mlp_bw (gnx_chain_bw_narrow.hip, fp32 features) and
// k_chain_mlp_bw_bf16 (gnx_chain_bw_narrow_bf16.hip, bfloat16 features).  Each of the two files defines GNX_CHAIN_BW_KERNEL (the kernel's name) and
// GNX_CHAIN_BW_BF16 (false / true) and includes this header once.  The text is the kernel itself and not a __device__ function both kernels
// call: behind a forced-inline call the fp32 kernel's registers moved (32-wide: 235 -> 251 VGPRs); as it stands its device code is the code it
// had in a file of its own, instruction for instruction (profiles/chain_bw_narrow_resources.json).  The two differ in three places, all
// loads and stores behind `if constexpr`: how the input row is gathered (chain_input_row / chain_input_row_bf16), how the upstream gradient is read
// (one dword / one 16-bit load per element, widened exactly) and how `direct` (d_ef) is stored (one dword / one 16-bit store per element, rounded
// to nearest even once).  Everything between — the tape, the deltas, the accumulators, the partial rows — is the same text, so the bf16 kernel
// computes, operation for operation, what the fp32 kernel computes on the widened tensors.
//
// BF16, what holds bfloat16 elements (declared float in the records, like the feature pointers of BlockArgs):
//   SRC_EDGE  f.a0, f.a1, f.a2 (ef, nf, gf), G, direct        SRC_NODE  f.a1, f.a2 (nf, gf), G; f.a0 is the fp32 ef' of this call
//   SRC_ROWS  G; f.a0 is the fp32 materialised input row
// ex1 / ex2 (dXg, dXn), dx and the partial rows are fp32 in both.  A bf16 buffer is 4-byte aligned (the entry checks); rows of odd width and
// replicas of an odd rows * d start 2-byte aligned: every bf16 access is one 16-bit load or store of an element of the tensor — no
// read-modify-write of a dword, no byte outside the tensor.
//
// GNX_CHAIN_BW_TRAIN (optional, 0 / 1; gnx_chain_bw_train_narrow.hip defines it 1): the training pullback k_chain_mlp_bw_train — the same text
// with the Dropout op of a training call's chains (op 7, gnx_chain_drop.h) behind `#if`, and the entries' record as a second kernel argument.
// In the forward half the dropped row goes on the tape like any layer's output; on the way back gin = d .* m with the mask regenerated; the
// entry has no accumulators, no parameter-gradient phase and no partial row.  With 0 the preprocessor leaves the two kernels above their text.
#pragma once
#include "gnx_chain_mlp.h"
#ifndef GNX_CHAIN_BW_TRAIN
#define GNX_CHAIN_BW_TRAIN 0
#endif
#if GNX_CHAIN_BW_TRAIN
#include "gnx_chain_drop.h"
#define GNX_CHAIN_BW_DROP_ARG , ChainDropArgs dr
#else
#define GNX_CHAIN_BW_DROP_ARG
#endif

namespace gnx {

struct ChainMlpBwArgs {
  ChainMlpArgs f;               // the function and the sources of its input row (f.out / f.ow unused)
  ChainBwNarrowShape sh;
  const float* G;               // upstream gradient [R][rows][width of the last layer] or nullptr
  const float* ex1; int ex1_stride, ex1_off; size_t ex1_rep;  // NODE / EDGE: dXg rows by graph, or nullptr
  const float* ex2; int ex2_stride; size_t ex2_rep;           // EDGE: dXn rows by destination node, or nullptr
  float* dx; int dx_c0;         // columns [dx_c0, K) of the row's input gradient, rows of length K - dx_c0; or nullptr
  float* direct;                // columns [0, dx_c0) (EDGE: d_ef), rows of length dx_c0; or nullptr
  float* part;                  // the partial rows, layer l at part + sh.part_off[l] * (R * nwg); or nullptr (no parameter gradient wanted)
};

constexpr int chain_bw_smax(int WMAX) { return (WMAX + 1 + 64 / WMAX - 1) / (64 / WMAX); }  // pairs per lane of a WMAX x (WMAX + 1) layer

// One layer's parameter-gradient phase over the cnt rows the wave parked: inputs at slots [xs, xs + K), deltas at [ds, ds + J).
template <int SMAX>
__device__ __forceinline__ void chain_bw_dw_phase(const float* tape, int ld, int cnt, int xs, int ds, int J, int K, float* acc_l, int lane) {
  const int NG = 64 / J, j = lane % J, kg = lane / J;
  float acc[SMAX]; int kk[SMAX];
#pragma unroll
  for (int q = 0; q < SMAX; ++q) {
    const int k = kg + NG * q;
    kk[q] = min(k, K);  // clamped: slots past the bias are summed and never written
    acc[q] = (kg < NG && k <= K) ? acc_l[k * J + j] : 0.f;
  }
  for (int i = 0; i < cnt; ++i) {
    const float dv = tape[i * ld + ds + j];
#pragma unroll
    for (int q = 0; q < SMAX; ++q)
      if (NG * q <= K) acc[q] = fmaf(dv, kk[q] < K ? tape[i * ld + xs + kk[q]] : 1.f, acc[q]);  // (uniform test)
  }
#pragma unroll
  for (int q = 0; q < SMAX; ++q) {
    const int k = kg + NG * q;
    if (kg < NG && k <= K) acc_l[k * J + j] = acc[q];
  }
}

#if !defined(GNX_CHAIN_BW_KERNEL) || !defined(GNX_CHAIN_BW_BF16)
#error "define GNX_CHAIN_BW_KERNEL and GNX_CHAIN_BW_BF16 before including gnx_chain_bw_kernel.h"
#endif
template <int WMAX, int SRC>
__global__ __launch_bounds__(256) void GNX_CHAIN_BW_KERNEL(ChainMlpBwArgs a GNX_CHAIN_BW_DROP_ARG) {
  constexpr bool BF16 = GNX_CHAIN_BW_BF16;
  extern __shared__ __attribute__((aligned(16))) float s_par[];
  constexpr int SMAX = chain_bw_smax(WMAX);
  const ChainMlpArgs& f = a.f;
  const int NT = blockDim.x, WAVES = NT >> 6, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ld = a.sh.ld, P = a.sh.P, nl = f.n_layers;
  float* const tape = s_par + a.sh.par_floats + wave * (64 * ld + P);  // this wave's rows, then its accumulators
  float* const accs = tape + 64 * ld;
  float* const my = tape + lane * ld;
  chain_stage_params<GNX_CHAIN_BW_TRAIN != 0>(f, s_par, NT);
  for (int p = lane; p < P; p += 64) accs[p] = 0.f;
  __syncthreads();
  const size_t r = blockIdx.y;
  const size_t c0 = ((size_t)blockIdx.x * WAVES + wave) * 64;  // a wave takes one chunk of 64 rows
  const int ow = f.layer[nl - 1].width;
  if (c0 < f.rows) {  // wave-uniform
    const int cnt = (int)(f.rows - c0 < 64 ? f.rows - c0 : 64);
    const bool live = lane < cnt;
    const size_t row = c0 + (live ? lane : cnt - 1);  // clamped: unconditional loads, guarded stores

    // ---- forward: the input row and every layer's output but the last onto the tape ----
    float cur[WMAX];
    if constexpr (BF16) chain_input_row_bf16<WMAX, SRC>(f, row, r, cur);
    else chain_input_row<WMAX, SRC>(f, row, r, cur);
#pragma unroll
    for (int k = 0; k < WMAX; ++k)
      if (k < f.K) my[k] = cur[k];
    {
      int kin = f.K;
#pragma unroll 1
      for (int l = 0; l < nl; ++l) {
        const int width = f.layer[l].width, op = f.layer[l].op;
#if GNX_CHAIN_BW_TRAIN
        if (op == kChainOpDropout) chain_drop_row<WMAX>(dr.seed, dr.stream[l], dr.p[l], dr.scale[l], (r * f.rows + row) * (size_t)width, width, cur);
        else
#endif
        if (l == nl - 1 && op == GNX_ACT_GELU) (void)chain_layer_fw<WMAX>(s_par, a.sh.par_off[l], kin, width, GNX_ACT_IDENTITY, cur);  // its pre-activation is all the way back reads
        else (void)chain_layer_fw<WMAX>(s_par, a.sh.par_off[l], kin, width, op, cur);
        if (l < nl - 1) {
#pragma unroll
          for (int k = 0; k < WMAX; ++k)
            if (k < width) my[a.sh.tape_out[l] + k] = cur[k];
        }
        kin = width;
      }
    }

    // ---- delta of the last layer: (upstream + the shares of the levels above) .* act' ----
    float d[WMAX];
    {
      const int op = f.layer[nl - 1].op, act = op < 5 ? op : GNX_ACT_IDENTITY;
      const typename ElemOf<BF16>::T* __restrict__ gp = a.G ? feat<BF16>(a.G) + (r * f.rows + row) * (size_t)ow : nullptr;
      const float* __restrict__ e1 = nullptr;
      const float* __restrict__ e2 = nullptr;
      if constexpr (SRC != SRC_ROWS) {
        if (a.ex1) e1 = a.ex1 + r * a.ex1_rep + (size_t)segment_of(f.seg_off, f.G, (int)row) * a.ex1_stride + a.ex1_off;
      }
      if constexpr (SRC == SRC_EDGE) {
        if (a.ex2) e2 = a.ex2 + r * a.ex2_rep + (size_t)f.edge_dst[row] * a.ex2_stride;
      }
#pragma unroll
      for (int k = 0; k < WMAX; ++k) {
        float g = 0.f;
        if (k < ow) {
          if constexpr (BF16) { if (gp) g = bf16_lo(gp[k]); }
          else { if (gp) g = gp[k]; }
          if (e1) g += e1[k];
          if (e2) g += e2[k];
          g *= act_grad_bw(cur[k], act);
        }
        d[k] = g;
      }
    }

    // ---- back through the layers ----
#pragma unroll 1
    for (int l = nl - 1; l >= 0; --l) {
      const int width = f.layer[l].width, op = f.layer[l].op;
      const int kin = l > 0 ? f.layer[l - 1].width : f.K, xs = l > 0 ? a.sh.tape_out[l - 1] : 0;
      const float* __restrict__ sp = s_par + a.sh.par_off[l];
      const bool want_gin = l > 0 || a.dx || a.direct;
      float gin[WMAX];
#pragma unroll
      for (int k = 0; k < WMAX; ++k) gin[k] = 0.f;
#if GNX_CHAIN_BW_TRAIN
      if (op == kChainOpDropout) {  // gin = d .* m, the forward's mask again
#pragma unroll
        for (int k = 0; k < WMAX; ++k) gin[k] = d[k];
        chain_drop_row<WMAX>(dr.seed, dr.stream[l], dr.p[l], dr.scale[l], (r * f.rows + row) * (size_t)width, width, gin);
      } else
#endif
      if (op < 5) {
        if (a.part) {
#pragma unroll
          for (int k = 0; k < WMAX; ++k)
            if (k < width) my[a.sh.dslot + k] = d[k];
          __builtin_amdgcn_wave_barrier();
          chain_bw_dw_phase<SMAX>(tape, ld, cnt, xs, a.sh.dslot, width, kin, accs + a.sh.part_off[l], lane);
          __builtin_amdgcn_wave_barrier();  // (the next layer's deltas overwrite these)
        }
        if (want_gin) {
          const int OP = ceil4(width);
#pragma unroll
          for (int k = 0; k < WMAX; ++k) {
            if (k < kin) {
              float acc = 0.f;
#pragma unroll
              for (int j0 = 0; j0 < WMAX; j0 += 4) {
                if (j0 < width) {
                  const float4 wv = *reinterpret_cast<const float4*>(sp + k * OP + j0);  // (the padding of W and of d is 0)
                  acc = fmaf(wv.x, d[j0], acc); acc = fmaf(wv.y, d[j0 + 1], acc); acc = fmaf(wv.z, d[j0 + 2], acc); acc = fmaf(wv.w, d[j0 + 3], acc);
                }
              }
              gin[k] = acc;
            }
          }
        }
      } else {
        // k_ln_backward with one norm: x from the tape, the statistics again, dx = (dxh - mean(dxh)) / sden - c * coef, dxh = dy .* gamma
        float c[WMAX];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < WMAX; ++k) { c[k] = k < width ? my[xs + k] : 0.f; s += c[k]; }
        const float mu = s / (float)width;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < WMAX; ++k)
          if (k < width) { c[k] -= mu; v = fmaf(c[k], c[k], v); }
        v /= (float)width;
        const float sigma = sqrtf(v);
        const float sden = op == 5 ? sigma + kChainLnEps : sqrtf(v + kChainLnEps);
        const float q = op == 5 ? sigma * sden * sden : sden * sden * sden;
        float sum_dxh = 0.f, sum_dxh_c = 0.f;
#pragma unroll
        for (int k0 = 0; k0 < WMAX; k0 += 4) {
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
        if (a.part) {  // [dy ; dy .* xhat] behind the tape: lane j < width sums dgamma[j], lane width + j sums dbeta[j]
#pragma unroll
          for (int k = 0; k < WMAX; ++k)
            if (k < width) { my[a.sh.dslot + k] = d[k]; my[a.sh.dslot + width + k] = d[k] * (c[k] / sden); }
          __builtin_amdgcn_wave_barrier();
          if (lane < 2 * width) {
            float* const ap = accs + a.sh.part_off[l] + lane;
            const int slot = a.sh.dslot + (lane < width ? width + lane : lane - width);
            float acc = *ap;
            for (int i = 0; i < cnt; ++i) acc += tape[i * ld + slot];
            *ap = acc;
          }
          __builtin_amdgcn_wave_barrier();
        }
        const float mean_dxh = sum_dxh / (float)width;
        const float coef = q > 0.f ? sum_dxh_c / ((float)width * q) : 0.f;
#pragma unroll
        for (int k = 0; k < WMAX; ++k) gin[k] = k < width ? (gin[k] - mean_dxh) / sden - c[k] * coef : 0.f;
      }
      if (l > 0) {  // delta of layer l - 1 from the gradient w.r.t. its output
        const int pop = f.layer[l - 1].op;
        if (pop >= 5 || pop == GNX_ACT_IDENTITY) {
#pragma unroll
          for (int k = 0; k < WMAX; ++k) d[k] = gin[k];
        } else {
          float y[WMAX];
          if (pop == GNX_ACT_GELU) {  // its pre-activation, from its input on the tape
            const int kin1 = l > 1 ? f.layer[l - 2].width : f.K, xs1 = l > 1 ? a.sh.tape_out[l - 2] : 0;
#pragma unroll
            for (int k = 0; k < WMAX; ++k) y[k] = k < kin1 ? my[xs1 + k] : 0.f;
            (void)chain_layer_fw<WMAX>(s_par, a.sh.par_off[l - 1], kin1, kin, GNX_ACT_IDENTITY, y);
          } else {
#pragma unroll
            for (int k = 0; k < WMAX; ++k) y[k] = k < kin ? my[xs + k] : 0.f;
          }
#pragma unroll
          for (int k = 0; k < WMAX; ++k) d[k] = k < kin ? gin[k] * act_grad_bw(y[k], pop) : 0.f;
        }
      } else if (live) {
        const size_t at = r * f.rows + row;
        if (a.direct) {
          if constexpr (BF16) {
            bf16_t* __restrict__ o = reinterpret_cast<bf16_t*>(a.direct) + at * (size_t)a.dx_c0;
#pragma unroll
            for (int k = 0; k < WMAX; ++k)
              if (k < a.dx_c0) o[k] = to_bf16(gin[k]);
          } else {
            float* __restrict__ o = a.direct + at * (size_t)a.dx_c0;
#pragma unroll
            for (int k = 0; k < WMAX; ++k)
              if (k < a.dx_c0) o[k] = gin[k];
          }
        }
        if (a.dx) {
          float* __restrict__ o = a.dx + at * (size_t)(f.K - a.dx_c0);
#pragma unroll
          for (int k = 0; k < WMAX; ++k)
            if (k >= a.dx_c0 && k < f.K) o[k - a.dx_c0] = gin[k];
        }
      }
    }
  }
  if (!a.part) return;  // uniform
  __syncthreads();
  const size_t wg = r * gridDim.x + blockIdx.x, nwg = (size_t)gridDim.x * gridDim.y;
  const float* const acc0 = s_par + a.sh.par_floats + 64 * ld;
  const int stride = 64 * ld + P;
  int kin = f.K;
  for (int l = 0; l < nl; ++l) {
    const int width = f.layer[l].width;
#if GNX_CHAIN_BW_TRAIN
    if (f.layer[l].op == kChainOpDropout) continue;  // (no parameters; its width is kin)
#endif
    const int Pl = f.layer[l].op < 5 ? width * (kin + 1) : 2 * width, at = a.sh.part_off[l];
    float* __restrict__ out = a.part + (size_t)at * nwg + wg * (size_t)Pl;
    for (int p = threadIdx.x; p < Pl; p += NT) {
      float v = acc0[at + p];
      for (int ww = 1; ww < WAVES; ++ww) v += acc0[ww * stride + at + p];
      out[p] = v;
    }
    kin = width;
  }
}

// What the two launchers do before their launch: the prologue under the pullback's rule, the LDS plan, the record; *lds: the dynamic LDS in bytes
inline int32_t chain_bw_narrow_args(const gnx_graphs* h, int entity, const gnx_chain& c, const float* in0, int d0, const float* in1, int d1, const float* in2, int d2,
                                    const ChainBwNarrowIo& io, const char* who, hipStream_t s, ChainMlpBwArgs& a, int* wmax, size_t* lds) {
  size_t rows;
  if (int32_t rc = chain_mlp_prologue(h, entity, c, in0, d0, in1, d1, in2, d2, CHAIN_RULE_BW, who, s, a.f, wmax, &rows)) return rc;
  a.sh = chain_bw_narrow_shape(c, a.f.K, rows);
  a.G = io.G;
  a.ex1 = io.ex1; a.ex1_stride = io.ex1_stride; a.ex1_off = io.ex1_off; a.ex1_rep = (size_t)h->G * io.ex1_stride;
  a.ex2 = io.ex2; a.ex2_stride = io.ex2_stride; a.ex2_rep = (size_t)h->N * io.ex2_stride;
  a.dx = io.dx; a.dx_c0 = io.dx_c0; a.direct = io.direct; a.part = io.part;
  *lds = sizeof(float) * ((size_t)a.sh.par_floats + (size_t)a.sh.waves * (64 * a.sh.ld + a.sh.P));
  return GNX_OK;
}

}  // namespace gnx
