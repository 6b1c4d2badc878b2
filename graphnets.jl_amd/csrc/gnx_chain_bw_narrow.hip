// The pullback of one Chain update function at narrow widths in one kernel (gnx_chain_block_backward_narrow, gnx_backward.hip).
//
//   k_chain_mlp_bw<WMAX, SRC> : one lane = one row of the entity.  The lane builds the function's input row (chain_input_row: the forward kernel's
//   code), runs it forward through all layers (chain_layer_fw: the forward kernel's operation order) and walks back through them in registers.
//
// What the way back needs lives on a per-lane tape in LDS: the input row and the output of every layer but the last, `ld` floats per lane, ld odd,
// lane l at [l * ld, (l + 1) * ld) — a lane's accesses to its own row fall on 64 different banks.  A gelu layer's pre-activation and a LayerNorm's
// mean and deviation are recomputed from the layer's input on the tape (the forward's operations again, so the same bits); nothing else is kept.
//   last-layer delta   (G + ex1[graph] + ex2[dst]) * act'          k_bw_delta's sum order and derivative formulas (act_grad_bw)
//   Dense              g_in[k] = sum_j W[k][j] delta[j], j ascending (k_bw_dx's order), then delta <- g_in .* act'(previous layer)
//   LayerNorm          k_ln_backward's formula for one norm, the row's sums taken by the lane in element order
// The input gradient of the row is stored (graph / node: the whole row into dXg / dXn; edge: the ef columns into d_ef, the node / graph columns
// into the compact [R E][2 dn + dg] tensor that k_bw_dnf and the d_gf column sums read); hidden rows and deltas never reach memory.
//
// Parameter gradients, as in k_core_bw_narrow (no atomics, a fixed order): for every layer on the way back the wave parks its 64 deltas behind
// the tape, and lane l owns the pairs (k, j = l % J) for k = l / J + (64 / J) q — k == K is the bias, whose input is 1.  A wave takes one chunk
// of 64 rows and sums it in row order into its LDS slice (a loop over chunks would keep every width test of the body alive in scalar registers
// across it: more than the register file has); a workgroup — two to four waves under the rule, as many as fit 64 KB of LDS — adds its waves in
// wave order and writes one partial row per layer in k_bw_dw_final's pair order (p = k * J + j; a LayerNorm as J = width, K = 1: gamma then beta), which
// k_bw_dw_final finishes over the workgroups.  Every accumulator starts at 0: the results do not depend on what the workspace held.
// Every global access is one dword (4-byte aligned buffers are enough); offsets are size_t.  No instantiation uses scratch
// (profiles/chain_bw_narrow_resources.json): register arrays are indexed by unrolled constants only.
#include <algorithm>

#include "gnx_chain_mlp.h"

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

template <int WMAX, int SRC>
__global__ __launch_bounds__(256) void k_chain_mlp_bw(ChainMlpBwArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_par[];
  constexpr int SMAX = chain_bw_smax(WMAX);
  const ChainMlpArgs& f = a.f;
  const int NT = blockDim.x, WAVES = NT >> 6, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ld = a.sh.ld, P = a.sh.P, nl = f.n_layers;
  float* const tape = s_par + a.sh.par_floats + wave * (64 * ld + P);  // this wave's rows, then its accumulators
  float* const accs = tape + 64 * ld;
  float* const my = tape + lane * ld;
  chain_stage_params(f, s_par, NT);
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
    chain_input_row<WMAX, SRC>(f, row, r, cur);
#pragma unroll
    for (int k = 0; k < WMAX; ++k)
      if (k < f.K) my[k] = cur[k];
    {
      int kin = f.K;
#pragma unroll 1
      for (int l = 0; l < nl; ++l) {
        const int width = f.layer[l].width, op = f.layer[l].op;
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
      const float* __restrict__ gp = a.G ? a.G + (r * f.rows + row) * (size_t)ow : nullptr;
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
          if (gp) g = gp[k];
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
          float* __restrict__ o = a.direct + at * (size_t)a.dx_c0;
#pragma unroll
          for (int k = 0; k < WMAX; ++k)
            if (k < a.dx_c0) o[k] = gin[k];
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

// The caller asked chain_bw_narrow_takes (gnx_chain_plan.h: the rule and the LDS plan, chain_bw_narrow_shape) and opens the ProfScope.
int32_t launch_chain_bw_narrow(const gnx_graphs* h, int entity, const gnx_chain& c, const float* in0, int d0, const float* in1, int d1, const float* in2, int d2,
                               const ChainBwNarrowIo& io, int64_t R, hipStream_t s) {
  ChainMlpBwArgs a{};
  int wmax;
  size_t rows;
  if (int32_t rc = chain_mlp_prologue(h, entity, c, in0, d0, in1, d1, in2, d2, CHAIN_RULE_BW, "launch_chain_bw_narrow", s, a.f, &wmax, &rows)) return rc;
  a.sh = chain_bw_narrow_shape(c, a.f.K, rows);
  a.G = io.G;
  a.ex1 = io.ex1; a.ex1_stride = io.ex1_stride; a.ex1_off = io.ex1_off; a.ex1_rep = (size_t)h->G * io.ex1_stride;
  a.ex2 = io.ex2; a.ex2_stride = io.ex2_stride; a.ex2_rep = (size_t)h->N * io.ex2_stride;
  a.dx = io.dx; a.dx_c0 = io.dx_c0; a.direct = io.direct; a.part = io.part;
  const dim3 grid((unsigned)a.sh.nwg, (unsigned)R), block(64 * a.sh.waves);
  const size_t lds = sizeof(float) * ((size_t)a.sh.par_floats + (size_t)a.sh.waves * (64 * a.sh.ld + a.sh.P));
  chain_mlp_dispatch(wmax, entity, [&](auto W, auto S) { GNX_LAUNCH((k_chain_mlp_bw<decltype(W)::value, decltype(S)::value>), grid, block, lds, s, a); });
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
