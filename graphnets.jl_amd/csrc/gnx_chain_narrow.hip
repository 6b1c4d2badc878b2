// GNBlock with Chain update functions at narrow widths: one update function = one kernel (gnx_chain_block_forward_narrow, gnx_chain.cpp).
//
//   k_chain_mlp<WMAX, SRC> : one lane = one row of the entity; the lane builds the function's input row in registers (SRC), runs it through
//                            ALL layers of the function — Dense with any activation, LayerNorm layer values — and stores the last layer's row.
//
// SRC_EDGE  [ef[e] ; nf[rowval[e]] ; nf[edge_dst[e]] ; gf[graph(e)]]                 (getedgefninput, gnblock.jl:65; k_fn_input_edge)
// SRC_NODE  [sum_{e in colptr[n] .. colptr[n+1]} ef'[e] ; nf[n] ; gf[graph(n)]]     (getnodefninput; sequential fp32 adds in CSC order: the bits
//                                                                                      of k_fn_input_node)
// SRC_ROWS  a materialised [rows][K] buffer                                          (the graph function behind launch_fn_input(kind 2))
//
// The current and the next activations are float[WMAX] arrays indexed by unrolled constants only (registers, no scratch:
// profiles/chain_narrow_resources.json); WMAX in {8, 16, 32} is the smallest that covers the input width and every layer width.  Entries at or
// beyond a layer's width are kept at exactly 0.f.  The function's parameters are staged in LDS once per workgroup, zero-padded to groups of
// four — a Dense as [ceil4(k_in)][ceil4(width)] weights (element (j, k) at k * ceil4(width) + j) + ceil4(width) biases, a LayerNorm as gamma and
// beta — and read with uniform addresses (a ds_read_b128 of one address is a broadcast, as in core_post_lds_body: gnx_core_post_kernel.h).
// A layer's products run as groups of 4 outputs x 4 inputs behind wave-uniform tests of the group against the layer's widths: a 16 -> 3 layer
// pays 4 x 1 groups, not the 32-wide tile of the matrix-core GEMM.  Every group is a basic block of its own, so the scheduler cannot hoist the
// weight reads of a whole layer into registers (the hazard the sched_barriers of core_post_lds_body fence).
// Feature and output pointers may be 4-byte aligned only: every global access is one dword.  Offsets are size_t.
#include "gnx_chain_mlp.h"  // the argument record, the parameter staging and the input row: shared with k_chain_mlp_bw (its chain_layer_fw is the loop below)

namespace gnx {

template <int WMAX, int SRC>
__global__ __launch_bounds__(256) void k_chain_mlp(ChainMlpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_par[];
  chain_stage_params(a, s_par, 256);
  __syncthreads();
  const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= a.rows) return;
  const size_t r = blockIdx.y;

  float cur[WMAX];
  chain_input_row<WMAX, SRC>(a, row, r, cur);

  int off = 0, kin = a.K;
#pragma unroll 1
  for (int l = 0; l < a.n_layers; ++l) {
    const int width = a.layer[l].width, op = a.layer[l].op;
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
      off += ceil4(kin) * OP + OP;
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
      off += 2 * OP;
    }
    kin = width;
  }

  float* __restrict__ o = a.out + (r * a.rows + row) * (size_t)a.ow;
#pragma unroll
  for (int k = 0; k < WMAX; ++k)
    if (k < a.ow) o[k] = cur[k];
}

// One update function of a Chain block in one launch.  entity 0: in0 / in1 / in2 = ef, nf, gf of widths d0, d1, d2 (SRC_EDGE); 1: ef', nf, gf
// (SRC_NODE); 2: in0 = the materialised [R G][d0] input rows (SRC_ROWS; d1 = d2 = 0).  The caller asked chain_narrow_takes (gnx_chain_plan.h).
int32_t launch_chain_narrow(const gnx_graphs* h, int entity, const gnx_chain& c, const float* in0, int d0, const float* in1, int d1, const float* in2, int d2,
                            float* out, int64_t R, hipStream_t s, const char* name) {
  if (chain_has_dropout(c)) return launch_chain_narrow_train(h, entity, c, in0, d0, in1, d1, in2, d2, out, R, s, name);  // (a training call: gnx_chain_train_narrow.hip)
  ChainMlpArgs a{};
  int wmax;
  size_t rows;
  if (int32_t rc = chain_mlp_prologue(h, entity, c, in0, d0, in1, d1, in2, d2, CHAIN_RULE_FW, "launch_chain_narrow", s, a, &wmax, &rows)) return rc;
  a.out = out; a.ow = c.widths[c.n_layers - 1];
  const dim3 grid((unsigned)((rows + 255) / 256), (unsigned)R);
  const size_t lds = sizeof(float) * chain_narrow_lds_floats(c, a.K);
  ProfScope ps(name, s);
  chain_mlp_dispatch(wmax, entity, [&](auto W, auto S) { GNX_LAUNCH((k_chain_mlp<decltype(W)::value, decltype(S)::value>), grid, dim3(256), lds, s, a); });
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
