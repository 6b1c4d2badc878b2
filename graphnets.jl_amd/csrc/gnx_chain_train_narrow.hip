// GNBlock with Chain update functions in training mode at narrow widths: one update function with Dropout entries = one kernel
// (gnx_chain_block_forward_train with narrow = 1, gnx_chain.cpp; the recompute of gnx_chain_block_backward_train, gnx_backward.hip).
//
//   k_chain_mlp_train<WMAX, SRC> : k_chain_mlp (gnx_chain_narrow.hip) with a Dropout op.  One lane = one row of the entity: the lane builds the
//                                  function's input row (chain_input_row), runs it through all layers (chain_layer_fw: k_chain_mlp's layer,
//                                  operation for operation — a chain's Dense and LayerNorm layers carry that kernel's bits) and, at a Dropout
//                                  entry, multiplies its row by the mask it regenerates in registers (chain_drop_row, gnx_chain_drop.h).
//
// The mask of Dropout entry l of function t is a pure function of (seed, 16 + 16 t + l, flat element index): nothing is stored, and the bits are
// those of the k_dropout launch the generic path makes for the entry.  The layers run as calls of chain_layer_fw and not as k_chain_mlp's loop
// in place: that kernel keeps its device code, and the cost of the call form (registers at WMAX = 32) stays inside the budget — no instantiation
// uses scratch (profiles/chain_train_narrow_resources.json).  Parameters in LDS, the width tests and the 4-byte alignment of every global
// access as in k_chain_mlp; a Dropout entry stages nothing.
#include "gnx_chain_drop.h"
#include "gnx_chain_mlp.h"

namespace gnx {

template <int WMAX, int SRC>
__global__ __launch_bounds__(256) void k_chain_mlp_train(ChainMlpArgs a, ChainDropArgs dr) {
  extern __shared__ __attribute__((aligned(16))) float s_par[];
  chain_stage_params<true>(a, s_par, 256);
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
    if (op == kChainOpDropout) chain_drop_row<WMAX>(dr.seed, dr.stream[l], dr.p[l], dr.scale[l], (r * a.rows + row) * (size_t)width, width, cur);
    else off = chain_layer_fw<WMAX>(s_par, off, kin, width, op, cur);
    kin = width;
  }

  float* __restrict__ o = a.out + (r * a.rows + row) * (size_t)a.ow;
#pragma unroll
  for (int k = 0; k < WMAX; ++k)
    if (k < a.ow) o[k] = cur[k];
}

// launch_chain_narrow for a function with Dropout entries (the caller asked the training forward's rule: chain_narrow_takes)
int32_t launch_chain_narrow_train(const gnx_graphs* h, int entity, const gnx_chain& c, const float* in0, int d0, const float* in1, int d1, const float* in2, int d2,
                                  float* out, int64_t R, hipStream_t s, const char* name) {
  ChainMlpArgs a{};
  int wmax;
  size_t rows;
  if (int32_t rc = chain_mlp_prologue(h, entity, c, in0, d0, in1, d1, in2, d2, CHAIN_RULE_FW, "launch_chain_narrow_train", s, a, &wmax, &rows)) return rc;
  for (int i = 0; i < c.n_layers; ++i)
    if (chain_layer_is_dropout(c.layers[i]) && !chain_drop_site(c.layers[i])) return fail(GNX_ERR_INVALID_ARG, "Chain: a Dropout entry outside a training call");
  const ChainDropArgs dr = chain_drop_args(c);
  a.out = out; a.ow = c.widths[c.n_layers - 1];
  const dim3 grid((unsigned)((rows + 255) / 256), (unsigned)R);
  const size_t lds = sizeof(float) * chain_narrow_lds_floats(c, a.K);
  ProfScope ps(name, s);
  chain_mlp_dispatch(wmax, entity, [&](auto W, auto S) { GNX_LAUNCH((k_chain_mlp_train<decltype(W)::value, decltype(S)::value>), grid, dim3(256), lds, s, a, dr); });
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
