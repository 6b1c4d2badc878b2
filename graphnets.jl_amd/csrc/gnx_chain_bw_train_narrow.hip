// The pullback of one Chain update function with Dropout entries at narrow widths in one kernel (gnx_chain_block_backward_train with narrow = 1,
// gnx_backward.hip).
//
//   k_chain_mlp_bw_train<WMAX, SRC> : k_chain_mlp_bw's text (gnx_chain_bw_kernel.h, included below with GNX_CHAIN_BW_TRAIN) with the Dropout op.
//   Forward half: at a Dropout entry the lane multiplies its row by the mask it regenerates in registers (chain_drop_row, gnx_chain_drop.h — the
//   bits of the training forward kernel and of the generic path's k_dropout launch) and the dropped row goes on the tape, where the Dense behind
//   the entry finds its input.  Way back: gin = d .* m, the mask regenerated again; the delta of the layer in front then uses that layer's own,
//   undropped output from its tape slot.  A Dropout as last entry multiplies the summed last delta (upstream + the shares of the levels above).
//   The entry has no accumulators, no parameter-gradient phase and no partial row: the LDS plan is chain_bw_narrow_shape's (gnx_chain_plan.h).
// Everything else — the tape, the deltas, the accumulators, the partial rows, the summation orders — is k_chain_mlp_bw's.
#include <algorithm>

#define GNX_CHAIN_BW_KERNEL k_chain_mlp_bw_train  // template <int WMAX, int SRC> __global__ void k_chain_mlp_bw_train(ChainMlpBwArgs, ChainDropArgs)
#define GNX_CHAIN_BW_BF16 false
#define GNX_CHAIN_BW_TRAIN 1
#include "gnx_chain_bw_kernel.h"

namespace gnx {

// launch_chain_bw_narrow for a function with Dropout entries.  The caller asked the training pullback's rule and opens the ProfScope.
int32_t launch_chain_bw_narrow_train(const gnx_graphs* h, int entity, const gnx_chain& c, const float* in0, int d0, const float* in1, int d1, const float* in2,
                                     int d2, const ChainBwNarrowIo& io, int64_t R, hipStream_t s) {
  ChainMlpBwArgs a{};
  int wmax;
  size_t lds;
  if (int32_t rc = chain_bw_narrow_args(h, entity, c, in0, d0, in1, d1, in2, d2, io, "launch_chain_bw_narrow_train", s, a, &wmax, &lds)) return rc;
  for (int i = 0; i < c.n_layers; ++i)
    if (chain_layer_is_dropout(c.layers[i]) && !chain_drop_site(c.layers[i])) return fail(GNX_ERR_INVALID_ARG, "Chain: a Dropout entry outside a training call");
  const ChainDropArgs dr = chain_drop_args(c);
  const dim3 grid((unsigned)a.sh.nwg, (unsigned)R), block(64 * a.sh.waves);
  chain_mlp_dispatch(wmax, entity, [&](auto W, auto S) { GNX_LAUNCH((k_chain_mlp_bw_train<decltype(W)::value, decltype(S)::value>), grid, block, lds, s, a, dr); });
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
