// The Dropout op of the fused Chain training kernels: k_chain_mlp_train (gnx_chain_train_narrow.hip) and k_chain_mlp_bw_train
// (gnx_chain_bw_train_narrow.hip) regenerate the mask of a lane's row in registers with this code.  The mask is gnx_chain_dropout_mask's, bit
// for bit (include/gnx.h): element k of the row that starts at flat index i0 = (r * rows + row) * w takes component (i0 + k) % 4 of
// philox4((i0 + k) / 4, stream, seed) through mask_of — what launch_dropout computes on the packed [R][rows][w] tensor.
#pragma once
#include "gnx_chain_plan.h"
#include "gnx_philox.h"

namespace gnx {

// the Dropout entries of one function: layer l's p, scale and stream id where layer l is a Dropout entry (op 7 of ChainMlpLayer)
constexpr int kChainOpDropout = 7;
struct ChainDropArgs {
  uint64_t seed;
  float p[kChainMaxLayers], scale[kChainMaxLayers];
  uint32_t stream[kChainMaxLayers];
};
inline ChainDropArgs chain_drop_args(const gnx_chain& c) {
  ChainDropArgs d{};
  for (int i = 0; i < c.n_layers; ++i) {
    if (!chain_layer_is_dropout(c.layers[i])) continue;
    const ChainDropSite* st = chain_drop_site(c.layers[i]);
    d.seed = st->seed;
    d.p[i] = st->p; d.scale[i] = st->p < 1.f ? 1.f / (1.f - st->p) : 0.f; d.stream[i] = st->stream;
  }
  return d;
}

// v[k] <- v[k] * m[k] for k < w, one fp32 multiply each.  The row's w elements lie in at most (3 + w + 3) / 4 consecutive Philox blocks from
// quad i0 / 4 (64-bit) on; each block is generated once and consumed before the next: position 4 q + j of the blocks is element 4 q + j - o of
// the row, o = i0 % 4 — selects over constant positions, the register array is never indexed by a variable.  Entries at or beyond w (exactly
// 0.f) stay 0.f.  The test of a block against the width is wave-uniform.
template <int WMAX>
__device__ __forceinline__ void chain_drop_row(uint64_t seed, uint32_t stream, float p, float scale, size_t i0, int w, float (&v)[WMAX]) {
  const uint64_t quad0 = (uint64_t)i0 >> 2;
  const int o = (int)(i0 & 3);
#pragma unroll
  for (int q = 0; q < (WMAX + 6) / 4; ++q) {
    if (4 * q < w + 3) {
      uint32_t c[4];
      philox4(quad0 + q, stream, seed, c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float m = mask_of(c[j], p, scale);
#pragma unroll
        for (int oo = 0; oo < 4; ++oo) {
          const int k = 4 * q + j - oo;
          if (k >= 0 && k < WMAX) v[k] = (o == oo && k < w) ? v[k] * m : v[k];
        }
      }
    }
  }
}

}  // namespace gnx
