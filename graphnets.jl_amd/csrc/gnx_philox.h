// The Dropout mask's generator (device code): Philox-4x32-10 and the map from 32 random bits to a mask value.  Element i of entity t's mask is
// component i % 4 of philox4(i / 4, t, seed) through mask_of — a pure function of (seed, t, i) — so every kernel that includes this header
// (k_dropout in gnx_dropout.hip, k_core_post_train in gnx_core_train_narrow.hip) regenerates the same mask bit for bit.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace gnx {

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
  const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
  const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
  c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
}
// Philox-4x32-10 (Salmon et al., SC'11): counter (quad index, entity), key = the seed
__device__ __forceinline__ void philox4(uint64_t quad, uint32_t entity, uint64_t seed, uint32_t (&out)[4]) {
  uint32_t c[4] = {(uint32_t)quad, (uint32_t)(quad >> 32), entity, 0x676e78u};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = c[i];
}
// Flux._dropout_kernel(y, p, q) = y > p ? 1 / q : 0 with y uniform on [0, 1): 24 random bits -> a float on the grid k / 2^24
__device__ __forceinline__ float mask_of(uint32_t bits, float p, float scale) { return (float)(bits >> 8) * 0x1p-24f > p ? scale : 0.f; }

}  // namespace gnx
