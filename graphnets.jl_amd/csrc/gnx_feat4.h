// Four consecutive elements of a feature buffer in one access: the LayerNorm kernels of a GNCore and the delta kernels of the block backward,
// whose lanes own four columns of a row.  fp32: one 16-byte access; bfloat16: one 8-byte access, widened on load (exact) and rounded to nearest
// even on store (pack_bf16 = two to_bf16).  Feature pointers are declared float whatever they hold, like those of BlockArgs.
#pragma once
#include "gnx_wave_kernel.h"

namespace gnx {
namespace {

// four consecutive bf16 elements from element i of a feature buffer (i % 4 == 0, base 8-B aligned), widened
__device__ __forceinline__ float4 ld_bf16x4(const float* base, size_t i) {
  const uint2 w = *reinterpret_cast<const uint2*>(reinterpret_cast<const bf16_t*>(base) + i);
  return make_float4(bf16_lo(w.x), bf16_hi(w.x), bf16_lo(w.y), bf16_hi(w.y));
}
// quad c of the row that starts at element `row0` of a feature buffer (row0 % 4 == 0; base 16-B aligned, 8-B for bf16)
template <bool BF16>
__device__ __forceinline__ float4 ld_feat4(const float* base, size_t row0, int c) {
  if constexpr (BF16) return ld_bf16x4(base, row0 + 4 * (size_t)c);
  else return reinterpret_cast<const float4*>(base + row0)[c];
}
template <bool BF16>
__device__ __forceinline__ void st_feat4(float* base, size_t row0, int c, float4 v) {
  if constexpr (BF16) *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(base) + row0 + 4 * (size_t)c) = make_uint2(pack_bf16(v.x, v.y), pack_bf16(v.z, v.w));
  else reinterpret_cast<float4*>(base + row0)[c] = v;
}

}  // namespace
}  // namespace gnx
