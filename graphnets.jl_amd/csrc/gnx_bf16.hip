// Conversions around the fp32 forward for gnx_block_forward_typed(elem = GNX_ELEM_BF16) on the paths without a native bf16 kernel
// (matrix-core / generic widths, GNX_FLAG_FORCE_GENERIC, GNX_FLAG_NO_JIT, a failed run-time specialisation): the inputs are widened into
// fp32 staging buffers of the workspace, gnx_block_forward runs on them, the outputs are rounded to bf16 (nearest even).  Widening is exact,
// and the rounding is the one the fused kernels apply on store (pack_bf16 / to_bf16 of gnx_wave_kernel.h): every path gives the same bits.
#include "gnx_launchers.h"
#include "gnx_wave_kernel.h"

namespace gnx {

namespace {

constexpr int kConvThreads = 256;

// 8 elements per thread: four dwords of a 4-B aligned bf16 buffer in one load, two float4 stores into the (16-B aligned) staging buffer.
// The last thread's partial group reads the dwords that hold its elements (never a dword without a byte of the buffer).
__global__ __launch_bounds__(kConvThreads) void k_bf16_widen(const unsigned* __restrict__ src, size_t n, float4* __restrict__ dst) {
  const size_t t = blockIdx.x * (size_t)kConvThreads + threadIdx.x;
  const size_t e0 = 8 * t;
  if (e0 >= n) return;
  if (e0 + 8 <= n) {
    const U4u v = *reinterpret_cast<const U4u*>(src + 4 * t);
    dst[2 * t] = make_float4(bf16_lo(v.x), bf16_hi(v.x), bf16_lo(v.y), bf16_hi(v.y));
    dst[2 * t + 1] = make_float4(bf16_lo(v.z), bf16_hi(v.z), bf16_lo(v.w), bf16_hi(v.w));
  } else {
    float* d = reinterpret_cast<float*>(dst);
    for (size_t e = e0; e < n; ++e) {
      const unsigned w = src[e >> 1];
      d[e] = (e & 1) ? bf16_hi(w) : bf16_lo(w);
    }
  }
}

// 8 elements per thread: two float4 loads, four dwords of packed bf16 in one store; a partial last group writes whole pairs as dwords and
// a lone last element as a 16-bit store (the other half of its dword lies outside the buffer)
__global__ __launch_bounds__(kConvThreads) void k_bf16_round(const float4* __restrict__ src, size_t n, unsigned* __restrict__ dst) {
  const size_t t = blockIdx.x * (size_t)kConvThreads + threadIdx.x;
  const size_t e0 = 8 * t;
  if (e0 >= n) return;
  if (e0 + 8 <= n) {
    const float4 a = src[2 * t], b = src[2 * t + 1];
    U4u v;
    v.x = pack_bf16(a.x, a.y); v.y = pack_bf16(a.z, a.w); v.z = pack_bf16(b.x, b.y); v.w = pack_bf16(b.z, b.w);
    *reinterpret_cast<U4u*>(dst + 4 * t) = v;
  } else {
    const float* s = reinterpret_cast<const float*>(src);
    size_t e = e0;
    for (; e + 2 <= n; e += 2) dst[e >> 1] = pack_bf16(s[e], s[e + 1]);
    if (e < n) reinterpret_cast<bf16_t*>(dst)[e] = to_bf16(s[e]);
  }
}

unsigned conv_blocks(size_t n) { return (unsigned)((n + 8 * (size_t)kConvThreads - 1) / (8 * (size_t)kConvThreads)); }

}  // namespace

// src: n bf16 values (4-B aligned), dst: n floats (16-B aligned)
int32_t launch_bf16_widen(const void* src, size_t n, float* dst, hipStream_t s) {
  if (n == 0) return GNX_OK;
  ProfScope ps("k_bf16_widen", s);
  GNX_LAUNCH(k_bf16_widen, dim3(conv_blocks(n)), dim3(kConvThreads), 0, s, static_cast<const unsigned*>(src), n, reinterpret_cast<float4*>(dst));
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

// src: n floats (16-B aligned), dst: n bf16 values (4-B aligned)
int32_t launch_bf16_round(const float* src, size_t n, void* dst, hipStream_t s) {
  if (n == 0) return GNX_OK;
  ProfScope ps("k_bf16_round", s);
  GNX_LAUNCH(k_bf16_round, dim3(conv_blocks(n)), dim3(kConvThreads), 0, s, reinterpret_cast<const float4*>(src), n, static_cast<unsigned*>(dst));
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
