// GNCore in training mode at narrow widths (D <= 16): FeedForward + Dropout + both residuals in one kernel per entity
// (gnx_core_forward_train_typed where gnx_core_train_fused_applies; src/gncore.jl:56-59, src/gnfeedforward.jl:27-31).
//
//   k_core_post_train<D, BF16> : y = fmaf(m, ffwd(gn2(x)), x + b) per row, b = block(gn1(x)) read as fp32 from the workspace.
//
// The body is core_post_lds_body's (gnx_core_post_kernel.h: a row per lane, the FeedForward's weights staged in LDS once per workgroup and read
// with uniform addresses — ds_read_b128 broadcasts — gn2 recomputed in the lane, the 4D hidden units produced and consumed in registers, two
// rows per lane sharing every weight read) with the mask as one more operand of the last operation.  The mask is gnx_dropout_mask's, bit for
// bit (gnx_philox.h): element i = row * D + k of the packed [R][rows][D] tensor takes component i % 4 of philox4(i / 4, entity, seed).  A
// row's D elements lie in at most (OMAX + D + 3) / 4 consecutive Philox blocks (OMAX: the largest i % 4 a row can start at — 0 where
// D % 4 == 0, 2 where D is even, else 3); each block is generated once per row, after the FeedForward, so that no mask register is live across
// the hidden loop.  A dropped element (m == 0) is x + b exactly: no second evaluation of the FeedForward is subtracted from the first, as the
// unfused correction of gnx_core_forward_train does.
// BF16: x and y are bfloat16 rows — widened exactly on load, rounded to nearest even once on store; b and everything between stay fp32.
// k_ln1_rows_bf16<D> is k_ln1_rows (gnx_core_narrow.hip) reading bf16 rows: gn1(x) in fp32 for the block, the same operations on the same
// values as the fp32 kernel on the widened rows.
#include "gnx_launchers.h"
#include "gnx_philox.h"
#include "gnx_wave_kernel.h"  // load_row / store_row / normalise / act_row / feat

namespace gnx {

struct CorePostTrain {
  const float* x;      // the caller's rows [rows][D], fp32 or bf16
  const float* b;      // block(gn1(x)) [rows][D], fp32
  float* y;            // [rows][D], fp32 or bf16
  size_t rows;         // R * rows of the entity
  const float *gamma2, *beta2;
  gnx_dense fc1, fc2;
  float eps; int eps_mode;
  float p, scale;      // drop probability, 1 / (1 - p) (0 at p = 1)
  uint64_t seed;
  uint32_t entity;
};

constexpr int core_post_train_rows(int) { return 2; }  // rows per lane: no instantiation spills at two (profiles/core_train_narrow_resources.json)

template <int D, bool BF16>
__global__ __launch_bounds__(256) void k_core_post_train(CorePostTrain a) {
  constexpr int M = core_post_train_rows(D);
  constexpr int H = 4 * D;
  constexpr int DP = (D + 3) / 4 * 4;  // padded row of W2 in LDS (16-B reads)
  constexpr int OMAX = D % 4 == 0 ? 0 : D % 2 == 0 ? 2 : 3;
  constexpr int NQ = (OMAX + D + 3) / 4;  // Philox blocks a row can touch
  const auto* __restrict__ x = feat<BF16>(a.x);
  auto* __restrict__ y = feat<BF16>(a.y);
  __shared__ __attribute__((aligned(16))) float s_w1[D * H];   // W1 (4D x D column-major): element (j, k) at k*H + j
  __shared__ __attribute__((aligned(16))) float s_w2[H * DP];  // W2 (D x 4D column-major): element (k, j) at j*D + k -> row j padded to DP
  __shared__ __attribute__((aligned(16))) float s_b1[H];
  __shared__ float s_v[3 * D];                                 // b2 | gamma2 | beta2
  for (int i = threadIdx.x; i < D * H; i += 256) s_w1[i] = a.fc1.weight[i];
  for (int i = threadIdx.x; i < H * DP; i += 256) { const int jrow = i / DP, k = i % DP; s_w2[i] = k < D ? a.fc2.weight[jrow * D + k] : 0.f; }
  for (int i = threadIdx.x; i < H; i += 256) s_b1[i] = a.fc1.bias ? a.fc1.bias[i] : 0.f;
  for (int i = threadIdx.x; i < D; i += 256) { s_v[i] = a.fc2.bias ? a.fc2.bias[i] : 0.f; s_v[D + i] = a.gamma2[i]; s_v[2 * D + i] = a.beta2[i]; }
  __syncthreads();

  const size_t stride = (size_t)gridDim.x * 256;
  const size_t row0 = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (row0 >= a.rows) return;
  float rs[M][D], z[M][D], acc[M][DP];
  size_t row[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const size_t rm = row0 + m * stride;
    row[m] = rm < a.rows ? rm : row0;  // clamped: a lane without an m-th row recomputes its first one (its store is skipped)
    float blk[D];
    load_row<D>(x + row[m] * D, z[m]);
    load_row<D>(a.b + row[m] * D, blk);
#pragma unroll
    for (int k = 0; k < D; ++k) rs[m][k] = z[m][k] + blk[k];  // the two residual terms (gncore.jl:56-59)
    normalise<D>(z[m], a.eps, a.eps_mode);
#pragma unroll
    for (int k = 0; k < D; ++k) z[m][k] = fmaf(s_v[D + k], z[m][k], s_v[2 * D + k]);
#pragma unroll
    for (int k = 0; k < DP; ++k) acc[m][k] = k < D ? s_v[k] : 0.f;
  }
  // four hidden units at a time, produced and consumed in registers
#pragma unroll 1
  for (int j0 = 0; j0 < H; j0 += 4) {
    float h[M][4];
    const float4 bb = *reinterpret_cast<const float4*>(s_b1 + j0);
#pragma unroll
    for (int m = 0; m < M; ++m) { h[m][0] = bb.x; h[m][1] = bb.y; h[m][2] = bb.z; h[m][3] = bb.w; }
#pragma unroll
    for (int k = 0; k < D; ++k) {
      if (k % 4 == 0) __builtin_amdgcn_sched_barrier(0);  // (else every weight read of the iteration is hoisted: see core_post_lds_body)
      const float4 w = *reinterpret_cast<const float4*>(s_w1 + k * H + j0);
#pragma unroll
      for (int m = 0; m < M; ++m) {
        h[m][0] = fmaf(w.x, z[m][k], h[m][0]); h[m][1] = fmaf(w.y, z[m][k], h[m][1]);
        h[m][2] = fmaf(w.z, z[m][k], h[m][2]); h[m][3] = fmaf(w.w, z[m][k], h[m][3]);
      }
    }
#pragma unroll
    for (int m = 0; m < M; ++m) act_row<4>(h[m], a.fc1.act);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < DP / 4; ++q) {
        const float4 w = *reinterpret_cast<const float4*>(s_w2 + (j0 + jj) * DP + 4 * q);
#pragma unroll
        for (int m = 0; m < M; ++m) {
          acc[m][4 * q] = fmaf(w.x, h[m][jj], acc[m][4 * q]); acc[m][4 * q + 1] = fmaf(w.y, h[m][jj], acc[m][4 * q + 1]);
          acc[m][4 * q + 2] = fmaf(w.z, h[m][jj], acc[m][4 * q + 2]); acc[m][4 * q + 3] = fmaf(w.w, h[m][jj], acc[m][4 * q + 3]);
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    if (m > 0 && row0 + m * stride >= a.rows) break;
    // the row's Philox blocks, each once: element k sits at position o + k of them
    const size_t i0 = row[m] * D;
    const uint64_t quad0 = i0 >> 2;
    const unsigned o = OMAX ? (unsigned)(i0 & 3) : 0u;
    uint32_t r[4 * NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      uint32_t c[4];
      philox4(quad0 + q, a.entity, a.seed, c);
#pragma unroll
      for (int j = 0; j < 4; ++j) r[4 * q + j] = c[j];
    }
    float out[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      uint32_t bits = r[k];  // (selects over constant positions: the register array is never indexed by a variable)
      if constexpr (OMAX >= 1 && OMAX != 2) { if (k + 1 < 4 * NQ) bits = o == 1 ? r[k + 1] : bits; }
      if constexpr (OMAX >= 2) { if (k + 2 < 4 * NQ) bits = o == 2 ? r[k + 2] : bits; }
      if constexpr (OMAX >= 3) { if (k + 3 < 4 * NQ) bits = o == 3 ? r[k + 3] : bits; }
      out[k] = fmaf(mask_of(bits, a.p, a.scale), acc[m][k], rs[m][k]);  // fc2 is the identity (the entry checks)
    }
    store_row<D>(y + row[m] * D, out);
  }
}

template <int D>
__global__ __launch_bounds__(256) void k_ln1_rows_bf16(const bf16_t* __restrict__ x, size_t rows, const float* gamma, const float* beta, float eps,
                                                       int eps_mode, float* __restrict__ y) {
  const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  const cfloatp g = as_const(gamma), b = as_const(beta);
  float v[D];
  load_row<D>(x + row * D, v);
  normalise<D>(v, eps, eps_mode);
#pragma unroll
  for (int k = 0; k < D; ++k) v[k] = fmaf(g[k], v[k], b[k]);
  store_row<D>(y + row * D, v);
}

#define GNX_CORE_WIDTHS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

int32_t launch_ln1_rows_bf16(const void* x, size_t rows, int d, const gnx_layernorm& l1, float eps, int eps_mode, float* y, hipStream_t s) {
  if (rows == 0) return GNX_OK;
  ProfScope ps("k_ln1_rows", s);
  const dim3 grid((unsigned)((rows + 255) / 256));
  const bf16_t* xb = static_cast<const bf16_t*>(x);
  switch (d) {
#define GNX_CASE(D) case D: GNX_LAUNCH((k_ln1_rows_bf16<D>), grid, dim3(256), 0, s, xb, rows, l1.gamma, l1.beta, eps, eps_mode, y); break;
    GNX_CORE_WIDTHS(GNX_CASE)
#undef GNX_CASE
    default: return fail(GNX_ERR_DIMS, "launch_ln1_rows_bf16: width not instantiated");
  }
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

int32_t launch_core_post_train(const void* x, size_t rows, int d, const gnx_layernorm& l2, const gnx_ffn& ff, float eps, int eps_mode, const float* block_out,
                               const gnx_dropout& dr, int entity, void* y, bool bf16, hipStream_t s) {
  if (rows == 0) return GNX_OK;
  ProfScope ps("k_core_post", s);
  const CorePostTrain a{static_cast<const float*>(x), block_out, static_cast<float*>(y), rows, l2.gamma, l2.beta, ff.fc1, ff.fc2, eps, eps_mode,
                        dr.p, dr.p < 1.f ? 1.f / (1.f - dr.p) : 0.f, dr.seed, (uint32_t)entity};
  switch (d) {
#define GNX_CASE(D)                                                                                   \
  case D: {                                                                                           \
    const size_t per = 256 * (size_t)core_post_train_rows(D);                                         \
    const dim3 grid((unsigned)((rows + per - 1) / per));                                              \
    if (bf16) GNX_LAUNCH((k_core_post_train<D, true>), grid, dim3(256), 0, s, a);                      \
    else GNX_LAUNCH((k_core_post_train<D, false>), grid, dim3(256), 0, s, a);                          \
    break;                                                                                            \
  }
    GNX_CORE_WIDTHS(GNX_CASE)
#undef GNX_CASE
    default: return fail(GNX_ERR_DIMS, "launch_core_post_train: width not instantiated");
  }
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
