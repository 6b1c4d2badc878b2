// The FeedForward pullback of the GNCore backward at narrow widths (D <= 16), in one kernel (gnx_core_backward_narrow).
//
// The generic step 2 of core_backward_impl (gnx_backward.hip) recomputes the hidden layer h = act(W1 z + b1) into memory, forms dh = g W2^T and
// delta1 = dh .* act'(h) in memory, and reads all of them again for the two weight gradients and for dz2 = delta1 W1^T.  Here a row is one lane:
// z, g, h, delta1 and dz2 of the row live in registers, the weights are uniform (scalar) loads, and only dz2 is stored.  The kernel takes the
// flattened R * rows of one entity — there is no graph structure in a FeedForward — and a wave walks its own contiguous row range 64 rows at
// a time with clamped, unconditional loads and guarded stores.
//
// Per row the operations are those of k_fw_dense, k_bw_dx (fc2), k_bw_delta<0> and k_bw_dx (fc1) in their order, so dz2 carries the bits of
// the generic kernels.  The weight and bias gradients are summed in another (fixed) order: a wave parks the chunk's rows in its own LDS slice,
// one phase per Dense — [z ; 1 ; delta1] for fc1, then [h ; 1 ; g] for fc2, the 1 being the bias's input — and lane l owns the pairs
// (k, j = l % J) for k = l / J + (64 / J) q: it reads its delta column once per row and the inputs of its slots at addresses that
// 64 / J lanes share (broadcast).  One accumulator per slot lives across the wave's chunks: rows in row order, chunks in chunk order; a
// workgroup adds its waves in wave order and writes one partial row per Dense in the pair order of k_bw_dw_partial (p = k * J + j, k == K the
// bias), which k_bw_dw_final finishes over the workgroups.  No atomics.
#include <algorithm>

#include "gnx_launchers.h"
#include "gnx_wave_kernel.h"  // cfloatp / as_const

namespace gnx {

struct CoreBwNarrow {
  const float* z;    // gn2(x) rows [rows][D]
  const float* g;    // upstream gradient of the FeedForward branch [rows][D]
  const float *W1, *b1, *W2;  // fc1 (4D x D column-major: element (j, k) at k*4D + j), its bias or nullptr, fc2 (D x 4D: (j, k') at k'*D + j)
  float* dz2;        // [rows][D]
  float* part1;      // [workgroups][4D (D + 1)] or nullptr (neither dW1 nor db1 wanted)
  float* part2;      // [workgroups][D (4D + 1)] or nullptr
  size_t rows;
  size_t rows_per_wave;  // a multiple of 64
  int act;           // fc1's activation: identity or relu
};

constexpr int CORE_BW_MAX_WG = 2048;  // partial rows per Dense at most
// waves of a workgroup: four while their LDS slices fit 64 KB
constexpr int core_bw_ld(int D) { return (5 * D + 1) | 1; }  // odd row length: the lanes' row writes fall on different banks
constexpr int core_bw_waves(int D) { return 4 * 64 * core_bw_ld(D) * 4 <= 65536 ? 4 : 2; }

// the weight-gradient phase of one Dense over the chunk parked in `rows`: inputs at columns [0, K] (column K holds 1), deltas at [K + 1, K + 1 + J)
template <int J, int K, int LD, int S>
__device__ __forceinline__ void core_bw_dw_phase(const float* rows, int cnt, int j, int kg, float (&acc)[S]) {
  constexpr int NG = 64 / J;
  int kk[S];
#pragma unroll
  for (int q = 0; q < S; ++q) kk[q] = min(kg + NG * q, K);  // clamped: slots past the bias are summed and never written
#pragma unroll 4
  for (int i = 0; i < cnt; ++i) {
    const float dv = rows[i * LD + K + 1 + j];
#pragma unroll
    for (int q = 0; q < S; ++q) acc[q] = fmaf(dv, rows[i * LD + kk[q]], acc[q]);
  }
}

// a workgroup's partial row of one Dense: every wave lays its accumulators out in its own slice, the waves are added in wave order
template <int J, int K, int LD, int S, int WAVES>
__device__ __forceinline__ void core_bw_dw_write(float* slices, int wave, int lane, int j, int kg, const float (&acc)[S], float* out) {
  constexpr int NG = 64 / J, P = J * (K + 1);
  static_assert(P <= 64 * LD, "a wave's slice holds its partial row");
  __syncthreads();  // (every wave is done with the rows it parked)
  float* mine = slices + wave * 64 * LD;
  if (kg < NG) {
#pragma unroll
    for (int q = 0; q < S; ++q)
      if (kg + NG * q <= K) mine[(kg + NG * q) * J + j] = acc[q];
  }
  __syncthreads();
  for (int p = threadIdx.x; p < P; p += 64 * WAVES) {
    float v = slices[p];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) v += slices[w * 64 * LD + p];
    out[p] = v;
  }
}

template <int D>
__global__ __launch_bounds__(64 * core_bw_waves(D)) void k_core_bw_narrow(CoreBwNarrow a) {
  constexpr int H = 4 * D, LD = core_bw_ld(D), WAVES = core_bw_waves(D);
  constexpr int NG1 = 64 / H, S1 = (D + 1 + NG1 - 1) / NG1;  // fc1: J = H, K = D
  constexpr int NG2 = 64 / D, S2 = (H + 1 + NG2 - 1) / NG2;  // fc2: J = D, K = H
  __shared__ float s_rows[WAVES * 64 * LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const cfloatp W1 = as_const(a.W1), W2 = as_const(a.W2), b1 = as_const(a.b1);
  const bool has_b1 = a.b1 != nullptr, relu = a.act == GNX_ACT_RELU;
  float* const rows = s_rows + wave * 64 * LD;
  const int j1 = lane % H, kg1 = lane / H, j2 = lane % D, kg2 = lane / D;
  float acc1[S1], acc2[S2];
#pragma unroll
  for (int q = 0; q < S1; ++q) acc1[q] = 0.f;
#pragma unroll
  for (int q = 0; q < S2; ++q) acc2[q] = 0.f;
  const size_t w = (size_t)blockIdx.x * WAVES + wave;
  const size_t r0 = w * a.rows_per_wave;
  const size_t r1 = r0 + a.rows_per_wave < a.rows ? r0 + a.rows_per_wave : a.rows;
  for (size_t c0 = r0; c0 < r1; c0 += 64) {  // wave-uniform
    const int cnt = (int)(r1 - c0 < 64 ? r1 - c0 : 64);
    const bool live = lane < cnt;
    const size_t row = c0 + (live ? lane : cnt - 1);  // clamped: unconditional loads, guarded stores
    float z[D], g[D], h[H], dz[D];
#pragma unroll
    for (int k = 0; k < D; ++k) { z[k] = a.z[row * D + k]; g[k] = a.g[row * D + k]; dz[k] = 0.f; }
    // k_fw_dense: h[j] = act(b1[j] + sum_k W1[k*H + j] z[k]), k ascending
#pragma unroll
    for (int j = 0; j < H; ++j) h[j] = has_b1 ? b1[j] : 0.f;
#pragma unroll
    for (int k = 0; k < D; ++k) {
#pragma unroll
      for (int j = 0; j < H; ++j) h[j] = fmaf(W1[k * H + j], z[k], h[j]);
    }
#pragma unroll
    for (int j = 0; j < H; ++j) h[j] = relu ? relu_f(h[j]) : h[j];  // act_apply, identity or relu
    if (a.part1) {  // uniform
#pragma unroll
      for (int k = 0; k < D; ++k) rows[lane * LD + k] = z[k];
      rows[lane * LD + D] = 1.f;
    }
    // four hidden units at a time: dh (k_bw_dx on fc2), delta1 (k_bw_delta<0>), then their terms of dz2 (k_bw_dx on fc1: j ascending)
#pragma unroll
    for (int j0 = 0; j0 < H; j0 += 4) {
      float d1[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float dh = 0.f;
#pragma unroll
        for (int jj = 0; jj < D; ++jj) dh = fmaf(W2[(j0 + u) * D + jj], g[jj], dh);
        d1[u] = dh * (relu ? (h[j0 + u] > 0.f ? 1.f : 0.f) : 1.f);  // act_grad_from_out
      }
#pragma unroll
      for (int k = 0; k < D; ++k) {
#pragma unroll
        for (int u = 0; u < 4; ++u) dz[k] = fmaf(W1[k * H + j0 + u], d1[u], dz[k]);
      }
      if (a.part1) {
#pragma unroll
        for (int u = 0; u < 4; ++u) rows[lane * LD + D + 1 + j0 + u] = d1[u];
      }
    }
    if (live) {
#pragma unroll
      for (int k = 0; k < D; ++k) a.dz2[row * D + k] = dz[k];
    }
    if (a.part1) {
      __builtin_amdgcn_wave_barrier();
      core_bw_dw_phase<H, D, LD, S1>(rows, cnt, j1, kg1, acc1);
      __builtin_amdgcn_wave_barrier();  // the next phase's rows overwrite these
    }
    if (a.part2) {
#pragma unroll
      for (int j = 0; j < H; ++j) rows[lane * LD + j] = h[j];
      rows[lane * LD + H] = 1.f;
#pragma unroll
      for (int k = 0; k < D; ++k) rows[lane * LD + H + 1 + k] = g[k];
      __builtin_amdgcn_wave_barrier();
      core_bw_dw_phase<D, H, LD, S2>(rows, cnt, j2, kg2, acc2);
      __builtin_amdgcn_wave_barrier();
    }
  }
  if (a.part1) core_bw_dw_write<H, D, LD, S1, WAVES>(s_rows, wave, lane, j1, kg1, acc1, a.part1 + (size_t)blockIdx.x * (H * (D + 1)));
  if (a.part2) core_bw_dw_write<D, H, LD, S2, WAVES>(s_rows, wave, lane, j2, kg2, acc2, a.part2 + (size_t)blockIdx.x * (D * (H + 1)));
}

#define GNX_CORE_BW_WIDTHS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

static int core_bw_narrow_waves(int d) {
  switch (d) {
#define GNX_CASE(D) case D: return core_bw_waves(D);
    GNX_CORE_BW_WIDTHS(GNX_CASE)
#undef GNX_CASE
    default: return 4;
  }
}

// chunks of 64 rows per wave, so that at most CORE_BW_MAX_WG workgroups cover the rows
static size_t core_bw_chunks_per_wave(size_t rows, int d) {
  const size_t nch = (rows + 63) / 64, slots = (size_t)CORE_BW_MAX_WG * core_bw_narrow_waves(d);
  return std::max<size_t>((nch + slots - 1) / slots, 1);
}

size_t core_bw_narrow_rows(size_t rows, int d) {
  if (rows == 0) return 0;
  const size_t per_wg = core_bw_chunks_per_wave(rows, d) * 64 * core_bw_narrow_waves(d);
  return (rows + per_wg - 1) / per_wg;
}

int32_t launch_core_bw_narrow(const float* z, const float* g, const gnx_ffn& ff, size_t rows, int d, float* dz2, float* part1, float* part2, hipStream_t s) {
  if (rows == 0) return GNX_OK;
  const CoreBwNarrow a{z, g, ff.fc1.weight, ff.fc1.bias, ff.fc2.weight, dz2, part1, part2, rows, core_bw_chunks_per_wave(rows, d) * 64, ff.fc1.act};
  const dim3 grid((unsigned)core_bw_narrow_rows(rows, d));
  switch (d) {
#define GNX_CASE(D) case D: GNX_LAUNCH((k_core_bw_narrow<D>), grid, dim3(64 * core_bw_waves(D)), 0, s, a); break;
    GNX_CORE_BW_WIDTHS(GNX_CASE)
#undef GNX_CASE
    default: return fail(GNX_ERR_DIMS, "launch_core_bw_narrow: width not instantiated");
  }
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
