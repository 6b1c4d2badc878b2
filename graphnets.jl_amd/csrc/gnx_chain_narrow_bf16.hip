// The fused Chain update-function kernel on bfloat16 feature rows (gnx_chain_block_forward_typed's native path, gnx_chain.cpp).
//
//   k_chain_mlp_bf16<WMAX, SRC> : k_chain_mlp (gnx_chain_narrow.hip) with bf16 feature inputs widened exactly on load, the layers run by
//                                 chain_layer_fw (gnx_chain_mlp.h: the forward's loop operation for operation, so the row carries k_chain_mlp's
//                                 bits), and the last layer's row stored twice: rounded to nearest even once as bf16 into the caller's buffer
//                                 and — where a later function of the same call reads it — unrounded as fp32 into a workspace carve (out32).
//
// SRC_EDGE  a0, a1, a2 = ef, nf, gf are bf16.
// SRC_NODE  a1, a2 = nf, gf are bf16; a0 is the fp32 ef' the edge launch of the same call left in the workspace: the sum over the in-edges
//           carries chain_input_row's bits.
// SRC_ROWS  a0 is the fp32 materialised input row, as in k_chain_mlp.
//
// A bf16 buffer is 4-byte aligned (the entry checks); rows of odd width and replicas of an odd rows * d start 2-byte aligned.  Every bf16
// access is one 16-bit load or store of an element of the tensor: nothing beyond 2-byte alignment is assumed and no byte outside a tensor is
// touched.  The loads are not paired: a lane issues as many loads as k_chain_mlp does (half the bytes each), and which half of a dword a row
// starts in varies by lane, so pairing would cost a funnel shift per pair on a kernel that waits on its gathers.
// The argument record is the forward's plus the two output pointers, in a record of its own: ChainMlpArgs keeps its size, and with it
// k_chain_mlp and k_chain_mlp_bw keep their registers (profiles/chain_narrow_resources.json, chain_bw_narrow_resources.json).
#include "gnx_chain_mlp.h"

namespace gnx {

struct ChainMlpBf16Args {
  ChainMlpArgs f;  // f.a0 .. f.a2: bf16 where the head of this file says so (declared float, like the feature pointers of BlockArgs); f.out unused
  bf16_t* out;     // [R][rows][ow] bf16
  float* out32;    // [R][rows][ow] fp32, or nullptr
};

// cur[at .. at + w) = widened p[0 .. w): one 16-bit load per element behind a uniform test
template <int WMAX>
__device__ __forceinline__ void chain_load_seg_bf16(const bf16_t* __restrict__ p, int at, int w, float (&cur)[WMAX]) {
#pragma unroll
  for (int k = 0; k < WMAX; ++k)
    if (k >= at && k < at + w) cur[k] = bf16_lo(p[k - at]);
}

// chain_input_row on bf16 features; entries at or beyond K exactly 0.f
template <int WMAX, int SRC>
__device__ __forceinline__ void chain_input_row_bf16(const ChainMlpArgs& a, size_t row, size_t r, float (&cur)[WMAX]) {
  if constexpr (SRC == SRC_ROWS) {
    chain_input_row<WMAX, SRC_ROWS>(a, row, r, cur);
    return;
  }
#pragma unroll
  for (int k = 0; k < WMAX; ++k) cur[k] = 0.f;
  const bf16_t* __restrict__ b0 = reinterpret_cast<const bf16_t*>(a.a0);
  const bf16_t* __restrict__ b1 = reinterpret_cast<const bf16_t*>(a.a1);
  const bf16_t* __restrict__ b2 = reinterpret_cast<const bf16_t*>(a.a2);
  if constexpr (SRC == SRC_EDGE) {
    const int e = (int)row;
    if (a.d0 > 0) chain_load_seg_bf16<WMAX>(b0 + (r * (size_t)a.E + e) * a.d0, 0, a.d0, cur);
    if (a.d1 > 0) {
      chain_load_seg_bf16<WMAX>(b1 + (r * (size_t)a.N + a.rowval[e]) * a.d1, a.d0, a.d1, cur);
      chain_load_seg_bf16<WMAX>(b1 + (r * (size_t)a.N + a.edge_dst[e]) * a.d1, a.d0 + a.d1, a.d1, cur);
    }
    if (a.d2 > 0) chain_load_seg_bf16<WMAX>(b2 + (r * (size_t)a.G + segment_of(a.seg_off, a.G, e)) * a.d2, a.d0 + 2 * a.d1, a.d2, cur);
  } else {
    const int n = (int)row;
    if (a.d0 > 0) {  // the fp32 ef' of this call: chain_input_row's sequential adds in CSC order
      const int e1 = a.colptr[n + 1];
      for (int e = a.colptr[n]; e < e1; ++e) {
        const float* __restrict__ p = a.a0 + (r * (size_t)a.E + e) * a.d0;
#pragma unroll
        for (int k = 0; k < WMAX; ++k)
          if (k < a.d0) cur[k] += p[k];
      }
    }
    if (a.d1 > 0) chain_load_seg_bf16<WMAX>(b1 + (r * (size_t)a.N + n) * a.d1, a.d0, a.d1, cur);
    if (a.d2 > 0) chain_load_seg_bf16<WMAX>(b2 + (r * (size_t)a.G + segment_of(a.seg_off, a.G, n)) * a.d2, a.d0 + a.d1, a.d2, cur);
  }
}

template <int WMAX, int SRC>
__global__ __launch_bounds__(256) void k_chain_mlp_bf16(ChainMlpBf16Args t) {
  extern __shared__ __attribute__((aligned(16))) float s_par[];
  const ChainMlpArgs& a = t.f;
  chain_stage_params(a, s_par, 256);
  __syncthreads();
  const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= a.rows) return;
  const size_t r = blockIdx.y;

  float cur[WMAX];
  chain_input_row_bf16<WMAX, SRC>(a, row, r, cur);

  int off = 0, kin = a.K;
#pragma unroll 1
  for (int l = 0; l < a.n_layers; ++l) {
    off = chain_layer_fw<WMAX>(s_par, off, kin, a.layer[l].width, a.layer[l].op, cur);
    kin = a.layer[l].width;
  }

  const size_t at = (r * a.rows + row) * (size_t)a.ow;
  bf16_t* __restrict__ o = t.out + at;
#pragma unroll
  for (int k = 0; k < WMAX; ++k)
    if (k < a.ow) o[k] = to_bf16(cur[k]);
  if (t.out32) {
    float* __restrict__ o32 = t.out32 + at;
#pragma unroll
    for (int k = 0; k < WMAX; ++k)
      if (k < a.ow) o32[k] = cur[k];
  }
}

// launch_chain_narrow on bf16 features (which of in0 .. in2 are bf16: the head of this file); out: bf16 rows, out32: the same rows in fp32 or
// nullptr.  The caller asked chain_narrow_takes.
int32_t launch_chain_narrow_bf16(const gnx_graphs* h, int entity, const gnx_chain& c, const void* in0, int d0, const void* in1, int d1, const void* in2, int d2,
                                 void* out, float* out32, int64_t R, hipStream_t s, const char* name) {
  ChainMlpBf16Args t{};
  int wmax;
  size_t rows;
  if (int32_t rc = chain_mlp_prologue(h, entity, c, static_cast<const float*>(in0), d0, static_cast<const float*>(in1), d1, static_cast<const float*>(in2), d2,
                                      CHAIN_RULE_FW, "launch_chain_narrow_bf16", s, t.f, &wmax, &rows)) return rc;
  t.f.ow = c.widths[c.n_layers - 1];
  t.out = static_cast<bf16_t*>(out); t.out32 = out32;
  const dim3 grid((unsigned)((rows + 255) / 256), (unsigned)R);
  const size_t lds = sizeof(float) * chain_narrow_lds_floats(c, t.f.K);
  ProfScope ps(name, s);
  chain_mlp_dispatch(wmax, entity, [&](auto W, auto S) { GNX_LAUNCH((k_chain_mlp_bf16<decltype(W)::value, decltype(S)::value>), grid, dim3(256), lds, s, t); });
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
