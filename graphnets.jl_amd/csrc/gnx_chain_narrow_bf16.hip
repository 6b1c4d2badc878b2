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
  bf16_t* out;     // [R][rows][ow] bf16, or nullptr
  float* out32;    // [R][rows][ow] fp32, or nullptr
};

// (chain_input_row_bf16, the gather of a bf16 input row: gnx_chain_mlp.h — the pullback kernel of gnx_chain_bw_narrow_bf16.hip builds its row with it too)

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
  if (t.out) {  // (uniform; the pullback's recompute wants the fp32 rows alone)
    bf16_t* __restrict__ o = t.out + at;
#pragma unroll
    for (int k = 0; k < WMAX; ++k)
      if (k < a.ow) o[k] = to_bf16(cur[k]);
  }
  if (t.out32) {
    float* __restrict__ o32 = t.out32 + at;
#pragma unroll
    for (int k = 0; k < WMAX; ++k)
      if (k < a.ow) o32[k] = cur[k];
  }
}

// launch_chain_narrow on bf16 features (which of in0 .. in2 are bf16: the head of this file); out: bf16 rows or nullptr, out32: the same rows in
// fp32 or nullptr.  The caller asked chain_narrow_takes.
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
