// The pullback of one Chain update function at narrow widths on bfloat16 features, in one kernel (gnx_chain_block_backward_narrow_typed's
// native path, gnx_backward.hip).
//
//   k_chain_mlp_bw_bf16<WMAX, SRC> : k_chain_mlp_bw (gnx_chain_bw_narrow.hip) with bf16 feature-shaped operands.  Both kernels are
//                                    one text (gnx_chain_bw_kernel.h); this file compiles it with BF16 = true, which changes loads
//                                    and stores only: the tape, the accumulators, the parameter-gradient phase, the LDS plan
//                                    (chain_bw_narrow_shape) and the launch geometry are the fp32 kernel's, and so is every arithmetic operation.
//
// SRC_EDGE  ef, nf, gf, the upstream gradient g_ef_out and `direct` (d_ef) are bf16.
// SRC_NODE  nf, gf and the upstream gradient g_nf_out are bf16; a0 is the fp32 ef' of this call, summed in CSC order.
// SRC_ROWS  the upstream gradient g_gf_out is bf16; a0 is the fp32 Xg rows.
// ex1 / ex2 (dXg, dXn), dx (dXe_c, dXn, dXg) and the partial rows stay fp32.
//
// A bf16 element read is widened exactly; d_ef is rounded to nearest even once per element.  A bf16 buffer is 4-byte aligned (the entry checks);
// rows of odd width and replicas of an odd rows * d start 2-byte aligned, and nothing more is assumed: every bf16 access is one 16-bit load or
// store of an element of the tensor — no dword is read, modified and written back, no byte outside a tensor is touched.
// The argument record is the fp32 kernel's (ChainMlpBwArgs), the bf16 pointers declared float as in ChainMlpArgs.  No instantiation uses
// scratch (profiles/chain_bw_narrow_bf16_resources.json).
#define GNX_CHAIN_BW_KERNEL k_chain_mlp_bw_bf16  // template <int WMAX, int SRC> __global__ void k_chain_mlp_bw_bf16(ChainMlpBwArgs)
#define GNX_CHAIN_BW_BF16 true
#include "gnx_chain_bw_kernel.h"

namespace gnx {

// launch_chain_bw_narrow on bf16 features (which of in0 .. in2, io.G and io.direct are bf16: the head of this file).  The caller asked
// chain_bw_narrow_takes and opens the ProfScope.
int32_t launch_chain_bw_narrow_bf16(const gnx_graphs* h, int entity, const gnx_chain& c, const void* in0, int d0, const void* in1, int d1, const void* in2, int d2,
                                    const ChainBwNarrowIo& io, int64_t R, hipStream_t s) {
  ChainMlpBwArgs a{};
  int wmax;
  size_t lds;
  if (int32_t rc = chain_bw_narrow_args(h, entity, c, static_cast<const float*>(in0), d0, static_cast<const float*>(in1), d1, static_cast<const float*>(in2), d2, io,
                                        "launch_chain_bw_narrow_bf16", s, a, &wmax, &lds)) return rc;
  const dim3 grid((unsigned)a.sh.nwg, (unsigned)R), block(64 * a.sh.waves);
  chain_mlp_dispatch(wmax, entity, [&](auto W, auto S) { GNX_LAUNCH((k_chain_mlp_bw_bf16<decltype(W)::value, decltype(S)::value>), grid, block, lds, s, a); });
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
