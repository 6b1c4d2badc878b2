// GNBlock with Chain update functions at matrix-core widths: one update function = one kernel (gnx_chain_block_forward_wide, gnx_chain.cpp).
//
//   k_chain_wide<NB, SRC> : the text of gnx_chain_wide_kernel.h on fp32 features — a workgroup of 2-4 waves, a wave OWNS 32 rows of the entity
//                           through all layers of the function, its rows in a wave-private LDS slice, the weights staged per workgroup as three
//                           bf16 planes, six-term products on the matrix cores.  Memory sees the function's input once and its output once.
//
// SRC_EDGE  the lanes gather [ef[e] ; nf[rowval[e]] ; nf[edge_dst[e]] ; gf[graph(e)]] straight into the slice (getedgefninput, gnblock.jl:65; the
//           indices of k_chain_mlp's edge form) — a LayerNorm as the first layer then normalises the gathered row like any other
// SRC_ROWS  a materialised [rows][K] buffer (launch_fn_input: the node and the graph function)
// Feature, parameter and output pointers may be 4-byte aligned only: every global access is one dword.  Offsets are size_t.
#define GNX_CHAIN_WIDE_BF16 0
#include "gnx_chain_wide_kernel.h"  // k_chain_wide<NB, SRC>

namespace gnx {

// One update function of a Chain block in one launch.  entity 0: in0 / in1 / in2 = ef, nf, gf of widths d0, d1, d2 (SRC_EDGE); 1, 2: in0 = the
// materialised [R rows][d0] input rows (SRC_ROWS; d1 = d2 = 0).  The caller asked chain_wide_takes (gnx_chain_plan.h).
int32_t launch_chain_wide(const gnx_graphs* h, int entity, const gnx_chain& c, const float* in0, int d0, const float* in1, int d1, const float* in2, int d2,
                          float* out, int64_t R, hipStream_t s, const char* name) {
  ChainWideArgs a{};
  ChainWideShape sh;
  if (int32_t rc = chain_wide_args(h, entity, c, in0, d0, in1, d1, in2, d2, s, "launch_chain_wide", a, sh)) return rc;
  a.out = out;
  const dim3 grid((unsigned)sh.nwg, (unsigned)R), block(64u * sh.waves);
  const size_t lds = sizeof(float) * (size_t)sh.floats;
  ProfScope ps(name, s);
  auto go = [&](auto nb) {
    constexpr int NB = decltype(nb)::value;
    if (entity == 0) GNX_LAUNCH((k_chain_wide<NB, SRC_EDGE>), grid, block, lds, s, a);
    else GNX_LAUNCH((k_chain_wide<NB, SRC_ROWS>), grid, block, lds, s, a);
  };
  sh.nb == 1 ? go(ChainInt<1>{}) : go(ChainInt<2>{});  // (chain_wide_cut: no function with more blocks is inside the rule)
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
