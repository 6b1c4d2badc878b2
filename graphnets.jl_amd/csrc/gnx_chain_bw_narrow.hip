// The pullback of one Chain update function at narrow widths in one kernel (gnx_chain_block_backward_narrow, gnx_backward.hip).
//
//   k_chain_mlp_bw<WMAX, SRC> : (its text: gnx_chain_bw_kernel.h, included below — shared with the bf16 kernel of gnx_chain_bw_narrow_bf16.hip)
//   one lane = one row of the entity.  The lane builds the function's input row (chain_input_row: the forward kernel's
//   code), runs it forward through all layers (chain_layer_fw: the forward kernel's operation order) and walks back through them in registers.
//
// What the way back needs lives on a per-lane tape in LDS: the input row and the output of every layer but the last, `ld` floats per lane, ld odd,
// lane l at [l * ld, (l + 1) * ld) — a lane's accesses to its own row fall on 64 different banks.  A gelu layer's pre-activation and a LayerNorm's
// mean and deviation are recomputed from the layer's input on the tape (the forward's operations again, so the same bits); nothing else is kept.
//   last-layer delta   (G + ex1[graph] + ex2[dst]) * act'          k_bw_delta's sum order and derivative formulas (act_grad_bw)
//   Dense              g_in[k] = sum_j W[k][j] delta[j], j ascending (k_bw_dx's order), then delta <- g_in .* act'(previous layer)
//   LayerNorm          k_ln_backward's formula for one norm, the row's sums taken by the lane in element order
// The input gradient of the row is stored (graph / node: the whole row into dXg / dXn; edge: the ef columns into d_ef, the node / graph columns
// into the compact [R E][2 dn + dg] tensor that k_bw_dnf and the d_gf column sums read); hidden rows and deltas never reach memory.
//
// Parameter gradients, as in k_core_bw_narrow (no atomics, a fixed order): for every layer on the way back the wave parks its 64 deltas behind
// the tape, and lane l owns the pairs (k, j = l % J) for k = l / J + (64 / J) q — k == K is the bias, whose input is 1.  A wave takes one chunk
// of 64 rows and sums it in row order into its LDS slice (a loop over chunks would keep every width test of the body alive in scalar registers
// across it: more than the register file has); a workgroup — two to four waves under the rule, as many as fit 64 KB of LDS — adds its waves in
// wave order and writes one partial row per layer in k_bw_dw_final's pair order (p = k * J + j; a LayerNorm as J = width, K = 1: gamma then beta), which
// k_bw_dw_final finishes over the workgroups.  Every accumulator starts at 0: the results do not depend on what the workspace held.
// Every global access is one dword (4-byte aligned buffers are enough); offsets are size_t.  No instantiation uses scratch
// (profiles/chain_bw_narrow_resources.json): register arrays are indexed by unrolled constants only.
#include <algorithm>

#define GNX_CHAIN_BW_KERNEL k_chain_mlp_bw  // template <int WMAX, int SRC> __global__ void k_chain_mlp_bw(ChainMlpBwArgs)
#define GNX_CHAIN_BW_BF16 false
#include "gnx_chain_bw_kernel.h"

namespace gnx {

// The caller asked chain_bw_narrow_takes (gnx_chain_plan.h: the rule and the LDS plan, chain_bw_narrow_shape) and opens the ProfScope.
int32_t launch_chain_bw_narrow(const gnx_graphs* h, int entity, const gnx_chain& c, const float* in0, int d0, const float* in1, int d1, const float* in2, int d2,
                               const ChainBwNarrowIo& io, int64_t R, hipStream_t s) {
  if (chain_has_dropout(c)) return launch_chain_bw_narrow_train(h, entity, c, in0, d0, in1, d1, in2, d2, io, R, s);  // (a training call: gnx_chain_bw_train_narrow.hip)
  ChainMlpBwArgs a{};
  int wmax;
  size_t lds;
  if (int32_t rc = chain_bw_narrow_args(h, entity, c, in0, d0, in1, d1, in2, d2, io, "launch_chain_bw_narrow", s, a, &wmax, &lds)) return rc;
  const dim3 grid((unsigned)a.sh.nwg, (unsigned)R), block(64 * a.sh.waves);
  chain_mlp_dispatch(wmax, entity, [&](auto W, auto S) { GNX_LAUNCH((k_chain_mlp_bw<decltype(W)::value, decltype(S)::value>), grid, block, lds, s, a); });
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
