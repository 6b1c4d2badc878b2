// The wave form of the Chain pullback on bfloat16 features (gnx_chain_block_backward_wave_typed, gnx_backward.hip; the rule:
// chain_bw_wave_takes with bf16, gnx_chain_plan.h).
//
//   k_chain_wave_partials_bf16<W> : k_chain_wave_partials with ef, nf and gf read as bf16; the partial rows are fp32 and carry the fp32 kernel's bits.
//   k_chain_wave_bw_bf16<W>       : k_chain_wave_bw — one wavefront per wave tile, both functions' parameters staged once per workgroup, per
//                                   wave a tape of 64 rows at odd ld, P_e + P_n accumulators and a slice [cap][oe | 1], the phases (a) - (d)
//                                   (gnx_chain_bw_wave.hip) — with ef, nf[src], nf[dst], nf[n], gf[g], g_ef_out and g_nf_out read as bf16 and
//                                   d_ef stored as bf16.
// Both are one text with their fp32 twins (gnx_chain_bw_wave_kernel.h), compiled here with BF16 = true and with the options of
// gnx_chain_bw_wave.hip: the element type changes loads and stores only, so the slice, the tape, the accumulators, dXg, the compact dXn and dXe
// and the partial rows are fp32 and hold, bit for bit, what the fp32 kernels hold on the widened tensors.  A bf16 element is read by one 16-bit
// load and widened by a shift; d_ef is rounded to nearest even once and stored by one 16-bit store from the lane that holds the row.  Rows of
// odd width and replicas of an odd rows * d start 2-byte aligned: nothing beyond that is assumed, no byte outside a tensor is touched.
// The graph level of the call runs on fp32 rows: k_chain_graph_rows_wave (gnx_chain_bw_wave.hip) assembles Xg from the partial rows and the
// widened gf, k_chain_mlp_bw_bf16<., SRC_ROWS> reads g_gf_out as bf16.
// No instantiation uses scratch; registers and LDS next to the fp32 twins': profiles/chain_bw_wave_bf16_resources.json.
#define GNX_CHAIN_BW_WAVE_NAME(x) x##_bf16  // k_chain_wave_partials_bf16, k_chain_wave_bw_bf16, launch_chain_wave_partials_bf16, launch_chain_wave_bw_bf16
#define GNX_CHAIN_BW_WAVE_BF16 true
#include "gnx_chain_bw_wave_kernel.h"
