// The fused narrow kernels with bfloat16 feature rows (k_block_wave<..., BF16 = true>, its chained form k_block_wave<..., CHAIN, BF16>,
// k_graph_t<C, ONEG, true>, the run form k_block_wave_run / k_graph_run of several steps in one launch) for the bf16 rows of the table in
// gnx_narrow_sets.h; gnx_narrow.hip asks the table, then routes gnx_block_forward_typed and the bf16 steps of gnx_block_forward_steps_typed
// here, every other narrow width set is specialised at run time (gnx_jit.cpp).  Also the block of a bf16 GNCore at README ex.3's widths
// (k_block_wave<..., LN, ..., BF16>, k_block_wave_ffe<..., BF16>: bf16 rows in, fp32 intermediates out).  Launchers only — the shared ones of
// gnx_narrow_launch.h with BF16 = true, each 1 where the table has no such kernel — and no predicate.
// A translation unit of its own because build.py compiles it without the SLP vectoriser (-fno-slp-vectorize; gnx_jit.cpp passes the same
// option for a bf16 key): with it, every widened value feeds a v_pk_fma_f32 as the low half of a register pair of its own, and the README
// ex.1 kernel needs 70 instead of 58 VGPRs — 7 instead of 8 waves per SIMD.  Scalar FMAs compute the same bits.
#include "gnx_launchers.h"
#include "gnx_narrow_launch.h"
#include "gnx_wave_kernel.h"

namespace gnx {

int32_t launch_fused_bf16(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, int phase) { return launch_narrow_plain<true>(h, a, R, s, phase); }
int32_t launch_chained_bf16(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s) { return launch_narrow_chained<true>(h, a, R, s); }
int32_t launch_ln_bf16(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, int phase) { return launch_narrow_ln<true>(h, a, R, s, phase); }
int32_t launch_run_bf16(const gnx_graphs* h, const BlockArgs& a, const RunTable& t, int Z, hipStream_t s) { return launch_narrow_run<true>(h, a, t, Z, s, 3); }  // (always both launches)

}  // namespace gnx
