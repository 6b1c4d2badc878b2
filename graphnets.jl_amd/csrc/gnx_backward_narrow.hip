// The edge level of the GNBlock backward at narrow widths, in one kernel (gnx_block_backward_fused): the ahead-of-time instantiations of
// k_bw_edge_wave / k_bw_edge_wave_bf16 (gnx_bw_edge_wave_kernel.h, where the kernel is described) and their launcher.  Any other eligible
// width set gets the same kernel at run time (gnx_jit.cpp: jit_get_bw_edge; gnx_block_backward_narrow).
#include "gnx_launchers.h"
#include "gnx_bw_edge_wave_kernel.h"

namespace gnx {

// the ahead-of-time narrow width sets whose edge level the generic path runs (J * K < 64): (de, dn, dg, oe)
#define GNX_BW_EDGE_WAVE_DIMS(X) X(10, 5, 0, 3) X(3, 4, 5, 3) X(0, 2, 0, 2) X(2, 2, 2, 2) X(4, 3, 2, 3)

bool bw_edge_wave_has(int de, int dn, int dg, int oe) {
#define GNX_X(DE, DN, DG, OE) if (de == DE && dn == DN && dg == DG && oe == OE) return true;
  GNX_BW_EDGE_WAVE_DIMS(GNX_X)
#undef GNX_X
  return false;
}

size_t bw_edge_wave_rows(const gnx_graphs* h) { return (size_t)((h->n_wtiles() + 3) / 4); }

int32_t launch_bw_edge_wave(const gnx_block_params* p, const BwEdgeWave& a, int64_t R, hipStream_t s, bool bf16) {
  if (a.n_wtiles <= 0 || a.E <= 0) return GNX_OK;
  const dim3 grid((unsigned)((a.n_wtiles + 3) / 4), (unsigned)R);
#define GNX_X(DE, DN, DG, OE)                                                        \
  if (p->de == DE && p->dn == DN && p->dg == DG && p->oe == OE) {                    \
    if (bf16) GNX_LAUNCH((k_bw_edge_wave_bf16<DE, DN, DG, OE>), grid, dim3(256), 0, s, a); \
    else GNX_LAUNCH((k_bw_edge_wave<DE, DN, DG, OE>), grid, dim3(256), 0, s, a);     \
    GNX_HIP(hipGetLastError());                                                      \
    return GNX_OK;                                                                   \
  }
  GNX_BW_EDGE_WAVE_DIMS(GNX_X)
#undef GNX_X
  return fail(GNX_ERR_DIMS, "fused edge pullback: width set not instantiated");
}

// the same launch with the kernel specialised at run time for the call's width set and element type (gnx_jit.cpp: jit_get_bw_edge)
int32_t launch_bw_edge_wave_jit(hipFunction_t fn, const BwEdgeWave& a, int64_t R, hipStream_t s) {
  if (a.n_wtiles <= 0 || a.E <= 0) return GNX_OK;
  BwEdgeWave aa = a;
  void* params[] = {&aa};
  GNX_HIP(module_launch(fn, (unsigned)((a.n_wtiles + 3) / 4), (unsigned)R, 1, 256, 1, 1, lds_pad_bytes(), s, params));
  return GNX_OK;
}

}  // namespace gnx
