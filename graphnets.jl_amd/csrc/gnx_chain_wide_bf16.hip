// The Chain forward at matrix-core widths on bfloat16 feature rows (gnx_chain_block_forward_wide_typed's native form, gnx_chain.cpp; the rule:
// chain_wide_typed_native, gnx_chain_plan.h).
//
//   k_chain_wide_bf16<NB, SRC> : the text of gnx_chain_wide_kernel.h with BF = true — k_chain_wide's work split (2-4 waves per workgroup, 32 rows
//                                per wave through all layers), its LDS plan (ChainWideShape, unchanged) and its weight staging, with another way
//                                for the data in and out:
//     SRC_EDGE  ef, nf and gf are bf16.  The lanes gather the row with packed dword loads where a pair of elements is aligned and 16-bit loads at
//               a segment's odd ends; the row is kept in LDS as bf16, aliased over the wave's fp32 slice at a stride of its own
//               (chain_wide_bf16_stride), and the first Dense runs three products per 16 reduction steps instead of six: the row is its own
//               high plane.  A function that opens with a LayerNorm widens the row into the fp32 slice instead.
//     SRC_ROWS  the materialised fp32 input rows, as k_chain_wide (the node and the graph function).
//     output    the wave's rows as one run of bf16 elements, each rounded once, dwords with 16-bit odd ends; and — where a later function of
//               the same call reads them — the same rows unrounded as fp32 into a workspace carve (out32).
//   k_chain_node_rows_bf16     : the node function's input rows [sum_{e->n} ef' ; nf ; gf_g] from the UNROUNDED fp32 ef' of this call and the bf16
//                                nf / gf, widened exactly — k_fn_input_node's indexing and its CSC summation order (gnx_generic.hip), so the rows
//                                carry launch_fn_input's bits on the widened inputs; no N-sized fp32 copy of nf is made.
//
// Finite data: every output is to_bf16 of gnx_chain_block_forward_wide's on the exactly widened inputs, bit for bit (the first Dense: three of
// x6_mma's six instructions multiply an all-zero plane and add +-0 to an accumulator that started at +0; the other three run in its order).
#define GNX_CHAIN_WIDE_BF16 1
#include "gnx_chain_wide_kernel.h"  // k_chain_wide_bf16<NB, SRC>, ChainWideBf16Args

namespace gnx {

struct ChainNodeRowsArgs {
  const float* ef;         // [R][E][de] fp32
  const bf16_t *nf, *gf;   // [R][N][dn], [R][G][dg] bf16
  int de, dn, dg, N, E, G;
  const int *colptr, *node_off;
  float* out;              // [R][N][de + dn + dg]
};

__global__ __launch_bounds__(256) void k_chain_node_rows_bf16(ChainNodeRowsArgs a) {
  const int K = a.de + a.dn + a.dg;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t r = blockIdx.y;
  if (idx >= (size_t)a.N * K) return;
  const int n = (int)(idx / K), k = (int)(idx % K);
  float v = 0.f;
  if (k < a.de) {
    for (int e = a.colptr[n]; e < a.colptr[n + 1]; ++e) v += a.ef[(r * a.E + e) * a.de + k];  // CSC order
  } else if (k < a.de + a.dn) {
    v = bf16_lo(a.nf[(r * a.N + n) * a.dn + (k - a.de)]);
  } else {
    v = bf16_lo(a.gf[(r * a.G + segment_of(a.node_off, a.G, n)) * a.dg + (k - a.de - a.dn)]);
  }
  a.out[r * (size_t)a.N * K + idx] = v;
}

// out: [R][N][de + dn + dg] fp32, the input rows of a wide node function of a bf16 call
int32_t launch_chain_node_rows_bf16(const gnx_graphs* h, const float* ef32, int de, const void* nf, int dn, const void* gf, int dg, int64_t R, float* out, hipStream_t s) {
  const size_t total = (size_t)h->N * (de + dn + dg);
  if (total == 0) return GNX_OK;
  ChainNodeRowsArgs a{ef32, static_cast<const bf16_t*>(nf), static_cast<const bf16_t*>(gf), de, dn, dg, (int)h->N, (int)h->E, (int)h->G, h->d_colptr, h->d_node_off, out};
  GNX_LAUNCH(k_chain_node_rows_bf16, dim3((unsigned)((total + 255) / 256), (unsigned)R), dim3(256), 0, s, a);
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

// launch_chain_wide on bf16 features.  entity 0: in0 / in1 / in2 = ef, nf, gf are bf16; 1, 2: in0 = the materialised fp32 input rows.  out: the
// bf16 rows; out32: the same rows unrounded in fp32, or nullptr.  The caller asked chain_wide_takes.
int32_t launch_chain_wide_bf16(const gnx_graphs* h, int entity, const gnx_chain& c, const void* in0, int d0, const void* in1, int d1, const void* in2, int d2,
                               void* out, float* out32, int64_t R, hipStream_t s, const char* name) {
  ChainWideBf16Args t{};
  ChainWideShape sh;
  auto cf = [](const void* q) { return static_cast<const float*>(q); };
  if (int32_t rc = chain_wide_args(h, entity, c, cf(in0), d0, cf(in1), d1, cf(in2), d2, s, "launch_chain_wide_bf16", t.f, sh)) return rc;
  if (!out) return fail(GNX_ERR_INVALID_ARG, "launch_chain_wide_bf16: the output is NULL");
  t.out = static_cast<bf16_t*>(out); t.out32 = out32;
  const dim3 grid((unsigned)sh.nwg, (unsigned)R), block(64u * sh.waves);
  const size_t lds = sizeof(float) * (size_t)sh.floats;
  ProfScope ps(name, s);
  auto go = [&](auto nb) {
    constexpr int NB = decltype(nb)::value;
    if (entity == 0) GNX_LAUNCH((k_chain_wide_bf16<NB, SRC_EDGE>), grid, block, lds, s, t);
    else GNX_LAUNCH((k_chain_wide_bf16<NB, SRC_ROWS>), grid, block, lds, s, t);
  };
  sh.nb == 1 ? go(ChainInt<1>{}) : go(ChainInt<2>{});  // (chain_wide_cut: no function with more blocks is inside the rule)
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

}  // namespace gnx
