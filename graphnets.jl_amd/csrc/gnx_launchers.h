// Functions that one translation unit of libgnx.so defines and another calls: launchers, their "does this form apply" predicates and
// their scratch-size queries.  The ONE declaration of each (the defining unit includes this header too, so a signature that drifts is
// a compile error, not a link error), and the one place their default arguments are written.  Not part of the ABI.
#pragma once
#include "gnx_internal.h"
#include "gnx_narrow_sets.h"

namespace gnx {

// What the edge launchers of the matrix-core block share (launch_edge_x6, launch_edge_enc, launch_edge_n, launch_core_edge_x6): filled once per edge
// update by launch_block_wide (gnx_wide.hip), by name — each launcher takes it plus only what is its own.
struct EdgeLaunch {
  const Tile* tiles; size_t n_tiles; const float* ef; size_t E;  // the edge rows, in 128-row tiles
  struct { const float* stats; const float* g; const float* b; bool inline_stats; float eps; int mode; } ln;  // gn1 of the edge rows: from a statistics table, or (inline_stats) in the kernel
  const float* We; int ldw;
  const float* psrc;  // the source-side table [R][N][.]: projected rows Ps (k_edge_n: the 64-wide rows themselves; encoder: nf, both sides)
  const float* pdst;  // projected rows Pd (bias and gf fold included)
  size_t N; const int* src; const int* dst; int act;
  float* out; float* colsum;  // ef' (the core form: x + ef' + FF) / its per-tile column sums or nullptr
  float* agg_out; size_t n_agg_rows; const int* chunk_row0;  // per-destination partial sums or nullptr
  int64_t R; void* scratch; hipStream_t stream;  // scratch: for the prepared weight planes when the layer brings none
};

// ---- gnx_generic.hip: dimension-generic kernels ----
int32_t launch_block_generic(const BlockArgs& a, int64_t R, int tile_n_cap, hipStream_t s, int phase);
int32_t launch_layernorm2(const float* x, size_t rows, int d, const gnx_layernorm& l1, const gnx_layernorm& l2, float eps, int eps_mode, float* y1, float* y2, hipStream_t s);
// the same on an x of bfloat16 elements (y1 / y2 fp32); the kernel form is chosen as for an fp32 x at that address
int32_t launch_layernorm2_bf16(const void* x, size_t rows, int d, const gnx_layernorm& l1, const gnx_layernorm& l2, float eps, int eps_mode, float* y1, float* y2, hipStream_t s);
int32_t launch_ffn_residual(const float* z, const float* x, size_t rows, int d, const gnx_ffn& ff, float* out, hipStream_t s);
int32_t launch_pad(const gnx_graphs* h, int kind, bool pad, const float* src, int d, int64_t R, float* dst, hipStream_t s);
int32_t launch_calibration(int n, hipStream_t s);
int xent_blocks(int64_t cols);
int32_t launch_xent_backward(const float* logits, const float* targets, int d, int64_t cols, const float* upstream, float* dl, hipStream_t s);
int32_t launch_xent(const float* logits, const float* targets, int d, int64_t cols, float* out, float* ws, hipStream_t s);
int32_t launch_collapse(const gnx_graphs* h, const float* ef, int d, int64_t R, float* out, hipStream_t s);
int32_t launch_collapse_padded(const gnx_graphs* h, const float* ef, int d, int64_t R, float* out, hipStream_t s);
int32_t launch_fn_input(const gnx_graphs* h, int kind, const float* ef, int de, const float* nf, int dn, const float* gf, int dg, int64_t R, float* out, hipStream_t s,
                        bool bf16 = false);

// ---- gnx_narrow.hip / gnx_narrow_bf16.hip / gnx_jit.cpp: the fused narrow block ----
// launch_*: 1 when the path does not apply to these dims (the caller falls through to the next path); phase: GNX_PHASE_* (gnx_internal.h)
// Which ahead-of-time forms a width set has is read from the table of gnx_narrow_sets.h, in any translation unit:
inline unsigned narrow_forms(const BlockArgs& a, bool bf16) { return narrow_forms(a.de, a.dn, a.dg, a.oe, a.on, bf16); }
// LayerNorm on load ahead of time (with bf16: the block of a bf16 core): the sets with NF_LN, at the default wave-tile size
inline bool narrow_ln_aot(const gnx_graphs* h, const BlockArgs& a, bool bf16) { return (narrow_forms(a, bf16) & NF_LN) && h->wtile_e_cap == 128; }
int32_t launch_block_narrow(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, int phase, bool bf16 = false);
void warm_block_narrow(const gnx_graphs* h, const gnx_block_params* p, bool bf16 = false);
bool block_narrow_ready(const gnx_graphs* h, const BlockArgs& a, hipStream_t s);
bool block_narrow_ffe_applies(const gnx_graphs* h, const BlockArgs& a, int act1, int act2);
bool block_narrow_chain_applies(const gnx_graphs* h, const BlockArgs& a, bool bf16 = false);
bool block_narrow_takes(const gnx_graphs* h, const BlockArgs& a, hipStream_t s, bool bf16 = false);
int32_t launch_block_narrow_chained(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, bool bf16);
bool block_narrow_run_applies(const gnx_graphs* h, const BlockArgs& a, bool bf16);
int32_t launch_block_narrow_run(const gnx_graphs* h, const BlockArgs& a, const RunTable& t, int Z, hipStream_t s, bool bf16, int phase = 3);
bool block_narrow_carry_applies(const gnx_graphs* h, const BlockArgs& a);
int32_t launch_block_narrow_carry(const gnx_graphs* h, const BlockArgs& a, const RunTable& t, int Z, const PrevTable& prev, hipStream_t s);
// gnx_narrow_bf16.hip: the same launchers on bf16 rows (a.ffe_w1 / LayerNorm on load: launch_ln_bf16); 1: the table has no such kernel
int32_t launch_fused_bf16(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, int phase);
int32_t launch_chained_bf16(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s);
int32_t launch_ln_bf16(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, int phase);
int32_t launch_run_bf16(const gnx_graphs* h, const BlockArgs& a, const RunTable& t, int Z, hipStream_t s);
bool jit_eligible(const BlockArgs& a, int ept);
int32_t jit_get(const BlockArgs& a, int ept, hipStream_t s, hipFunction_t* block, hipFunction_t* graph, bool bf16 = false);
int32_t jit_get_core_post3(int d0, int d1, int d2, hipStream_t s, hipFunction_t* fn);

// ---- gnx_core_narrow.hip: narrow-width GNCore kernels ----
bool core_narrow_width(int d);
int32_t launch_ln1_rows(const float* x, size_t rows, int d, const gnx_layernorm& l1, float eps, int eps_mode, float* y, hipStream_t s);
bool core_post3_applies(const size_t rows[3], const int d[3], const gnx_ffn ff[3], bool deferred, hipStream_t s);
// block_out (bf16 rows only; else nullptr): x and out are bf16 rows and the block's outputs are read from these fp32 buffers instead of from out
int32_t launch_core_post3(const float* const x[3], const size_t rows[3], const int d[3], const gnx_layernorm l2[3], const gnx_ffn ff[3], float eps,
                          int eps_mode, float* const out[3], hipStream_t s, const BlockArgs* blk, int n_rows, bool skip_edges = false,
                          const float* const block_out[3] = nullptr);
int32_t launch_core_post(const float* x, size_t rows, int d, const gnx_layernorm& l2, const gnx_ffn& ff, float eps, int eps_mode, float* out, hipStream_t s,
                         const float* block_out = nullptr);

// ---- gnx_wide.hip: the matrix-core block and row-wise Dense ----
int32_t launch_block_wide(const gnx_graphs* h, const BlockArgs& a, int64_t R, hipStream_t s, int phase);
size_t wide_workspace_bytes(const gnx_graphs* h, const gnx_block_params* p, int64_t R);
void warm_block_wide(const gnx_graphs* h, const gnx_block_params* p, bool rows_gemm);
bool block_wide_ln_applies(const gnx_graphs* h, const BlockArgs& a);
bool block_wide_edge_x6_applies(const gnx_graphs* h, const BlockArgs& a);
int32_t launch_dense_rows(const gnx_graphs* h, int entity, const float* A, int K, const gnx_dense& d, int OUT, const float* add1,
                          const float* add2, float* out, int64_t R, hipStream_t s, const char* name);
int32_t launch_rows_matmul(const gnx_graphs* h, int entity, const float* A, int K, const float* B, int ldw, int OUT, float* out, int64_t R,
                           hipStream_t s, const char* name, const float* gmul, int gmul_act, float* tile_colsum, int* n_tiles_out, const float* add1);

// ---- gnx_ffn_fused.hip / gnx_ffn_x6.hip: FeedForward + residual on the matrix cores, row statistics ----
int32_t launch_ffn_fused(const gnx_graphs* h, int entity, const float* z, int d, const gnx_ffn& ff, const float* add1, const float* add2, float* out,
                         int64_t R, hipStream_t s, const float* ln_stats = nullptr, const gnx_layernorm* ln = nullptr, void* scratch = nullptr, size_t scratch_bytes = 0,
                         bool ln_inline = false, float ln_eps = 0.f, int ln_mode = 0);
bool ffn_fused_applies(const float* z, int d, const gnx_ffn& ff, const float* add1, const float* add2, const float* out);
bool ln_stats_applies(const float* x, int d);
int32_t launch_ln_stats(const float* x, size_t rows, int d, float eps, int eps_mode, float* stats, hipStream_t s);
bool ffn_x6_applies(const float* z, int d, const gnx_ffn& ff, const float* add1, const float* add2, const float* out, size_t scratch_bytes);
int32_t launch_ffn_x6(const float* z, size_t nrows, int d, const gnx_ffn& ff, const float* add1, const float* add2, float* out, int64_t R, hipStream_t s,
                      const float* ln_stats, const gnx_layernorm* ln, void* scratch, bool ln_inline, float ln_eps, int ln_mode);
int32_t launch_ffn_x6_prep(const float* W1, const float* W2, int d, void* scratch, hipStream_t s, const float* ln_gamma, const float* ln_beta, const float* b1);
size_t ffn_x6_scratch_bytes(int d);
size_t ffn_x6_fold_scratch_bytes(int d);
int32_t launch_core_edge_x6(const EdgeLaunch& e, const gnx_ffn& ff, const gnx_layernorm* ln2, void* scratch_f);  // (e.ln: gn1, folded into the planes; e.out: the CORE's edge output)

// ---- gnx_edge_x6.hip: the six-term edge / projection / node kernels of the matrix-core block ----
int32_t launch_edge_x6(const EdgeLaunch& e, int oe);  // oe: 128, or 1..32 (the narrow form: one zero-padded slice, no per-destination sums)
int32_t launch_edge_x6_prep(const float* We, int ldw, void* scratch, hipStream_t s, int n_out, const float* ln_gamma, const float* ln_beta);
size_t edge_x6_scratch_bytes();
size_t edge_x6_fold_scratch_bytes();
int32_t launch_fold_beta(const float* W, int ldw, int K, int n_out, const float* beta, const float* bias, float* out, hipStream_t s);
bool proj_x6_applies(int dn, int oe, const float* nf, const float* W, const float* out, size_t N);
int32_t launch_proj_x6(const Tile* tiles, size_t n_tiles, const float* nf, size_t N, const float* ln_stats, const float* ln_g, const float* ln_b, const float* Ws, const float* Wd,
                       int ldw, const float* bias, const float* bias_g, int G, float* out_s, float* out_d, int64_t R, void* scratch, hipStream_t s, bool only_d = false,
                       float* zn_out = nullptr);
int32_t launch_proj_x6_prep(const float* Ws, const float* Wd, int ldw, void* scratch, hipStream_t s);
size_t proj_x6_scratch_bytes();
// the encoder form of k_edge_x6 ((10, 5, .) => 128 unprojected; e.psrc: nf, e.pdst and e.ln unused)
int32_t launch_edge_enc(const EdgeLaunch& e, const float* bias, const float* bias_g, int G);
int32_t launch_edge_enc_prep(const float* We, int ldw, void* scratch, hipStream_t s);
size_t edge_enc_scratch_bytes();
bool node_x6_applies(int oe, int dn, int on, int act, const float* nf, const float* Wn, const float* out, size_t N);
int32_t launch_node_x6(const Tile* tiles, size_t n_tiles, const float* nf, size_t N, const float* ln_stats, const float* ln_g, const float* ln_b, const float* agg,
                       size_t n_agg_rows, const int* agg_row, const int* agg_parts, const int* agg_chunk, const int* chunk_row0, const float* Wn, int ldw, const float* bias,
                       const float* bias_g, int G, int act, float* out, float* colsum, int64_t R, void* scratch, hipStream_t s);
int32_t launch_node_x6_prep(const float* Wn, int ldw, void* scratch, hipStream_t s);
size_t node_x6_scratch_bytes();

// ---- gnx_edge_n.hip: the edge update with the source side gathered raw (K = 128 + 64) and a register epilogue ----
bool edge_n_enabled();
size_t edge_n_scratch_bytes();
int32_t launch_edge_n(const EdgeLaunch& e);  // (e.psrc: the 64-wide source rows, raw or normalised)

// ---- gnx_bf16.hip: bf16 <-> fp32 conversion of whole tensors ----
int32_t launch_bf16_widen(const void* src, size_t n, float* dst, hipStream_t s);
int32_t launch_bf16_round(const float* src, size_t n, void* dst, hipStream_t s);

// ---- gnx_backward_wide.hip: matrix-core primitives of the backward pass ----
bool bw_use_mfma(size_t rows, int J, int K);     // dX
bool bw_use_mfma_dw(size_t rows, int J, int K);  // dW
size_t dw_mfma_partial_floats(size_t rows, int J, int K);
int32_t dw_mfma(const float* delta, const float* X, size_t rows, int J, int K, float* dW, float* partial, hipStream_t s);
int32_t dx_mfma(const gnx_graphs* h, int entity, const float* delta, const float* W, int J, int K, int ka, int kb, float* out, int64_t R,
                float* WT, bool fill, hipStream_t s, const char* name, const float* gmul = nullptr, int gmul_act = 0, float* tile_colsum = nullptr, int* n_tiles_out = nullptr);
int32_t transpose_w(const float* W, int K, int J, float* WT, hipStream_t s);
int32_t rows_times_wt(const gnx_graphs* h, int entity, const float* A, int J, const float* WT, int K, int ka, int kb, float* out, const float* add1,
                      int64_t R, hipStream_t s, const char* name);
int32_t segsum_rows(const float* src, const int* ptr, const int* idx, int N, int E, int D, int64_t R, float* out, hipStream_t s, const char* name);
int32_t add_cols(const float* in, int ld, int off, size_t rows, int d, float* out, int accumulate, hipStream_t s);

// ---- gnx_backward_narrow.hip: the edge level of the block backward at narrow widths in one kernel (gnx_block_backward_fused) ----
struct BwEdgeWave;  // the kernel's argument record: gnx_bw_edge_wave_kernel.h
bool bw_edge_wave_has(int de, int dn, int dg, int oe);  // is the width set instantiated?
size_t bw_edge_wave_rows(const gnx_graphs* h);          // partial rows per replica
// bf16: ef, nf, gf, g_ef_out, ef_out and d_ef hold bfloat16 elements (declared float, like the feature pointers of BlockArgs)
int32_t launch_bw_edge_wave(const gnx_block_params* p, const BwEdgeWave& a, int64_t R, hipStream_t s, bool bf16 = false);
// gnx_jit.cpp: the same kernel specialised at run time (gnx_block_backward_narrow).  Eligible: oe >= 1, Ke >= 1, oe Ke < 64 (at most two
// (k, j) pairs per lane), the kernel's static LDS within a workgroup's 64 KB, run-time specialisation enabled.
bool jit_bw_edge_eligible(int de, int dn, int dg, int oe);
// 0: *fn is ready; 1: not available (the caller runs the generic edge level).  Never compiles or loads while `s` is being captured.
int32_t jit_get_bw_edge(int de, int dn, int dg, int oe, bool bf16, hipStream_t s, hipFunction_t* fn);
// the launch of launch_bw_edge_wave with that function
int32_t launch_bw_edge_wave_jit(hipFunction_t fn, const BwEdgeWave& a, int64_t R, hipStream_t s);

// ---- gnx_core_bw_narrow.hip: the FeedForward pullback of the core backward at narrow widths in one kernel (gnx_core_backward_narrow) ----
size_t core_bw_narrow_rows(size_t rows, int d);  // partial rows (= workgroups) of the launch over `rows` rows at width d
// dz2 = the pullback of ff through z = gn2(x) with upstream g; part1 / part2: [core_bw_narrow_rows][4d (d + 1)] / [..][d (4d + 1)] partial rows of
// fc1's / fc2's weight and bias gradient in k_bw_dw_final's pair order, or nullptr (not wanted).  d: a core_narrow_width; fc1 identity or relu
int32_t launch_core_bw_narrow(const float* z, const float* g, const gnx_ffn& ff, size_t rows, int d, float* dz2, float* part1, float* part2, hipStream_t s);

// ---- gnx_dropout.hip ----
bool dropout_active(const gnx_dropout* d);
int32_t check_dropout(const gnx_dropout* d);
int32_t launch_dropout(const gnx_dropout& d, int entity, size_t n, const float* in, float* out, int mode, hipStream_t s);

// ---- gnx_core_train_narrow.hip: the training-mode FeedForward + Dropout + residuals of a narrow core in one kernel (gnx_core_forward_train_typed) ----
// launch_ln1_rows on bfloat16 rows (y fp32)
int32_t launch_ln1_rows_bf16(const void* x, size_t rows, int d, const gnx_layernorm& l1, float eps, int eps_mode, float* y, hipStream_t s);
// y = fmaf(m, ffwd(gn2(x)), x + block_out), m the mask of `dr` for `entity`; x and y hold bfloat16 elements with bf16, block_out is fp32.
// d: a core_narrow_width; fc1 identity or relu, fc2 identity
int32_t launch_core_post_train(const void* x, size_t rows, int d, const gnx_layernorm& l2, const gnx_ffn& ff, float eps, int eps_mode, const float* block_out,
                               const gnx_dropout& dr, int entity, void* y, bool bf16, hipStream_t s);

// ---- gnx_chain_narrow.hip: one update function of a Chain block in one kernel (gnx_chain_block_forward_narrow; the rule: gnx_chain_plan.h) ----
// entity 0: in0 / in1 / in2 = ef, nf, gf (widths d0, d1, d2); 1: ef', nf, gf; 2: in0 = the materialised [R G][d0] input rows (d1 = d2 = 0)
int32_t launch_chain_narrow(const gnx_graphs* h, int entity, const gnx_chain& c, const float* in0, int d0, const float* in1, int d1, const float* in2, int d2,
                            float* out, int64_t R, hipStream_t s, const char* name);
// ---- gnx_chain_narrow_bf16.hip: the same on bf16 features (gnx_chain_block_forward_typed's native path) ----
// entity 0: in0 / in1 / in2 are bf16; 1: in0 is the fp32 ef' of this call, in1 / in2 are bf16; 2: in0 is fp32.  out: bf16 rows, or nullptr
// (the pullback's recompute); out32: the same rows unrounded in fp32, or nullptr.  The caller asked chain_narrow_takes.
int32_t launch_chain_narrow_bf16(const gnx_graphs* h, int entity, const gnx_chain& c, const void* in0, int d0, const void* in1, int d1, const void* in2, int d2,
                                 void* out, float* out32, int64_t R, hipStream_t s, const char* name);

// ---- gnx_chain_bw_narrow.hip: the pullback of one update function of a Chain block in one kernel (gnx_chain_block_backward_narrow) ----
struct ChainBwNarrowIo {
  const float* G;                           // upstream gradient of the function's output, or nullptr
  const float* ex1; int ex1_stride, ex1_off;  // dXg [R G][ex1_stride], columns from ex1_off (node / edge level), or nullptr
  const float* ex2; int ex2_stride;           // dXn [R N][ex2_stride], columns from 0 (edge level), or nullptr
  float* dx; int dx_c0;                     // columns [dx_c0, K) of the input gradient, rows of length K - dx_c0, or nullptr
  float* direct;                            // columns [0, dx_c0), rows of length dx_c0 (d_ef), or nullptr
  float* part;                              // [sum_l P_l][R nwg] partial rows (layer l at part + part_off[l] * R * nwg), or nullptr
};
// entity / in0..in2 as launch_chain_narrow.  The caller asked chain_bw_narrow_takes and opens the ProfScope.
int32_t launch_chain_bw_narrow(const gnx_graphs* h, int entity, const gnx_chain& c, const float* in0, int d0, const float* in1, int d1, const float* in2, int d2,
                               const ChainBwNarrowIo& io, int64_t R, hipStream_t s);
// ---- gnx_chain_bw_narrow_bf16.hip: the same on bf16 features (gnx_chain_block_backward_narrow_typed's native path) ----
// in0 .. in2 as launch_chain_narrow_bf16; io.G and io.direct hold bfloat16 elements (declared float), io.ex1, io.ex2, io.dx and io.part are fp32
int32_t launch_chain_bw_narrow_bf16(const gnx_graphs* h, int entity, const gnx_chain& c, const void* in0, int d0, const void* in1, int d1, const void* in2, int d2,
                                    const ChainBwNarrowIo& io, int64_t R, hipStream_t s);
// ---- gnx_chain_train_narrow.hip / gnx_chain_bw_train_narrow.hip: the two launchers above for a function with Dropout entries (a training call:
//      every entry bound to its ChainDropSite).  launch_chain_narrow / launch_chain_bw_narrow hand such a chain over themselves ----
int32_t launch_chain_narrow_train(const gnx_graphs* h, int entity, const gnx_chain& c, const float* in0, int d0, const float* in1, int d1, const float* in2, int d2,
                                  float* out, int64_t R, hipStream_t s, const char* name);
int32_t launch_chain_bw_narrow_train(const gnx_graphs* h, int entity, const gnx_chain& c, const float* in0, int d0, const float* in1, int d1, const float* in2,
                                     int d2, const ChainBwNarrowIo& io, int64_t R, hipStream_t s);

// ---- gnx_forward.hip: the validation of a core forward, for the training-mode entries of gnx_dropout.hip (a FormScope of the call's flags open) ----
int32_t core_forward_check_dims(const gnx_core_params* p);  // (needs no handle)
int32_t core_forward_check(const gnx_graphs* h, const gnx_core_params* p, int64_t R, const void* ef, const void* nf, const void* gf, const void* ef_out,
                           const void* nf_out, const void* gf_out, uint32_t flags);

// ---- gnx_build_device.hip: the CSC of a dense batch built on the device ----
int32_t build_csc_on_device(const void* const* adj, const void* packed, int packed_on_device, const int64_t* n_nodes, int64_t G, int32_t elem_kind, int32_t row_major,
                            gnx::vec_i64& h_colptr, gnx::vec_i64& h_rowval, const std::vector<int64_t>& h_node_off, DenseCscOnDevice* keep);

}  // namespace gnx
