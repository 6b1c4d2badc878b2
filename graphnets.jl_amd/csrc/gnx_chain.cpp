// GNBlock whose update functions are Flux `Chain`s of `Dense` layers.
//
// The reference's GNBlock is a struct of three arbitrary Chains (src/gnblock.jl:1-6); its constructor builds `Chain(Dense)` for
// each (src/gnblock.jl:55-60) and that one-layer form is what gnx_block_forward fuses.  Users replace them by MLPs
// (`GNBlock(Chain(Dense(20 => 64, relu), Dense(64 => 3)), ...)`): this entry point runs such a block, composed from the pieces the
// library already has — no new kernels:
//   (a LayerNorm as the edge function's first layer: run behind an identity Dense — gnx_internal.h, ChainLnFirst)
//   edge function : its FIRST Dense is the edge update of a one-layer block (gnx_block_forward with node / graph outputs switched
//                   off: the fused / matrix-core edge kernels, the (K_e, E) input never materialised); further layers are row-wise
//                   Dense launches (k_rows_gemm) over [E][width] arrays that ping-pong in the workspace;
//   node function : getnodefninput (gnx_fn_input kind 1: [sum_{e->n} ef' ; nf ; gf_g], N rows) then row-wise Dense layers;
//   graph function: getgraphfninput (kind 2, G rows) then row-wise Dense layers.
// Semantics are exactly (m::GNBlock)(x) of src/gnblock.jl:63-69 with Chain update functions; zero-width outputs -> `nothing`.
// gnx_chain_block_forward_narrow: the same block with every update function whose input and layer widths are at most 32 in ONE kernel
// (gnx_chain_narrow.hip: k_chain_mlp, a row per lane through all layers); a function outside that rule runs the launches above.
// gnx_chain_block_forward_typed: either entry on bfloat16 features — where every function that runs is inside the rule, the same kernels reading
// and writing bf16 rows (gnx_chain_narrow_bf16.hip); elsewhere fp32 copies around the fp32 entry (gnx_staging.h).
#include <algorithm>

#include "gnx_launchers.h"
#include "gnx_staging.h"

using namespace gnx;

// A `LayerNorm(d)` layer value of a Chain (gnx_dense.kind = GNX_LAYER_LAYERNORM): y = gamma . (x - mean) / (sigma + eps) + beta per row, one
// wavefront per row, any width — the arithmetic of k_layernorm2 (gnx_generic.hip), i.e. of GNGraphNorm's LayerNorms (gngraphnorm.jl:19-26)
__global__ __launch_bounds__(256) void k_chain_layernorm(const float* __restrict__ x, size_t rows, int d, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float eps, int eps_mode, float* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * d;
  float s = 0.f;
  for (int k = lane; k < d; k += 64) s += xr[k];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float mu = s / (float)d;
  float v = 0.f;
  for (int k = lane; k < d; k += 64) { const float c = xr[k] - mu; v = fmaf(c, c, v); }
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  v /= (float)d;
  const float inv = eps_mode == 0 ? 1.f / (sqrtf(v) + eps) : 1.f / sqrtf(v + eps);
  for (int k = lane; k < d; k += 64) y[row * d + k] = fmaf(gamma[k], (xr[k] - mu) * inv, beta[k]);
}

__global__ void k_chain_identity(float* __restrict__ w, int k) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)k * k) w[i] = (i / k == i % k) ? 1.f : 0.f;
}

namespace gnx {
int32_t ChainLnFirst::fill(float* ident, hipStream_t s) const {
  if (!on || ke == 0) return GNX_OK;
  GNX_LAUNCH(k_chain_identity, dim3((unsigned)(((size_t)ke * ke + 255) / 256)), dim3(256), 0, s, ident, ke);
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}
// one layer of a Chain, row-wise over all rows of the entity: Dense (launch_dense_rows) or LayerNorm; shared with the backward's recompute
int32_t launch_chain_layer(const gnx_graphs* h, int entity, const gnx_dense& layer, const float* x, int k_in, int width, float* out, int64_t R, hipStream_t s,
                           const char* name) {
  if (chain_layer_is_dropout(layer)) {  // a training call's entry (ChainTrain): out = x .* mask, the mask of the entry's site
    const ChainDropSite* st = chain_drop_site(layer);
    if (!st) return fail(GNX_ERR_INVALID_ARG, "Chain: a Dropout entry outside a training call");
    const size_t n = (size_t)R * (entity == 0 ? (size_t)h->E : (entity == 1 ? (size_t)h->N : (size_t)h->G)) * (size_t)width;
    return launch_dropout(gnx_dropout{st->p, 0, st->seed}, (int)st->stream, n, x, out, 1, s);
  }
  if (!chain_layer_is_ln(layer)) return launch_dense_rows(h, entity, x, k_in, layer, width, nullptr, nullptr, out, R, s, name);
  const size_t rows = (size_t)R * (entity == 0 ? (size_t)h->E : (entity == 1 ? (size_t)h->N : (size_t)h->G));
  if (rows == 0 || width == 0) return GNX_OK;
  ProfScope ps("k_chain_layernorm", s);
  GNX_LAUNCH(k_chain_layernorm, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, rows, width, layer.weight, layer.bias, kChainLnEps, chain_layer_ln_mode(layer), out);
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}
}  // namespace gnx

namespace {

int32_t check_chain(const gnx_chain& c, const char* what, int k_in, bool train) {
  if (c.n_layers < 0 || c.n_layers > kChainMaxLayers) return fail(GNX_ERR_INVALID_ARG, std::string(what) + ": n_layers must be 0..16");
  if (c.n_layers > 0 && (!c.layers || !c.widths)) return fail(GNX_ERR_INVALID_ARG, std::string(what) + ": layers / widths is NULL");
  for (int i = 0; i < c.n_layers; ++i) {
    if (c.widths[i] < 0) return fail(GNX_ERR_DIMS, std::string(what) + ": negative layer width");
    if (i + 1 < c.n_layers && c.widths[i] == 0) return fail(GNX_ERR_DIMS, std::string(what) + ": only the last layer of a Chain may have width 0");
    if (c.layers[i].act < GNX_ACT_IDENTITY || c.layers[i].act > GNX_ACT_GELU) return fail(GNX_ERR_INVALID_ARG, std::string(what) + ": unknown activation");
    const int kind = c.layers[i].kind & 0xff;
    if (train && kind == GNX_LAYER_DROPOUT) continue;  // (placed, shaped and bound to its site by ChainTrain)
    if (kind != GNX_LAYER_DENSE && kind != GNX_LAYER_LAYERNORM) return fail(GNX_ERR_INVALID_ARG, std::string(what) + ": unknown layer kind");
    if (kind == GNX_LAYER_LAYERNORM) {  // a LayerNorm(d) layer value: gamma, beta of its input's width, no activation of its own
      if (c.widths[i] != (i > 0 ? c.widths[i - 1] : k_in)) return fail(GNX_ERR_DIMS, std::string(what) + ": a LayerNorm layer keeps the width of its input");
      if (c.layers[i].act != GNX_ACT_IDENTITY) return fail(GNX_ERR_INVALID_ARG, std::string(what) + ": a LayerNorm layer has no activation");
      if (c.widths[i] > 0 && (!c.layers[i].weight || !c.layers[i].bias)) return fail(GNX_ERR_INVALID_ARG, std::string(what) + ": a LayerNorm layer needs gamma and beta");
    }
  }
  return GNX_OK;
}

int32_t check_params(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t R, bool train = false) {
  if (!h || !p) return fail(GNX_ERR_INVALID_ARG, "NULL handle or params");
  if (R <= 0 || (R > 1 && h->G != 1) || R > 65535) return fail(GNX_ERR_INVALID_ARG, "bad n_replicas");
  if (p->de < 0 || p->dn < 0 || p->dg < 0) return fail(GNX_ERR_DIMS, "negative feature width");
  if (p->de + p->dn + p->dg == 0) return fail(GNX_ERR_DIMS, "all input widths are 0 (gnblock.jl:48, batch.jl:56)");
  auto out_width = [](const gnx_chain& c) { return c.n_layers > 0 ? c.widths[c.n_layers - 1] : 0; };
  int32_t rc;
  if ((rc = check_chain(p->edgefn, "edgefn", p->de + 2 * p->dn + p->dg, train))) return rc;
  const int oe = out_width(p->edgefn);
  if ((rc = check_chain(p->nodefn, "nodefn", oe + p->dn + p->dg, train))) return rc;
  const int on = out_width(p->nodefn);
  if ((rc = check_chain(p->graphfn, "graphfn", oe + on + p->dg, train))) return rc;
  if (oe + on + out_width(p->graphfn) == 0) return fail(GNX_ERR_DIMS, "all output widths are 0 (gnblock.jl:49)");
  // A zero-width ef' / nf' is an empty segment of the next function's input, exactly as for one-layer update functions
  // (gnblock.jl:63-69 computes getnodefninput / getgraphfninput over the 0-row h_ef; width 0 <=> nothing in launch_fn_input).
  return GNX_OK;
}

}  // namespace

namespace gnx {

ChainPlan::ChainPlan(const gnx_graphs* h, const gnx_chain_block_params* p0, int64_t R, int32_t elem, bool narrow, ChainRule rule, const char* const query_of[3], bool train)
    : rc(check_params(h, p0, R, train)) {
  if (rc) return;
  bf16 = elem == GNX_ELEM_BF16;
  query = query_of[bf16 ? 2 : narrow];
  sh = chain_shape(h->E, h->N, h->G, *p0, R);
  fused = narrow ? chain_fused_mask(sh, rule) : 0;
  p = (fused & 1) ? p0 : lnf.init(p0, nullptr);  // (the identity layer's weights sit at a fixed place of the workspace: bind_ident)
  if (lnf.on) sh = chain_shape(h->E, h->N, h->G, *p, R);
}
// The refusals in include/gnx.h's order — the chains' arrays, every p_l, a missing p[t], the entries' places and shapes — then the copy.
ChainTrain::ChainTrain(const gnx_chain_block_params* p0, const gnx_chain_dropout* d, bool every_entry) {
  if (!p0) { rc = fail(GNX_ERR_INVALID_ARG, "NULL handle or params"); return; }
  const gnx_chain* in[3] = {&p0->edgefn, &p0->nodefn, &p0->graphfn};
  const char* const what[3] = {"edgefn", "nodefn", "graphfn"};
  for (int t = 0; t < 3; ++t) {
    if (in[t]->n_layers < 0 || in[t]->n_layers > kChainMaxLayers) { rc = fail(GNX_ERR_INVALID_ARG, std::string(what[t]) + ": n_layers must be 0..16"); return; }
    if (in[t]->n_layers > 0 && (!in[t]->layers || !in[t]->widths)) { rc = fail(GNX_ERR_INVALID_ARG, std::string(what[t]) + ": layers / widths is NULL"); return; }
  }
  auto is_drop = [&](int t, int i) { return chain_layer_is_dropout(in[t]->layers[i]); };
  for (int t = 0; t < 3 && d; ++t)
    for (int i = 0; i < in[t]->n_layers && d->p[t]; ++i)
      if (is_drop(t, i) && !(d->p[t][i] >= 0.f && d->p[t][i] <= 1.f)) { rc = fail(GNX_ERR_INVALID_ARG, std::string(what[t]) + ": Dropout: p must lie in [0, 1] (Flux.Dropout asserts 0 <= p <= 1)"); return; }
  for (int t = 0; t < 3 && d; ++t)
    for (int i = 0; i < in[t]->n_layers && !d->p[t]; ++i)
      if (is_drop(t, i)) { rc = fail(GNX_ERR_INVALID_ARG, std::string(what[t]) + ": the chain has a Dropout entry and gnx_chain_dropout.p of the function is NULL"); return; }
  for (int t = 0; t < 3; ++t)
    for (int i = 0; i < in[t]->n_layers; ++i) {
      if (!is_drop(t, i)) continue;
      const gnx_dense& l = in[t]->layers[i];
      if (i == 0 || is_drop(t, i - 1)) { rc = fail(GNX_ERR_INVALID_ARG, std::string(what[t]) + ": a Dropout entry follows a Dense or LayerNorm entry (never first, never behind another Dropout)"); return; }
      if (in[t]->widths[i] != in[t]->widths[i - 1]) { rc = fail(GNX_ERR_INVALID_ARG, std::string(what[t]) + ": a Dropout entry keeps the width of the entry in front of it"); return; }
      if (l.weight || l.bias || l.act != GNX_ACT_IDENTITY || l.kind != GNX_LAYER_DROPOUT) { rc = fail(GNX_ERR_INVALID_ARG, std::string(what[t]) + ": a Dropout entry has no weight, no bias and no activation"); return; }
    }
  p = *p0;
  gnx_chain* out[3] = {&p.edgefn, &p.nodefn, &p.graphfn};
  for (int t = 0; t < 3; ++t) {
    int n = 0;
    for (int i = 0; i < in[t]->n_layers; ++i) {
      gnx_dense l = in[t]->layers[i];
      if (is_drop(t, i)) {
        const float pl = every_entry ? 0.5f : (d ? d->p[t][i] : 0.f);
        if (!(pl > 0.f)) continue;  // the identity: removed
        sites[t][n] = ChainDropSite{d ? d->seed : 0, pl, (uint32_t)(16 + 16 * t + i)};
        l.bias = reinterpret_cast<const float*>(&sites[t][n]);  // (never read as floats: chain_drop_site)
        active = true;
      }
      layers[t][n] = l; widths[t][n] = in[t]->widths[i]; src[t][n] = i;
      ++n;
    }
    out[t]->layers = layers[t]; out[t]->widths = widths[t]; out[t]->n_layers = n;
  }
}
const gnx_chain_block_grads* ChainTrain::map_grads(const gnx_chain_block_grads* g0) {
  if (!g0) return nullptr;
  grads = *g0;
  const gnx_dense_grad* in[3] = {g0->edgefn, g0->nodefn, g0->graphfn};
  const gnx_chain* ch[3] = {&p.edgefn, &p.nodefn, &p.graphfn};
  for (int t = 0; t < 3; ++t)
    for (int i = 0; in[t] && i < ch[t]->n_layers; ++i) g[t][i] = chain_layer_is_dropout(layers[t][i]) ? gnx_dense_grad{nullptr, nullptr} : in[t][src[t][i]];
  if (g0->edgefn) grads.edgefn = g[0];
  if (g0->nodefn) grads.nodefn = g[1];
  if (g0->graphfn) grads.graphfn = g[2];
  return &grads;
}

int32_t chain_check_features(const ChainShape& sh, const void* ef, const void* nf, const void* gf, const char* message) {
  return (sh.de > 0 && !ef && sh.trows[0] > 0) || (sh.dn > 0 && !nf) || (sh.dg > 0 && !gf) ? fail(GNX_ERR_INVALID_ARG, message) : GNX_OK;
}

}  // namespace gnx

namespace {

// layers [first, n) of a chain, row-wise: x [rows][k_in] -> ... -> out [rows][out_width]; intermediates ping-pong in buf[0/1]
int32_t run_layers(const gnx_graphs* h, int entity, const gnx_chain& c, int first, const float* x, int k_in, float* const buf[2], float* out,
                   int64_t R, hipStream_t s, const char* name) {
  const float* cur = x;
  int k = k_in;
  for (int i = first; i < c.n_layers; ++i) {
    float* dst = i + 1 == c.n_layers ? out : buf[(i - first) & 1];
    if (c.widths[i] > 0 && k > 0 && !c.layers[i].weight && !chain_layer_is_dropout(c.layers[i])) return fail(GNX_ERR_INVALID_ARG, "Chain: Dense weight is NULL");
    const int32_t rc = launch_chain_layer(h, entity, c.layers[i], cur, k, c.widths[i], dst, R, s, name);
    if (rc) return rc;
    cur = dst;
    k = c.widths[i];
  }
  return GNX_OK;
}

// What every Chain forward entry receives.  The six feature-shaped tensors hold `elem` elements.
struct ChainFwCall {
  const gnx_graphs* h; const gnx_chain_block_params* p; int32_t elem;
  const void *ef, *nf, *gf; int64_t R; void *ef_out, *nf_out, *gf_out, *ws; size_t ws_bytes; uint32_t flags; void* stream;
};

// The forward's plan.  native: a bf16 call whose every running function is fused — one k_chain_mlp_bf16 launch each, three fp32 carves behind the
// layout (chain_native_counts); any other bf16 call is staged: fp32 copies of its six tensors around the fp32 launches.  wide_tables: the
// row-wise layers and a fused edge function read the matrix-core tables; the query builds them outside any capture.
const char* const kFwQuery[3] = {"workspace missing or smaller than gnx_chain_block_workspace_bytes()", "workspace missing or smaller than gnx_chain_block_forward_narrow_workspace_bytes()",
                                 "workspace missing or smaller than gnx_chain_block_forward_typed_workspace_bytes()"};
struct ChainFwPlan : ChainPlan {
  bool native = false;
  ChainWs w{};
  ChainFwPlan(const gnx_graphs* h, const gnx_chain_block_params* p0, int64_t R, int32_t elem, bool narrow, bool train = false)
      : ChainPlan(h, p0, R, elem, narrow, CHAIN_RULE_FW, kFwQuery, train) {
    native = !rc && bf16 && narrow && chain_typed_native(sh, fused);
  }
  bool wide_tables() const { return chain_fw_reads_wide_tables(sh, fused); }
  void lay_out(const gnx_graphs* h) {  // (the inner block's query builds what its edge update reads of the handle)
    w = chain_fw_layout(sh, fused, lnf.ident_floats(), sh.ow[0] > 0 && !(fused & 1) ? gnx_block_workspace_bytes(h, &sh.edge_block, sh.R) : 0);
    size_t counts[3];
    chain_native_counts(sh, counts);
    const int d[6] = {sh.de, sh.dn, sh.dg, sh.ow[0], sh.ow[1], sh.ow[2]};
    sized(w.total, native ? stage_layout(w.total, counts, 3) : stage_features(w.total, h, sh.R, d, 6));
  }
};

// the fp32 launches of a checked call on its plan's layout: a fused function in one kernel, any other as the composition at the head of this file
int32_t chain_forward_fp32(const ChainFwCall& c, ChainFwPlan& pl, const float* ef, const float* nf, const float* gf, float* ef_out, float* nf_out, float* gf_out) {
  const gnx_graphs* h = c.h;
  const hipStream_t s = (hipStream_t)c.stream;
  const ChainWs& w = pl.w;
  char* base = static_cast<char*>(c.ws);
  auto F = [&](const ChainCarve& v) { return reinterpret_cast<float*>(base + v.off); };
  int32_t rc;
  pl.bind_ident(F(w.ident));
  if ((rc = pl.lnf.fill(F(w.ident), s))) return rc;
  const gnx_chain_block_params* p = pl.p;
  const unsigned fused = pl.fused;
  const int de = p->de, dn = p->dn, dg = p->dg, oe = pl.sh.ow[0], on = pl.sh.ow[1], og = pl.sh.ow[2], Kn = pl.sh.k0[1], Kg = pl.sh.k0[2];
  // ---- edge function (gnblock.jl:65): first Dense fused with getedgefninput, the rest row-wise ----
  if (fused & 1) {
    if ((rc = launch_chain_narrow(h, 0, p->edgefn, ef, de, nf, dn, gf, dg, ef_out, c.R, s, "k_rows_gemm_chain_e"))) return rc;
  } else if (oe > 0 && h->E > 0) {
    float* first_out = p->edgefn.n_layers == 1 ? ef_out : F(w.e_buf[0]);
    if ((rc = gnx_block_forward(h, &pl.sh.edge_block, ef, nf, gf, c.R, first_out, nullptr, nullptr, base + w.block.off, w.block.bytes, c.flags, c.stream))) return rc;
    if (p->edgefn.n_layers > 1) {
      float* const bufs[2] = {F(w.e_buf[1]), F(w.e_buf[0])};  // layer 1 reads e_buf[0], writes e_buf[1], ...
      if ((rc = run_layers(h, 0, p->edgefn, 1, first_out, p->edgefn.widths[0], bufs, ef_out, c.R, s, "k_rows_gemm_chain_e"))) return rc;
    }
  }
  // ---- node function (gnblock.jl:66): sees the NEW ef', the OLD nf and gf ----
  if (fused & 2) {
    if ((rc = launch_chain_narrow(h, 1, p->nodefn, ef_out, oe, nf, dn, gf, dg, nf_out, c.R, s, "k_rows_gemm_chain_n"))) return rc;
  } else if (on > 0) {
    if ((rc = launch_fn_input(h, 1, ef_out, oe, nf, dn, gf, dg, c.R, F(w.n_in), s))) return rc;
    float* const bufs[2] = {F(w.n_buf[0]), F(w.n_buf[1])};
    if ((rc = run_layers(h, 1, p->nodefn, 0, F(w.n_in), Kn, bufs, nf_out, c.R, s, "k_rows_gemm_chain_n"))) return rc;
  }
  // ---- graph function (gnblock.jl:67): NEW ef', NEW nf', OLD gf ----
  if (og > 0) {
    if ((rc = launch_fn_input(h, 2, ef_out, oe, nf_out, on, gf, dg, c.R, F(w.g_in), s))) return rc;
    if (fused & 4) {
      if ((rc = launch_chain_narrow(h, 2, p->graphfn, F(w.g_in), Kg, nullptr, 0, nullptr, 0, gf_out, c.R, s, "k_rows_gemm_chain_g"))) return rc;
    } else {
      float* const bufs[2] = {F(w.g_buf[0]), F(w.g_buf[1])};
      if ((rc = run_layers(h, 2, p->graphfn, 0, F(w.g_in), Kg, bufs, gf_out, c.R, s, "k_rows_gemm_chain_g"))) return rc;
    }
  }
  return GNX_OK;
}

// the native bf16 launches (ChainPlan::native): every function that runs is one k_chain_mlp_bf16 launch on the bf16 rows; ef' / nf' unrounded and
// the widened gf sit in the plan's three carves for the functions of this call that read them
int32_t chain_forward_native(const ChainFwCall& c, const ChainFwPlan& pl) {
  const gnx_graphs* h = c.h;
  const gnx_chain_block_params* p = pl.p;
  const hipStream_t s = (hipStream_t)c.stream;
  const int oe = pl.sh.ow[0], on = pl.sh.ow[1], og = pl.sh.ow[2];
  auto at = [&](int i) { return pl.st.n[i] > 0 ? pl.st.at(c.ws, i) : nullptr; };
  float *ef32 = at(0), *nf32 = at(1);
  int32_t rc;
  if (pl.fused & 1) {
    if ((rc = launch_chain_narrow_bf16(h, 0, p->edgefn, c.ef, p->de, c.nf, p->dn, c.gf, p->dg, c.ef_out, ef32, c.R, s, "k_rows_gemm_chain_e"))) return rc;
  }
  if (pl.fused & 2) {
    if ((rc = launch_chain_narrow_bf16(h, 1, p->nodefn, ef32, oe, c.nf, p->dn, c.gf, p->dg, c.nf_out, nf32, c.R, s, "k_rows_gemm_chain_n"))) return rc;
  }
  if (og > 0) {  // (chain_typed_native: inside the rule)
    float* gf32 = at(2);
    if (gf32 && (rc = launch_bf16_widen(c.gf, pl.st.n[2], gf32, s))) return rc;
    float* g_in = reinterpret_cast<float*>(static_cast<char*>(c.ws) + pl.w.g_in.off);
    if ((rc = launch_fn_input(h, 2, ef32, oe, nf32, on, gf32, p->dg, c.R, g_in, s))) return rc;
    if ((rc = launch_chain_narrow_bf16(h, 2, p->graphfn, g_in, pl.sh.k0[2], nullptr, 0, nullptr, 0, c.gf_out, nullptr, c.R, s, "k_rows_gemm_chain_g"))) return rc;
  }
  return GNX_OK;
}

// One Chain forward call: validate and plan, the refusals that read nothing of the handle but its counts — NULL features, bf16 alignment — the
// layout, the workspace refusal, the plan's tables; then the plan's form.  A staged bf16 call widens into the workspace, runs the fp32 launches on
// the copies and rounds the outputs.
int32_t chain_fw_run(const ChainFwCall& c, bool narrow, bool train = false) {
  ChainFwPlan pl(c.h, c.p, c.R, c.elem, narrow, train);
  if (pl.rc) return pl.rc;
  if (train) pl.query = "workspace missing or smaller than gnx_chain_block_forward_train_workspace_bytes()";
  const hipStream_t s = (hipStream_t)c.stream;
  gnx::FormScope forms(c.flags);  // the forms this call selected (gnx.h: GNX_FLAG_EDGE_FP32 ...)
  gnx::DeviceTurn turn(s, !pl.native && pl.sh.wide);  // (any layer of any chain at matrix-core widths; the native path has none)
  int32_t rc;
  if ((rc = chain_check_features(pl.sh, c.ef, c.nf, c.gf, "an input with non-zero width is NULL (width 0 <=> nothing)"))) return rc;
  if ((pl.sh.ow[0] > 0 && !c.ef_out && c.h->E > 0) || (pl.sh.ow[1] > 0 && !c.nf_out) || (pl.sh.ow[2] > 0 && !c.gf_out)) return fail(GNX_ERR_INVALID_ARG, "an output with non-zero width is NULL");
  const void* bufs[6] = {c.ef, c.nf, c.gf, c.ef_out, c.nf_out, c.gf_out};
  if (pl.bf16 && (rc = check_bf16_aligned(bufs, 6))) return rc;
  pl.lay_out(c.h);
  if (!c.ws || c.ws_bytes < pl.total) return fail(GNX_ERR_WORKSPACE, pl.query);
  if (((uintptr_t)c.ws & 15) != 0) return fail(GNX_ERR_WORKSPACE, "workspace must be 16-byte aligned");
  if (pl.wide_tables() && (rc = gnx_ensure_wide_tables(c.h, s))) return rc;
  auto cf = [](const void* q) { return static_cast<const float*>(q); };
  if (!pl.bf16) return chain_forward_fp32(c, pl, cf(c.ef), cf(c.nf), cf(c.gf), static_cast<float*>(c.ef_out), static_cast<float*>(c.nf_out), static_cast<float*>(c.gf_out));
  if (pl.native) return chain_forward_native(c, pl);
  if ((rc = stage_widen(pl.st, c.ws, bufs, 0, 3, s))) return rc;
  auto at = [&](int i) { return pl.st.n[i] > 0 ? pl.st.at(c.ws, i) : nullptr; };
  if ((rc = chain_forward_fp32(c, pl, at(0), at(1), at(2), at(3), at(4), at(5)))) return rc;
  return stage_round(pl.st, c.ws, bufs, 3, 6, s);
}

// a _workspace_bytes entry: the plan's total, and the plan's tables built here, outside any capture (a failure resurfaces in the call)
size_t chain_fw_query(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t R, int32_t elem, bool narrow, bool train = false) {
  ChainFwPlan pl(h, p, R, elem, narrow, train);
  if (pl.rc) return 0;
  pl.lay_out(h);
  if (pl.wide_tables()) (void)gnx_ensure_wide_tables(h);
  return pl.total;
}

bool elem_ok(int32_t elem) { return elem == GNX_ELEM_F32 || elem == GNX_ELEM_BF16; }

}  // namespace

extern "C" {

// Every _workspace_bytes: the plan's total (and the plan's tables built).  Every _applies: the plan's mask, or its native flag.  Every call entry:
// the record, then chain_fw_run.
size_t gnx_chain_block_workspace_bytes(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t R) { return chain_fw_query(h, p, R, GNX_ELEM_F32, false); }

int32_t gnx_chain_block_forward(const gnx_graphs* h, const gnx_chain_block_params* p, const float* ef, const float* nf, const float* gf, int64_t R,
                                float* ef_out, float* nf_out, float* gf_out, void* ws, size_t ws_bytes, uint32_t flags, void* stream) {
  return chain_fw_run(ChainFwCall{h, p, GNX_ELEM_F32, ef, nf, gf, R, ef_out, nf_out, gf_out, ws, ws_bytes, flags, stream}, false);
}

int32_t gnx_chain_block_forward_narrow_applies(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t R) {
  return check_params(h, p, R) == GNX_OK ? (int32_t)chain_fused_mask(chain_shape(h->E, h->N, h->G, *p, R), CHAIN_RULE_FW) : 0;
}

size_t gnx_chain_block_forward_narrow_workspace_bytes(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t R) { return chain_fw_query(h, p, R, GNX_ELEM_F32, true); }

int32_t gnx_chain_block_forward_narrow(const gnx_graphs* h, const gnx_chain_block_params* p, const float* ef, const float* nf, const float* gf, int64_t R,
                                       float* ef_out, float* nf_out, float* gf_out, void* ws, size_t ws_bytes, uint32_t flags, void* stream) {
  return chain_fw_run(ChainFwCall{h, p, GNX_ELEM_F32, ef, nf, gf, R, ef_out, nf_out, gf_out, ws, ws_bytes, flags, stream}, true);
}

// gnx_chain_block_forward_typed: either entry above on fp32 or bf16 features (narrow selects which one the call mirrors)
int32_t gnx_chain_block_forward_typed_applies(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t R, int32_t elem, int32_t narrow) {
  return elem == GNX_ELEM_BF16 && narrow == 1 && ChainFwPlan(h, p, R, elem, true).native ? 1 : 0;  // (the constructor reads the handle's counts alone)
}

size_t gnx_chain_block_forward_typed_workspace_bytes(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t R, int32_t elem, int32_t narrow) {
  return elem_ok(elem) && (narrow == 0 || narrow == 1) ? chain_fw_query(h, p, R, elem, narrow != 0) : 0;
}

int32_t gnx_chain_block_forward_typed(const gnx_graphs* h, const gnx_chain_block_params* p, int32_t elem, const void* ef, const void* nf, const void* gf, int64_t R,
                                      void* ef_out, void* nf_out, void* gf_out, void* ws, size_t ws_bytes, int32_t narrow, uint32_t flags, void* stream) {
  if (!elem_ok(elem)) return fail(GNX_ERR_INVALID_ARG, "elem must be GNX_ELEM_F32 or GNX_ELEM_BF16");
  if (narrow != 0 && narrow != 1) return fail(GNX_ERR_INVALID_ARG, "narrow must be 0 or 1");
  return chain_fw_run(ChainFwCall{h, p, elem, ef, nf, gf, R, ef_out, nf_out, gf_out, ws, ws_bytes, flags, stream}, narrow != 0);
}

// ---- training mode: Dropout entries inside the chains (include/gnx.h; ChainTrain, gnx_staging.h) ----
int32_t gnx_chain_dropout_mask(const gnx_chain_dropout* d, int32_t function, int32_t layer, float p, int64_t n, float* out, void* stream) {
  if (!d || (!out && n > 0) || n < 0) return fail(GNX_ERR_INVALID_ARG, "gnx_chain_dropout_mask: NULL argument or negative length");
  if (function < 0 || function > 2 || layer < 0 || layer >= kChainMaxLayers) return fail(GNX_ERR_INVALID_ARG, "gnx_chain_dropout_mask: function outside 0..2 or layer outside 0..15");
  if (!(p >= 0.f && p <= 1.f)) return fail(GNX_ERR_INVALID_ARG, "Dropout: p must lie in [0, 1] (Flux.Dropout asserts 0 <= p <= 1)");
  if (n == 0) return GNX_OK;
  return launch_dropout(gnx_dropout{p, 0, d->seed}, 16 + 16 * function + layer, (size_t)n, nullptr, out, 0, (hipStream_t)stream);
}

// the mask of the training rule with every Dropout entry active (the plan header's two rules read the entries)
int32_t gnx_chain_block_train_applies(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t R, int32_t backward) {
  if (!h || (backward != 0 && backward != 1)) return 0;
  ChainTrain tr(p, nullptr, true);
  if (tr.rc || check_params(h, &tr.p, R, true) != GNX_OK) return 0;
  const ChainShape sh = chain_shape(h->E, h->N, h->G, tr.p, R);
  if (backward && sh.ow[0] == 0) return 0;  // (no pullback without an edge output)
  return (int32_t)chain_fused_mask(sh, backward ? CHAIN_RULE_BW : CHAIN_RULE_FW);
}

// The query sees no record: what a call with every entry active needs, and no less than the mirrored entry on the stripped chains.
size_t gnx_chain_block_forward_train_workspace_bytes(const gnx_graphs* h, const gnx_chain_block_params* p, int64_t R, int32_t narrow) {
  if (!h || (narrow != 0 && narrow != 1)) return 0;
  ChainTrain all(p, nullptr, true), none(p, nullptr);
  if (all.rc || none.rc) return 0;
  const size_t a = chain_fw_query(h, &all.p, R, GNX_ELEM_F32, narrow != 0, all.active), b = chain_fw_query(h, &none.p, R, GNX_ELEM_F32, narrow != 0);
  return a && b ? std::max(a, b) : 0;
}

int32_t gnx_chain_block_forward_train(const gnx_graphs* h, const gnx_chain_block_params* p, const gnx_chain_dropout* dropout, const float* ef, const float* nf,
                                      const float* gf, int64_t R, float* ef_out, float* nf_out, float* gf_out, void* ws, size_t ws_bytes, int32_t narrow,
                                      uint32_t flags, void* stream) {
  if (!h || !p) return fail(GNX_ERR_INVALID_ARG, "NULL handle or params");
  ChainTrain tr(p, dropout);
  if (tr.rc) return tr.rc;
  if (narrow != 0 && narrow != 1) return fail(GNX_ERR_INVALID_ARG, "narrow must be 0 or 1");
  return chain_fw_run(ChainFwCall{h, &tr.p, GNX_ELEM_F32, ef, nf, gf, R, ef_out, nf_out, gf_out, ws, ws_bytes, flags, stream}, narrow != 0, tr.active);
}

}  // extern "C"
