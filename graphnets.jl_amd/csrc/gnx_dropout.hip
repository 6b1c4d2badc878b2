// Training-mode Dropout of a GNCore's FeedForwards.
//
// The reference's FeedForward is Chain(Dense(d => 4d, relu), Dense(4d => d), Dropout(p)) (src/gnfeedforward.jl:27-31): in training mode
// (inside a gradient call) Flux multiplies the FeedForward's OUTPUT element-wise by a fresh mask, m = rand > p ? 1 / (1 - p) : 0; in test
// mode the layer is the identity, which is what gnx_core_forward computes.  (GNBlock keeps a Dropout(p) field that its forward never applies:
// src/gnblock.jl:63-69.)  A core in training mode is therefore
//     y = x + block(gn1(x)) + m .* ffwd(gn2(x))                                                              (src/gncore.jl:56-59)
// The masks are not stored: element i of entity t's mask is a pure function of (seed, t, i) — Philox-4x32-10 keyed by the seed, counter
// (i / 4, t) — so the backward pass regenerates the forward's mask from the same gnx_dropout value, and a host can ask for it
// (gnx_dropout_mask) to check either pass against its own arithmetic.  Flux's mask comes from the array's own random-number generator; no
// implementation on another device reproduces those bits, so parity here is the FORM (independent per element, keep probability 1 - p, scale
// 1 / (1 - p), the same mask in both passes), tested against float64 with the library's mask handed to the oracle.
//
// gnx_core_forward_train = gnx_core_forward (every fused form as it is) followed by a correction y += (m - 1) .* f with f = ffwd(gn2(x))
// recomputed unfused into the workspace (LayerNorm launch + two row-wise Dense launches per entity) — the training step's backward recomputes
// the same intermediates anyway, and the inference kernels stay free of a mask operand.
#include <algorithm>

#include "gnx_launchers.h"
#include "gnx_philox.h"  // philox4 / mask_of: shared with k_core_post_train (gnx_core_train_narrow.hip)
#include "gnx_staging.h"
#include "gnx_wave_kernel.h"  // pack_bf16 / to_bf16

namespace gnx {

namespace {
// MODE 0: out = m;  1: out = in .* m;  2: out += (m - 1) .* in.  One thread per four consecutive elements (one Philox block).
template <int MODE>
__global__ __launch_bounds__(256) void k_dropout(const float* __restrict__ in, float* __restrict__ out, size_t n, float p, float scale, uint64_t seed,
                                                 uint32_t entity, int vec) {
  const size_t quad = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t i0 = quad * 4;
  if (i0 >= n) return;
  uint32_t r[4];
  philox4(quad, entity, seed, r);
  float m[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) m[j] = mask_of(r[j], p, scale);
  if (vec && i0 + 4 <= n) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), o = a;
    if (MODE != 0) a = *reinterpret_cast<const float4*>(in + i0);
    if (MODE == 2) o = *reinterpret_cast<const float4*>(out + i0);
    if (MODE == 0) o = make_float4(m[0], m[1], m[2], m[3]);
    else if (MODE == 1) o = make_float4(a.x * m[0], a.y * m[1], a.z * m[2], a.w * m[3]);
    else o = make_float4(fmaf(m[0] - 1.f, a.x, o.x), fmaf(m[1] - 1.f, a.y, o.y), fmaf(m[2] - 1.f, a.z, o.z), fmaf(m[3] - 1.f, a.w, o.w));
    *reinterpret_cast<float4*>(out + i0) = o;
    return;
  }
  for (int j = 0; j < 4 && i0 + j < n; ++j) {
    if (MODE == 0) out[i0 + j] = m[j];
    else if (MODE == 1) out[i0 + j] = in[i0 + j] * m[j];
    else out[i0 + j] = fmaf(m[j] - 1.f, in[i0 + j], out[i0 + j]);
  }
}

// The bf16-storing form of MODE 2 (gnx_core_forward_train_typed off the fused path): out = to_bf16(fmaf(m - 1, f, y)) with y the fp32 core's
// output — the correction and the one rounding of its result in one pass, so no value is rounded twice.  f, y: 16-B aligned fp32; out: 4-B
// aligned bf16 (a quad starts at byte 8 * quad: two dwords); a partial last quad is stored element by element.
__global__ __launch_bounds__(256) void k_dropout_bf16(const float* __restrict__ f, const float* __restrict__ y, bf16_t* __restrict__ out, size_t n, float p,
                                                      float scale, uint64_t seed, uint32_t entity) {
  const size_t quad = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t i0 = quad * 4;
  if (i0 >= n) return;
  uint32_t r[4];
  philox4(quad, entity, seed, r);
  float m[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) m[j] = mask_of(r[j], p, scale);
  if (i0 + 4 <= n) {
    const float4 a = *reinterpret_cast<const float4*>(f + i0), o = *reinterpret_cast<const float4*>(y + i0);
    U2u v;
    v.x = pack_bf16(fmaf(m[0] - 1.f, a.x, o.x), fmaf(m[1] - 1.f, a.y, o.y));
    v.y = pack_bf16(fmaf(m[2] - 1.f, a.z, o.z), fmaf(m[3] - 1.f, a.w, o.w));
    *reinterpret_cast<U2u*>(out + i0) = v;
    return;
  }
  for (int j = 0; j < 4 && i0 + j < n; ++j) out[i0 + j] = to_bf16(fmaf(m[j] - 1.f, f[i0 + j], y[i0 + j]));
}
}  // namespace

bool dropout_active(const gnx_dropout* d) { return d && d->p > 0.f; }

int32_t check_dropout(const gnx_dropout* d) {
  if (d && !(d->p >= 0.f && d->p <= 1.f)) return fail(GNX_ERR_INVALID_ARG, "Dropout: p must lie in [0, 1] (Flux.Dropout asserts 0 <= p <= 1)");
  return GNX_OK;
}

// mode as k_dropout's MODE; `in` unused for mode 0
int32_t launch_dropout(const gnx_dropout& d, int entity, size_t n, const float* in, float* out, int mode, hipStream_t s) {
  if (n == 0) return GNX_OK;
  const float scale = d.p < 1.f ? 1.f / (1.f - d.p) : 0.f;
  const int vec = (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
  const dim3 grid((unsigned)(((n + 3) / 4 + 255) / 256));
  ProfScope ps("k_dropout", s);
  if (mode == 0) GNX_LAUNCH(k_dropout<0>, grid, dim3(256), 0, s, in, out, n, d.p, scale, d.seed, (uint32_t)entity, vec);
  else if (mode == 1) GNX_LAUNCH(k_dropout<1>, grid, dim3(256), 0, s, in, out, n, d.p, scale, d.seed, (uint32_t)entity, vec);
  else GNX_LAUNCH(k_dropout<2>, grid, dim3(256), 0, s, in, out, n, d.p, scale, d.seed, (uint32_t)entity, vec);
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

// out = to_bf16(y + (m - 1) .* f) (k_dropout_bf16)
static int32_t launch_dropout_bf16(const gnx_dropout& d, int entity, size_t n, const float* f, const float* y, void* out, hipStream_t s) {
  if (n == 0) return GNX_OK;
  const float scale = d.p < 1.f ? 1.f / (1.f - d.p) : 0.f;
  const dim3 grid((unsigned)(((n + 3) / 4 + 255) / 256));
  ProfScope ps("k_dropout", s);
  GNX_LAUNCH(k_dropout_bf16, grid, dim3(256), 0, s, f, y, static_cast<bf16_t*>(out), n, d.p, scale, d.seed, (uint32_t)entity);
  GNX_HIP(hipGetLastError());
  return GNX_OK;
}

namespace {
struct TrainLayout { size_t core, l1, l2, hid, f, total; };
TrainLayout train_layout(const gnx_graphs* h, const gnx_core_params* p, int64_t R, size_t core_bytes) {
  const size_t rows[3] = {(size_t)R * h->E, (size_t)R * h->N, (size_t)R * h->G};
  const int d[3] = {p->block.de, p->block.dn, p->block.dg};
  size_t bmax = 0;
  for (int t = 0; t < 3; ++t) bmax = std::max(bmax, sizeof(float) * rows[t] * (size_t)std::max(d[t], 0));
  TrainLayout L{};
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += align_up(bytes, 256); return at; };
  L.core = take(core_bytes);
  L.l1 = take(bmax); L.l2 = take(bmax); L.hid = take(4 * bmax); L.f = take(bmax);
  L.total = o + 256;
  return L;
}

// The correction of a training forward after gnx_core_forward wrote y32 = x + block + f_fused: f = ffwd(gn2(x)) recomputed unfused into the
// workspace, then y32 += (m - 1) .* f in place — or, with ybf, to_bf16(y32 + (m - 1) .* f) into ybf[t] (bf16 rows), y32 left as it is.
int32_t train_correct(const gnx_graphs* h, const gnx_core_params* p, const gnx_dropout& dr, int64_t R, const float* const x[3], float* const y32[3],
                      void* const* ybf, char* base, const TrainLayout& L, hipStream_t s) {
  auto F = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  const size_t rows[3] = {(size_t)R * h->E, (size_t)R * h->N, (size_t)R * h->G};
  const int d[3] = {p->block.de, p->block.dn, p->block.dg};
  int32_t rc;
  for (int t = 0; t < 3; ++t) {
    if (rows[t] == 0) continue;
    if ((rc = launch_layernorm2(x[t], rows[t], d[t], p->ln1[t], p->ln2[t], p->eps, p->eps_mode, F(L.l1), F(L.l2), s))) return rc;
    if ((rc = launch_dense_rows(h, t, F(L.l2), d[t], p->ff[t].fc1, 4 * d[t], nullptr, nullptr, F(L.hid), R, s, "train_ff1"))) return rc;
    if ((rc = launch_dense_rows(h, t, F(L.hid), 4 * d[t], p->ff[t].fc2, d[t], nullptr, nullptr, F(L.f), R, s, "train_ff2"))) return rc;
    if (ybf) rc = launch_dropout_bf16(dr, t, rows[t] * (size_t)d[t], F(L.f), y32[t], ybf[t], s);
    else rc = launch_dropout(dr, t, rows[t] * (size_t)d[t], F(L.f), y32[t], 2, s);
    if (rc) return rc;
  }
  return GNX_OK;
}

// ---- gnx_core_forward_train_typed ----
// FUSED (gnx_core_train_fused_applies): gn1(x) and block(gn1(x)) per entity in fp32, the block's own workspace; nothing else — no copy of a
// bf16 tensor, no hidden units, no f.
struct FusedLayout { size_t l1[3], bout[3], blk, blk_bytes, total; };
FusedLayout fused_layout(const gnx_graphs* h, const gnx_core_params* p, int64_t R) {
  const size_t rows[3] = {(size_t)R * h->E, (size_t)R * h->N, (size_t)R * h->G};
  const int d[3] = {p->block.de, p->block.dn, p->block.dg};
  FusedLayout L{};
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += align_up(bytes, 256); return at; };
  for (int t = 0; t < 3; ++t) L.l1[t] = take(sizeof(float) * rows[t] * (size_t)d[t]);
  for (int t = 0; t < 3; ++t) L.bout[t] = take(sizeof(float) * rows[t] * (size_t)d[t]);
  L.blk_bytes = gnx_block_workspace_bytes(h, &p->block, R);
  L.blk = take(L.blk_bytes);
  L.total = o + 256;
  return L;
}
// bf16 off the fused path: behind train_layout, fp32 copies of the three inputs (0..2) and the fp32 core's three outputs (3..5)
Staging train_bf16_staging(const gnx_graphs* h, const gnx_core_params* p, int64_t R, size_t train_total) {
  const int d[6] = {p->block.de, p->block.dn, p->block.dg, p->block.de, p->block.dn, p->block.dg};
  return stage_features(train_total, h, R, d, 6);
}
}  // namespace
}  // namespace gnx

using namespace gnx;

extern "C" {

int32_t gnx_dropout_mask(const gnx_dropout* d, int32_t entity, int64_t n, float* out, void* stream) {
  if (!d || (!out && n > 0) || n < 0 || entity < 0 || entity > 2) return fail(GNX_ERR_INVALID_ARG, "gnx_dropout_mask: NULL argument, negative length or entity outside 0..2");
  if (int32_t rc = check_dropout(d)) return rc;
  if (n == 0) return GNX_OK;  // (the mask of an entity without rows: a batch without edges)
  return launch_dropout(*d, entity, (size_t)n, nullptr, out, 0, (hipStream_t)stream);
}

size_t gnx_core_train_workspace_bytes(const gnx_graphs* h, const gnx_core_params* p, int64_t R) {
  if (!h || !p || R <= 0) return 0;
  const size_t core = gnx_core_workspace_bytes(h, p, R);
  if (core == 0) return 0;
  (void)gnx_ensure_wide_tables(h);  // the unfused FeedForward runs on the row-wise Dense launcher
  return train_layout(h, p, R, core).total;
}

int32_t gnx_core_forward_train(const gnx_graphs* h, const gnx_core_params* p, const gnx_dropout* dr, const float* ef, const float* nf, const float* gf,
                               int64_t R, float* ef_out, float* nf_out, float* gf_out, void* ws, size_t ws_bytes, uint32_t flags, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!h || !p) return fail(GNX_ERR_INVALID_ARG, "NULL handle or params");
  if (int32_t rc = check_dropout(dr)) return rc;
  const size_t core = gnx_core_workspace_bytes(h, p, R);
  if (core == 0) return fail(GNX_ERR_DIMS, "gnx_core_forward_train: gnx_core_workspace_bytes rejects these parameters (GNCore needs dims => dims, all(dims .> 0), n_replicas >= 1)");
  const TrainLayout L = train_layout(h, p, R, core);
  if (!ws || ws_bytes < (dropout_active(dr) ? L.total : core)) return fail(GNX_ERR_WORKSPACE, "workspace missing or smaller than gnx_core_train_workspace_bytes()");
  if (((uintptr_t)ws & 15) != 0) return fail(GNX_ERR_WORKSPACE, "workspace must be 16-byte aligned");
  char* base = static_cast<char*>(ws);
  // (everything that can refuse the call is checked BEFORE the forward writes an output — a refused call leaves the outputs alone)
  if (dropout_active(dr))
    for (int t = 0; t < 3; ++t)
      if (p->ff[t].fc2.act != GNX_ACT_IDENTITY) return fail(GNX_ERR_INVALID_ARG, "core training forward: fc2 must be identity");
  DeviceTurn turn(s, matrix_core_widths(p->block));
  int32_t rc = gnx_core_forward(h, p, ef, nf, gf, R, ef_out, nf_out, gf_out, base + L.core, core, flags, stream);
  if (rc || !dropout_active(dr)) return rc;
  FormScope forms(flags);
  PreparedScope prepared(p->prepared);  // (the recompute below runs the row-wise Dense launcher: no planes are looked up today, and none is missed if that changes)
  const float* const x[3] = {ef, nf, gf};
  float* const y[3] = {ef_out, nf_out, gf_out};
  return train_correct(h, p, *dr, R, x, y, nullptr, base, L, s);
}

int32_t gnx_core_train_fused_applies(const gnx_graphs* h, const gnx_core_params* p, int64_t R, int32_t elem) {
  return gnx_core_backward_narrow_applies(h, p, R, elem);  // the one rule of both narrow training kernels (CoreBwPlan::narrow, gnx_backward.hip)
}

size_t gnx_core_train_typed_workspace_bytes(const gnx_graphs* h, const gnx_core_params* p, int64_t R, int32_t elem, uint32_t flags) {
  if (!h || !p || R <= 0 || (elem != GNX_ELEM_F32 && elem != GNX_ELEM_BF16) || (flags & GNX_FLAG_DEFER_GRAPH_UPDATE)) return 0;
  if (gnx_core_train_fused_applies(h, p, R, elem)) return fused_layout(h, p, R).total;  // (gnx_block_workspace_bytes inside: whatever the block needs is built here)
  const size_t train = gnx_core_train_workspace_bytes(h, p, R);
  if (elem == GNX_ELEM_F32 || train == 0) return train;
  return train_bf16_staging(h, p, R, train).total;
}

int32_t gnx_core_forward_train_typed(const gnx_graphs* h, const gnx_core_params* p, int32_t elem, const gnx_dropout* dr, const void* ef, const void* nf,
                                     const void* gf, int64_t R, void* ef_out, void* nf_out, void* gf_out, void* ws, size_t ws_bytes, uint32_t flags,
                                     void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (elem != GNX_ELEM_F32 && elem != GNX_ELEM_BF16) return fail(GNX_ERR_INVALID_ARG, "elem must be GNX_ELEM_F32 or GNX_ELEM_BF16");
  int32_t rc = check_dropout(dr);
  if (rc) return rc;
  if (!dropout_active(dr)) return gnx_core_forward_typed(h, p, elem, ef, nf, gf, R, ef_out, nf_out, gf_out, ws, ws_bytes, flags, stream);
  const bool bf16 = elem == GNX_ELEM_BF16;
  const void* bufs[6] = {ef, nf, gf, ef_out, nf_out, gf_out};
  if (bf16 && (rc = check_bf16_aligned(bufs, 6))) return rc;
  if (flags & GNX_FLAG_DEFER_GRAPH_UPDATE) return fail(GNX_ERR_INVALID_ARG, "GNX_FLAG_DEFER_GRAPH_UPDATE is not supported with an active Dropout");
  if (!p) return fail(GNX_ERR_INVALID_ARG, "NULL handle or params");
  if ((rc = core_forward_check_dims(p))) return rc;
  if (!h) return fail(GNX_ERR_INVALID_ARG, "NULL handle or params");
  const bool fused = gnx_core_train_fused_applies(h, p, R, elem) != 0;
  if (!fused && !bf16)
    return gnx_core_forward_train(h, p, dr, static_cast<const float*>(ef), static_cast<const float*>(nf), static_cast<const float*>(gf), R,
                                  static_cast<float*>(ef_out), static_cast<float*>(nf_out), static_cast<float*>(gf_out), ws, ws_bytes, flags, stream);
  FormScope forms(flags);
  if ((rc = core_forward_check(h, p, R, ef, nf, gf, ef_out, nf_out, gf_out, flags))) return rc;
  for (int t = 0; t < 3; ++t)
    if (p->ff[t].fc2.act != GNX_ACT_IDENTITY) return fail(GNX_ERR_INVALID_ARG, "core training forward: fc2 must be identity");
  const size_t rows[3] = {(size_t)R * h->E, (size_t)R * h->N, (size_t)R * h->G};
  const int d[3] = {p->block.de, p->block.dn, p->block.dg};
  char* base = static_cast<char*>(ws);
  auto F = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  if (fused) {
    const FusedLayout L = fused_layout(h, p, R);
    if ((rc = check_ws(ws, ws_bytes, L.total, "workspace missing or smaller than gnx_core_train_typed_workspace_bytes()"))) return rc;
    // gn1(x) per entity, the block on those rows (step 1 of the core backward), then the FeedForward + Dropout + residuals in one launch per entity
    for (int t = 0; t < 3; ++t)
      if ((rc = bf16 ? launch_ln1_rows_bf16(bufs[t], rows[t], d[t], p->ln1[t], p->eps, p->eps_mode, F(L.l1[t]), s)
                     : launch_ln1_rows(static_cast<const float*>(bufs[t]), rows[t], d[t], p->ln1[t], p->eps, p->eps_mode, F(L.l1[t]), s))) return rc;
    if ((rc = gnx_block_forward(h, &p->block, F(L.l1[0]), F(L.l1[1]), F(L.l1[2]), R, F(L.bout[0]), F(L.bout[1]), F(L.bout[2]), base + L.blk, L.blk_bytes, flags,
                                stream))) return rc;
    for (int t = 0; t < 3; ++t)
      if ((rc = launch_core_post_train(bufs[t], rows[t], d[t], p->ln2[t], p->ff[t], p->eps, p->eps_mode, F(L.bout[t]), *dr, t, const_cast<void*>(bufs[3 + t]), bf16,
                                       s))) return rc;
    return GNX_OK;
  }
  // bf16 off the fused path: gnx_core_forward_train's launches on fp32 copies, its last pass storing bf16 (the native bf16 forward's outputs
  // are rounded already: not used here)
  const size_t core = gnx_core_workspace_bytes(h, p, R);
  if (core == 0) return fail(GNX_ERR_DIMS, "gnx_core_forward_train_typed: gnx_core_workspace_bytes rejects these parameters");
  const TrainLayout L = train_layout(h, p, R, core);
  const Staging w = train_bf16_staging(h, p, R, L.total);
  if ((rc = check_ws(ws, ws_bytes, w.total, "workspace missing or smaller than gnx_core_train_typed_workspace_bytes()"))) return rc;
  if ((rc = stage_widen(w, ws, bufs, 0, 3, s))) return rc;
  const float* const x[3] = {w.n[0] ? w.at(ws, 0) : nullptr, w.at(ws, 1), w.at(ws, 2)};  // (a batch without edges: NULL, as for the fp32 core)
  float* const y32[3] = {w.n[3] ? w.at(ws, 3) : nullptr, w.at(ws, 4), w.at(ws, 5)};
  DeviceTurn turn(s, matrix_core_widths(p->block));
  if ((rc = gnx_core_forward(h, p, x[0], x[1], x[2], R, y32[0], y32[1], y32[2], base + L.core, core, flags, stream))) return rc;
  PreparedScope prepared(p->prepared);
  return train_correct(h, p, *dr, R, x, y32, const_cast<void* const*>(bufs + 3), base, L, s);
}

}  // extern "C"
