// C-ABI entry points of the forward path: argument validation (mirroring the reference's assertions), workspace
// carving and kernel-path selection.  No allocation and no synchronisation happens here, so every call is
// asynchronous on the caller's stream and can be captured into a hipGraph.
#include <algorithm>
#include <cstdlib>

#include "gnx_staging.h"
#include "gnx_step_hazard.h"

namespace gnx {

static_assert(GNX_ACT_IDENTITY == 0 && GNX_ACT_RELU == 1 && GNX_ACT_TANH == 2 && GNX_ACT_SIGMOID == 3 && GNX_ACT_GELU == 4,
              "act_apply (gnx_device.h) hard-codes the activation codes");

static int32_t check_block(const gnx_graphs* h, const gnx_block_params* p, int64_t R) {
  if (!h || !p) return fail(GNX_ERR_INVALID_ARG, "NULL handle or params");
  if (R <= 0) return fail(GNX_ERR_INVALID_ARG, "n_replicas must be >= 1");
  if (R > 1 && h->G != 1)
    return fail(GNX_ERR_INVALID_ARG, "n_replicas > 1 needs a single-graph handle (shared adjacency, batch.jl:66)");
  if (R > 65535) return fail(GNX_ERR_TOO_LARGE, "n_replicas exceeds the grid limit (65535)");
  const int d[6] = {p->de, p->dn, p->dg, p->oe, p->on, p->og};
  for (int i = 0; i < 6; ++i)
    if (d[i] < 0) return fail(GNX_ERR_DIMS, "negative feature width");
  if (p->de + p->dn + p->dg == 0) return fail(GNX_ERR_DIMS, "all input widths are 0 (gnblock.jl:48, batch.jl:56)");
  if (p->oe + p->on + p->og == 0) return fail(GNX_ERR_DIMS, "all output widths are 0 (gnblock.jl:49)");
  const gnx_dense* fn[3] = {&p->edgefn, &p->nodefn, &p->graphfn};
  const int out[3] = {p->oe, p->on, p->og};
  const int in[3] = {p->de + 2 * p->dn + p->dg, p->oe + p->dn + p->dg, p->oe + p->on + p->dg};
  for (int i = 0; i < 3; ++i) {
    if (out[i] > 0 && in[i] > 0 && !fn[i]->weight) return fail(GNX_ERR_INVALID_ARG, "Dense weight is NULL");
    if (fn[i]->act < GNX_ACT_IDENTITY || fn[i]->act > GNX_ACT_GELU) return fail(GNX_ERR_INVALID_ARG, "unknown activation");
  }
  return GNX_OK;
}

struct BlockWs {
  size_t agg_off, part_off, total;
};

static BlockWs block_ws(const gnx_graphs* h, const gnx_block_params* p, int64_t R) {
  BlockWs w;
  w.agg_off = 0;
  const size_t agg = align_up(sizeof(float) * (size_t)R * h->N * p->oe, 256);
  w.part_off = w.agg_off + agg;
  // partial-sum rows: generic path [n_tiles][C]; fused narrow path [n_wtiles (or workgroups)][4*ceil(C/4)]
  const size_t C = (size_t)(p->oe + p->on);
  const size_t rows_bytes = std::max((size_t)h->n_tiles() * C, (size_t)h->n_wtiles() * ((C + 3) / 4 * 4));
  const size_t wide_part = wide_workspace_bytes(h, p, R);
  const size_t part = align_up(std::max(sizeof(float) * (size_t)R * rows_bytes, wide_part), 256);
  w.total = w.part_off + part + 256;
  return w;
}

// ---- one block forward: the call record, its validation, and one function per FORM of the forward ----
// What an entry point asks of the block kernels.  Every form below takes the record plus only what that form needs.
struct BlockCall {
  const gnx_graphs* h;
  const gnx_block_params* p;
  int32_t elem;  // GNX_ELEM_F32 / GNX_ELEM_BF16: what the six feature pointers point to
  const void *ef, *nf, *gf;
  int64_t R;
  void *ef_out, *nf_out, *gf_out;
  void* ws;
  size_t ws_bytes;
  uint32_t flags;
  hipStream_t s;
  int phase;  // GNX_PHASE_* (gnx_internal.h)
  // the same call on another stream and phase / on other inputs
  BlockCall on(hipStream_t stream, int ph) const { BlockCall c = *this; c.s = stream; c.phase = ph; return c; }
  BlockCall with(const void* e, const void* n, const void* g) const { BlockCall c = *this; c.ef = e; c.nf = n; c.gf = g; return c; }
};

// check_block, then the buffers the call's phases read and write
static int32_t check_call(const BlockCall& c) {
  if (const int32_t rc = check_block(c.h, c.p, c.R)) return rc;
  const gnx_graphs* h = c.h;
  const gnx_block_params* p = c.p;
  if (c.phase & GNX_PHASE_EDGE_NODE) {
    // a batch without a single edge has (DE, 0) edge features: its (empty) buffers may be NULL
    if ((p->de > 0 && !c.ef && h->E > 0) || (p->dn > 0 && !c.nf) || (p->dg > 0 && !c.gf))
      return fail(GNX_ERR_INVALID_ARG, "an input with non-zero width is NULL (width 0 <=> nothing)");
    // (a whole bf16 call counts gf_out among the outputs: the wording of the bf16 entry points, which refuse everything before a launch)
    const bool typed_whole = c.elem == GNX_ELEM_BF16 && (c.phase & GNX_PHASE_GRAPH);
    if ((p->oe > 0 && !c.ef_out && h->E > 0) || (p->on > 0 && !c.nf_out) || (typed_whole && p->og > 0 && !c.gf_out))
      return fail(GNX_ERR_INVALID_ARG, "an output with non-zero width is NULL");
  }
  if ((c.phase & GNX_PHASE_GRAPH) && ((p->dg > 0 && !c.gf) || (p->og > 0 && !c.gf_out))) return fail(GNX_ERR_INVALID_ARG, "gf / gf_out is NULL");
  return GNX_OK;
}

// A validated call — the ONE place that validates a call and fills the kernels' argument block: the scopes every form opens first (the forms
// this call selected, gnx.h: GNX_FLAG_FFN_FP32 ..., for every dispatch predicate; the layer's prepared weight planes, if the caller made them —
// a core passes its own through its block), then rc == GNX_OK and the arguments + workspace carve, or the error.
struct Prepared {
  FormScope forms;
  PreparedScope planes;
  BlockArgs a;
  BlockWs w;
  int32_t rc;
  explicit Prepared(const BlockCall& c) : forms(c.flags), planes(c.p ? c.p->prepared : nullptr), rc(fill(c)) {}
  int32_t fill(const BlockCall& c) {
    const gnx_graphs* h = c.h;
    const gnx_block_params* p = c.p;
    if (const int32_t bad = check_call(c)) return bad;
    w = block_ws(h, p, c.R);
    if (const int32_t bad = check_ws(c.ws, c.ws_bytes, w.total, "workspace missing or smaller than gnx_block_workspace_bytes()")) return bad;
    a = block_probe(h, p);
    a.We = p->edgefn.weight; a.be = p->edgefn.bias; a.act_e = p->edgefn.act;
    a.Wn = p->nodefn.weight; a.bn = p->nodefn.bias; a.act_n = p->nodefn.act;
    a.Wg = p->graphfn.weight; a.bg = p->graphfn.bias; a.act_g = p->graphfn.act;
    // (bf16 rows travel in the float* fields: only the native bf16 kernels read them, as what they are)
    a.ef = p->de ? static_cast<const float*>(c.ef) : nullptr; a.nf = p->dn ? static_cast<const float*>(c.nf) : nullptr; a.gf = p->dg ? static_cast<const float*>(c.gf) : nullptr;
    a.ef_out = static_cast<float*>(c.ef_out); a.nf_out = static_cast<float*>(c.nf_out); a.gf_out = static_cast<float*>(c.gf_out);
    a.agg = reinterpret_cast<float*>(static_cast<char*>(c.ws) + w.agg_off);
    a.partials = reinterpret_cast<float*>(static_cast<char*>(c.ws) + w.part_off);
    a.colptr = h->d_colptr; a.rowval = h->d_rowval; a.node_off = h->d_node_off; a.edge_off = h->d_edge_off;
    a.tile_off = h->d_tile_off; a.tiles = h->d_tiles;
    a.wtile_off = h->d_wtile_off; a.wtiles = h->d_wtiles; a.n_tiles = (int)h->n_tiles();
    a.packs = h->d_packs; a.n_packs = h->n_packs;
    return GNX_OK;
  }
};

// The plain GNBlock.  fp32 rows: the fused narrow kernel, else the matrix-core kernels, else the generic ones.  bf16 rows: only the fused
// kernels read them natively (the caller checked that one takes these widths: typed_native).
static int32_t block_plain(const BlockCall& c) {
  Prepared q(c);
  if (q.rc) return q.rc;
  if (c.elem == GNX_ELEM_BF16) {
    const int32_t rc = launch_block_narrow(c.h, q.a, c.R, c.s, c.phase, true);
    return rc == 1 ? fail(GNX_ERR_INVALID_ARG, "internal: no fused bf16 kernel for these widths") : rc;
  }
  if (!(c.flags & GNX_FLAG_FORCE_GENERIC)) {
    int32_t rc = launch_block_narrow(c.h, q.a, c.R, c.s, c.phase);  // fused wave-per-tile kernel: ahead-of-time width sets, else specialised at run time
    if (rc != 1) return rc;
    if (!(c.flags & GNX_FLAG_NO_MFMA)) {
      rc = launch_block_wide(c.h, q.a, c.R, c.s, c.phase);  // fp32 MFMA gathered-row GEMMs
      if (rc != 1) return rc;
    }
  }
  return launch_block_generic(q.a, c.R, c.h->tile_n_cap, c.s, c.phase);
}

// The chained step: this call's edge + node update with the previous call's graph update (`prev`, may be NULL) at the front of the launch.
// took == false: these widths do not chain and nothing was launched — the caller runs the plain form.
static int32_t block_chained(const BlockCall& c, const gnx_pending_update* prev, bool& took) {
  took = false;
  Prepared q(c);
  if (q.rc) return q.rc;
  const bool bf16 = c.elem == GNX_ELEM_BF16;
  took = !(c.flags & GNX_FLAG_FORCE_GENERIC) && block_narrow_chain_applies(c.h, q.a, bf16);
  if (!took) return GNX_OK;
  if (prev && prev->workspace) {
    q.a.prev_partials = reinterpret_cast<const float*>(static_cast<const char*>(prev->workspace) + q.w.part_off);
    q.a.prev_gf = prev->gf; q.a.prev_gf_out = prev->gf_out;
  }
  return launch_block_narrow_chained(c.h, q.a, c.R, c.s, bf16);
}

// the edge FeedForward of a GNCore inside the block's edge launch: ef_out then receives the CORE's edge output
static void set_edge_ffn(BlockArgs& a, const gnx_ffn& ff, const gnx_layernorm& ln2) {
  a.ffe_w1 = ff.fc1.weight; a.ffe_b1 = ff.fc1.bias; a.ffe_w2 = ff.fc2.weight; a.ffe_b2 = ff.fc2.bias;
  a.ffe_g2 = ln2.gamma; a.ffe_be2 = ln2.beta; a.ffe_act1 = ff.fc1.act; a.ffe_act2 = ff.fc2.act;
}

// Narrow GNCore: the fused narrow kernel applies LayerNorm ln1 (3 entries) to its inputs as it loads them.  took == false: that kernel is not
// available for these widths, nothing was launched and the caller normalises itself.  `ffe` (may be NULL: not offered) + ffe_ln2: the edge
// FeedForward and both residual terms run in the block kernel's edge lanes when they can (ffe_took).
struct NarrowLnResult {
  bool took = false, ffe_took = false;
  BlockArgs args{};  // took: the block's arguments as launched (k_core_post3 finishes a deferred graph update from them)
};
static int32_t block_narrow_ln(const BlockCall& c, const gnx_layernorm* ln1, float ln_eps, int ln_mode, const gnx_ffn* ffe, const gnx_layernorm& ffe_ln2,
                               NarrowLnResult& r) {
  r.took = r.ffe_took = false;
  Prepared q(c);
  if (q.rc || (c.flags & GNX_FLAG_FORCE_GENERIC)) return q.rc;
  BlockArgs& a = q.a;
  for (int t = 0; t < 3; ++t) { a.ln_g[t] = ln1[t].gamma; a.ln_b[t] = ln1[t].beta; }
  a.ln_eps = ln_eps; a.ln_mode = ln_mode;
  if (!block_narrow_ready(c.h, a, c.s)) return GNX_OK;  // nothing launched: the caller runs gn1 as its own kernels
  r.took = true;
  r.ffe_took = ffe && (c.phase & GNX_PHASE_EDGE_NODE) && block_narrow_ffe_applies(c.h, a, ffe->fc1.act, ffe->fc2.act);
  if (r.ffe_took) set_edge_ffn(a, *ffe, ffe_ln2);
  r.args = a;
  return launch_block_narrow(c.h, a, c.R, c.s, c.phase);
}

// Matrix-core GNCore: ef / nf normalised on load from their row statistics (gf arrives normalised).  Two functions: ASK whether this block
// takes that form (launches nothing), and RUN a phase of it.  Both decide with gamma / beta of ef and nf in the arguments:
static bool wide_ln_applies(const BlockCall& c, const gnx_layernorm* ln1, BlockArgs& a) {
  for (int t = 0; t < 2; ++t) { a.ln_g[t] = ln1[t].gamma; a.ln_b[t] = ln1[t].beta; }
  return !(c.flags & (GNX_FLAG_FORCE_GENERIC | GNX_FLAG_NO_MFMA)) && block_wide_ln_applies(c.h, a);
}
// edge_x6: ... and its edge update is k_edge_x6 (the caller may then leave the edge rows' statistics to that kernel)
static int32_t block_wide_ln_ask(const BlockCall& c, const gnx_layernorm* ln1, bool& applies, bool& edge_x6) {
  applies = edge_x6 = false;
  Prepared q(c);
  if (q.rc) return q.rc;
  applies = wide_ln_applies(c, ln1, q.a);
  edge_x6 = applies && block_wide_edge_x6_applies(c.h, q.a);
  return GNX_OK;
}
// how a run treats the edge rows
struct WideLnEdges {
  bool inline_stats = false;  // no statistics table for the edges: k_edge_x6 computes them in registers
  // ... and then (all three set, a phase with GNX_PHASE_EDGE_NODE) the edge FeedForward + residuals run in that launch too
  const gnx_ffn* ffe = nullptr;
  const gnx_layernorm* ffe_ln2 = nullptr;
  void* ffe_scratch = nullptr;
};
// stats: the row statistics of ef and nf (an entry may be NULL: that input is used as it is).  took == false: the block declined, nothing launched.
static int32_t block_wide_ln_run(const BlockCall& c, const gnx_layernorm* ln1, float ln_eps, int ln_mode, const float* const stats[2], const WideLnEdges& e,
                                 bool& took) {
  took = false;
  Prepared q(c);
  if (q.rc || !(took = wide_ln_applies(c, ln1, q.a))) return q.rc;
  BlockArgs& a = q.a;
  a.ln_stats[0] = stats[0]; a.ln_stats[1] = stats[1];
  if (e.inline_stats) { a.ln_stats[0] = nullptr; a.ln_inline_e = 1; a.ln_eps = ln_eps; a.ln_mode = ln_mode; }
  if (e.inline_stats && e.ffe && e.ffe_ln2 && e.ffe_scratch && (c.phase & GNX_PHASE_EDGE_NODE)) { set_edge_ffn(a, *e.ffe, *e.ffe_ln2); a.ffe_scratch = e.ffe_scratch; }
  return launch_block_wide(c.h, a, c.R, c.s, c.phase);
}

// ---- bfloat16 features (gnx_block_forward_typed) ----
// Does a fused kernel read and write bf16 rows for these widths under the call's forms (FormScope open)?  A run-time specialisation counts
// once it is loaded (gnx_block_typed_workspace_bytes loads it; never inside a capture).
static bool typed_native(const gnx_graphs* h, const gnx_block_params* p, uint32_t flags, hipStream_t s) {
  return !(flags & GNX_FLAG_FORCE_GENERIC) && block_narrow_takes(h, block_probe(h, p), s, true);
}

// workspace of a bf16 call: gnx_block_forward's, then (fallback only) fp32 staging of the six tensors (gnx_staging.h)
static Staging typed_ws(const gnx_graphs* h, const gnx_block_params* p, int64_t R, bool native) {
  const int d[6] = {p->de, p->dn, p->dg, p->oe, p->on, p->og};
  return stage_features(block_ws(h, p, R).total, h, R, d, native ? 0 : 6);
}

// side stream + fork / join events of the handle (see gnx_internal.h); failure just leaves the core on one stream
static void ensure_aux(const gnx_graphs* h) {
  std::call_once(h->aux_once, [h]() {
    // the streams and their events belong to the HANDLE's device, whatever device is current in the querying thread
    int prev = -1;
    (void)hipGetDevice(&prev);
    struct Restore { int d; ~Restore() { if (d >= 0) (void)hipSetDevice(d); } } restore{prev != h->device ? prev : -1};
    if (prev != h->device && hipSetDevice(h->device) != hipSuccess) { (void)hipGetLastError(); return; }
    for (auto& ax : h->aux) {
      hipStream_t st = nullptr;
      hipEvent_t e1 = nullptr, e2 = nullptr;
      hipEvent_t es[4] = {};
      bool ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&e1, hipEventDisableTiming) == hipSuccess &&
                hipEventCreateWithFlags(&e2, hipEventDisableTiming) == hipSuccess;
      for (auto& e : es) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
      if (ok) {
        ax.stream = st; ax.fork = e1; ax.join = e2;
        for (int j = 0; j < 4; ++j) ax.step[j] = es[j];
      } else {
        for (hipEvent_t e : es)
          if (e) (void)hipEventDestroy(e);
        if (e1) (void)hipEventDestroy(e1);
        if (e2) (void)hipEventDestroy(e2);
        if (st) (void)hipStreamDestroy(st);
        (void)hipGetLastError();
        break;
      }
    }
  });
}

// A free side-stream set of the handle's pool (gnx_internal.h: AuxSet), held while the caller enqueues its work: a second host thread in that
// section — same handle, another stream, other buffers — takes the next set; set == NULL (every set taken, or none created): the caller runs
// everything on its own stream.  need_step_events: only a set that has the ring of per-step events.
struct AuxHold {
  std::unique_lock<std::mutex> lock;
  const gnx_graphs::AuxSet* set = nullptr;
};
static AuxHold take_aux(const gnx_graphs* h, bool need_step_events) {
  AuxHold hold;
  for (auto& ax : h->aux) {
    if (!ax.stream || (need_step_events && !ax.step[3])) break;
    std::unique_lock<std::mutex> lk(ax.mu, std::try_to_lock);
    if (lk.owns_lock()) { hold.lock = std::move(lk); hold.set = &ax; break; }
  }
  return hold;
}

// `side` on the set's stream beside `main` on the caller's stream s.  The join event is recorded even after a failed launch — a capture must not
// end with the side stream un-joined — and every status is looked at only once both streams have their work.
template <class Side, class Main>
static int32_t fork_join(const gnx_graphs::AuxSet* aux, hipStream_t s, Side side, Main main) {
  GNX_HIP(hipEventRecord(aux->fork, s));
  GNX_HIP(hipStreamWaitEvent(aux->stream, aux->fork, 0));
  const int32_t rc = side(aux->stream);
  const hipError_t e1 = hipEventRecord(aux->join, aux->stream);
  const int32_t rc2 = main();
  const hipError_t e2 = hipStreamWaitEvent(s, aux->join, 0);
  if (rc) return rc;
  if (rc2) return rc2;
  GNX_HIP(e1);
  GNX_HIP(e2);
  return GNX_OK;
}

}  // namespace gnx

using namespace gnx;

extern "C" {

size_t gnx_block_workspace_bytes(const gnx_graphs* h, const gnx_block_params* p, int64_t R) {
  if (!h || !p || R <= 0) return 0;
  if (check_block(h, p, R) == GNX_OK) {
    warm_block_narrow(h, p);        // run-time specialisation happens here, not in a capture
    warm_block_wide(h, p, false);   // ... and so does the build of the matrix-core tables when these widths take that path
  }
  ensure_aux(h);  // the side streams of gnx_block_forward_steps' two-stream schedule (created outside any capture)
  return block_ws(h, p, R).total;
}

int32_t gnx_block_forward(const gnx_graphs* h, const gnx_block_params* p, const float* ef, const float* nf, const float* gf,
                          int64_t R, float* ef_out, float* nf_out, float* gf_out, void* ws, size_t ws_bytes, uint32_t flags,
                          void* stream) {
  DeviceTurn turn((hipStream_t)stream, p && matrix_core_widths(*p));  // (one matrix-core call at a time per device: gnx_internal.h)
  return block_plain(BlockCall{h, p, GNX_ELEM_F32, ef, nf, gf, R, ef_out, nf_out, gf_out, ws, ws_bytes, flags, (hipStream_t)stream,
                               (flags & GNX_FLAG_DEFER_GRAPH_UPDATE) ? GNX_PHASE_EDGE_NODE : GNX_PHASE_ALL});
}

size_t gnx_block_typed_workspace_bytes(const gnx_graphs* h, const gnx_block_params* p, int64_t R, int32_t elem, uint32_t flags) {
  if (elem == GNX_ELEM_F32) return gnx_block_workspace_bytes(h, p, R);
  if (elem != GNX_ELEM_BF16 || !h || !p || R <= 0 || (flags & GNX_FLAG_DEFER_GRAPH_UPDATE)) return 0;
  ensure_aux(h);  // the side streams of gnx_block_forward_steps_typed's two-stream schedule (the native path never reaches the fp32 query)
  FormScope forms(flags);
  if (check_block(h, p, R) != GNX_OK) return 0;
  warm_block_narrow(h, p, true);  // the bf16 specialisation of these widths, if they need one
  const bool native = typed_native(h, p, flags, nullptr);
  if (!native) (void)gnx_block_workspace_bytes(h, p, R);  // warms the fp32 path the fallback runs
  return typed_ws(h, p, R, native).total;
}

int32_t gnx_block_forward_typed(const gnx_graphs* h, const gnx_block_params* p, int32_t elem, const void* ef, const void* nf, const void* gf, int64_t R,
                                void* ef_out, void* nf_out, void* gf_out, void* ws, size_t ws_bytes, uint32_t flags, void* stream) {
  if (elem == GNX_ELEM_F32)
    return gnx_block_forward(h, p, static_cast<const float*>(ef), static_cast<const float*>(nf), static_cast<const float*>(gf), R, static_cast<float*>(ef_out),
                             static_cast<float*>(nf_out), static_cast<float*>(gf_out), ws, ws_bytes, flags, stream);
  if (elem != GNX_ELEM_BF16) return fail(GNX_ERR_INVALID_ARG, "elem must be GNX_ELEM_F32 or GNX_ELEM_BF16");
  if (flags & GNX_FLAG_DEFER_GRAPH_UPDATE) return fail(GNX_ERR_INVALID_ARG, "GNX_FLAG_DEFER_GRAPH_UPDATE is not supported with bf16 features");
  const hipStream_t s = (hipStream_t)stream;
  FormScope forms(flags);
  BlockCall call{h, p, GNX_ELEM_BF16, ef, nf, gf, R, ef_out, nf_out, gf_out, ws, ws_bytes, flags, s, GNX_PHASE_ALL};
  int32_t rc = check_call(call);
  if (rc) return rc;
  const void* bufs[6] = {ef, nf, gf, ef_out, nf_out, gf_out};
  if ((rc = check_bf16_aligned(bufs, 6))) return rc;
  const bool native = typed_native(h, p, flags, s);
  const Staging w = typed_ws(h, p, R, native);
  if ((rc = check_ws(ws, ws_bytes, w.total, "workspace missing or smaller than gnx_block_typed_workspace_bytes()"))) return rc;
  if (native) {
    DeviceTurn turn(s, false);  // (narrow widths: no matrix instruction)
    call.ws_bytes = w.base;
    return block_plain(call);
  }
  // every other path: widen into the workspace, the fp32 forward (its own dispatch, DeviceTurn included), round the outputs
  if ((rc = stage_widen(w, ws, bufs, 0, 3, s))) return rc;
  rc = gnx_block_forward(h, p, p->de ? w.at(ws, 0) : nullptr, p->dn ? w.at(ws, 1) : nullptr, p->dg ? w.at(ws, 2) : nullptr, R, p->oe ? w.at(ws, 3) : nullptr,
                         p->on ? w.at(ws, 4) : nullptr, p->og ? w.at(ws, 5) : nullptr, ws, w.base, flags, stream);
  return rc ? rc : stage_round(w, ws, bufs, 3, 6, s);
}

// the graph update a call left pending (gnx_block_graph_update; a flush of the loops below): the kernels of this phase read only gf, the graph
// function's parameters and the workspace
static int32_t graph_update(const gnx_graphs* h, const gnx_block_params* p, int32_t elem, const gnx_pending_update& u, int64_t R, uint32_t flags, hipStream_t s) {
  return block_plain(BlockCall{h, p, elem, nullptr, nullptr, u.gf, R, nullptr, nullptr, u.gf_out, const_cast<void*>(u.workspace), u.workspace_bytes, flags, s,
                               GNX_PHASE_GRAPH});
}

// One step of a chain of calls (gnx_block_forward_chained; a step of the loops below), `c` the whole step: chained where these widths chain —
// prev's graph update rides in this launch, this step's is left in *pending — else prev finished the plain way, the step run whole, nothing
// pending (matrix-core / generic kernels, run-time specialised widths, batches of small graphs whose graph update already runs inside the
// block kernel).  The exported pending-update record has float* fields and no element type: a bf16 step exists inside the loop only, validates
// before any launch, and its whole-step form is gnx_block_forward_typed.
static int32_t chained_step(const BlockCall& c, const gnx_pending_update* prev, gnx_pending_update* pending) {
  const bool bf16 = c.elem == GNX_ELEM_BF16;
  int32_t rc = bf16 ? check_call(c) : GNX_OK;
  if (rc) return rc;
  if (prev && prev->workspace && (prev->workspace == c.ws || (c.p && c.p->og > 0 && prev->gf_out == c.gf_out)))
    return fail(GNX_ERR_INVALID_ARG, bf16 ? "internal: the pending step's workspace / gf_out is this step's"
                                          : "the pending call's workspace / gf_out must not be this call's (its graph update has not run yet)");
  bool took = false;
  rc = block_chained(c.on(c.s, GNX_PHASE_EDGE_NODE), prev, took);
  if (rc) return rc;
  if (took) {
    *pending = gnx_pending_update{c.ws, c.ws_bytes, static_cast<const float*>(c.gf), static_cast<float*>(c.gf_out)};
    return GNX_OK;
  }
  if (prev && prev->workspace) {
    rc = graph_update(c.h, c.p, c.elem, *prev, c.R, c.flags, c.s);
    if (rc) return rc;
  }
  *pending = gnx_pending_update{};
  return bf16 ? gnx_block_forward_typed(c.h, c.p, GNX_ELEM_BF16, c.ef, c.nf, c.gf, c.R, c.ef_out, c.nf_out, c.gf_out, c.ws, c.ws_bytes, c.flags, c.s) : block_plain(c);
}

int32_t gnx_block_forward_chained(const gnx_graphs* h, const gnx_block_params* p, const float* ef, const float* nf, const float* gf, int64_t R, float* ef_out,
                                  float* nf_out, float* gf_out, void* ws, size_t ws_bytes, uint32_t flags, void* stream, const gnx_pending_update* prev,
                                  gnx_pending_update* pending) {
  if (!pending) return fail(GNX_ERR_INVALID_ARG, "pending is NULL");
  DeviceTurn turn((hipStream_t)stream, p && matrix_core_widths(*p));
  if (flags & GNX_FLAG_DEFER_GRAPH_UPDATE) return fail(GNX_ERR_INVALID_ARG, "gnx_block_forward_chained defers the graph update itself");
  return chained_step(BlockCall{h, p, GNX_ELEM_F32, ef, nf, gf, R, ef_out, nf_out, gf_out, ws, ws_bytes, flags, (hipStream_t)stream, GNX_PHASE_ALL}, prev, pending);
}

// the bytes a step reads and writes (gnx_step_hazard.h: elem bytes per feature); the workspace is the part the block's kernels use (ws_extent)
static StepSpans step_spans(const gnx_graphs* h, const gnx_block_params* p, int64_t R, const gnx_block_step& st, size_t elem, size_t ws_extent) {
  const void* const in[3] = {st.ef, st.nf, st.gf};
  const void* const out[3] = {st.ef_out, st.nf_out, st.gf_out};
  const long long rows[3] = {(long long)h->E, (long long)h->N, (long long)h->G};
  const int in_w[3] = {p->de, p->dn, p->dg}, out_w[3] = {p->oe, p->on, p->og};
  return step_spans_of(in, out, st.workspace, st.workspace_bytes, rows, in_w, out_w, R, elem, ws_extent);
}

// Can the steps of this call run on two streams?  The fused narrow kernel (plain, chained, pack form, run-time specialised) only: the
// matrix-core widths keep one stream (concurrent matrix kernels: DeviceTurn's history), and so do the generic kernels.
static bool steps_overlap_applies(const gnx_graphs* h, const gnx_block_params* p, int64_t R, uint32_t flags, hipStream_t s) {
  if (!h || !p || matrix_core_widths(*p) || (flags & GNX_FLAG_FORCE_GENERIC) || form(GNX_FLAG_NO_FORK) || profile_enabled()) return false;
  if (check_block(h, p, R) != GNX_OK) return false;  // (the one-stream loop reports it)
  return block_narrow_takes(h, block_probe(h, p), s);
}

// The most steps the loop below puts into one launch: GNX_STEPS_RUN_MAX (read once; 1: one launch per step, the schedule before runs),
// clamped to the table's slots.  The default is the measured best of 2, 4 and 8 on the 1M-edge graph (profiles/steps_runs_c2.md): what a run
// gains grows with its length, and two shorter runs side by side on two streams gain nothing over one.
constexpr int kStepsRunDefault = 8;
static_assert(kRunMax == kRunSlots, "gnx_step_hazard.h groups what gnx_device.h's table holds");
static int steps_run_max() {
  static const int v = [] {
    const char* e = getenv("GNX_STEPS_RUN_MAX");
    const int n = e && *e ? atoi(e) : kStepsRunDefault;
    return n < 1 ? 1 : (n > kRunMax ? kRunMax : n);
  }();
  return v;
}

// GNX_STEPS_DEFER=0 (read once): no run carries the graph updates of the run before it — every run of several steps is two launches, the
// schedule before carrying runs.  For A/B measurements.
static bool steps_defer_on() {
  static const bool v = [] {
    const char* e = getenv("GNX_STEPS_DEFER");
    return !(e && *e && atoi(e) == 0);
  }();
  return v;
}
static int partial_rows_of(const gnx_graphs* h);

// The loop of gnx_block_forward_steps (bf16 rows: gnx_block_forward_steps_typed on the native path), on one stream or — `overlap` — on two.  The
// caller holds the DeviceTurn and the FormScope.
static int32_t steps_schedule(const gnx_graphs* h, const gnx_block_params* p, int32_t elem, const gnx_block_step* steps, int64_t n_steps, int64_t R,
                              uint32_t flags, void* stream, bool overlap) {
  // The schedule lives in gnx_step_hazard.h (StepsPlanner): which steps share a launch, which stream a run goes to, what it waits for, where
  // a graph update ends up.  Here: the side stream, the spans and the validation of the steps a window holds, the launch predicates, and
  // the planner's operations issued one by one.
  // Two streams: even runs on the caller's, odd runs on a side stream of the handle's pool (taken as gnx_core_forward takes it), so that
  // run j + 1's launch fills the slots that run j's ramp and drain leave idle and the per-launch cost of one hides under the other.
  // Every set taken, GNX_FLAG_NO_FORK, the per-kernel profiler on, or not the fused narrow kernel: one stream, the runs in order.
  const AuxHold hold = overlap ? take_aux(h, true) : AuxHold{};
  const gnx_graphs::AuxSet* aux = hold.set;
  const bool two = aux != nullptr;
  hipStream_t str[2] = {(hipStream_t)stream, aux ? aux->stream : nullptr};
  const bool bf16 = elem == GNX_ELEM_BF16;
  const bool valid = h && p && check_block(h, p, R) == GNX_OK;  // (else the first step reports the error)
  // per feature: 4 or 2 bytes; the workspace extent is the workspace query's (bf16 on this path: the native kernels, no staging)
  const size_t elem_bytes = bf16 ? 2 : sizeof(float);
  const size_t ws_extent = !valid ? 0 : bf16 ? typed_ws(h, p, R, true).total : block_ws(h, p, R).total;
  auto call_of = [&](const gnx_block_step& st, hipStream_t s) {
    return BlockCall{h, p, elem, st.ef, st.nf, st.gf, R, st.ef_out, st.nf_out, st.gf_out, st.workspace, st.workspace_bytes, flags, s, GNX_PHASE_ALL};
  };
  auto pending_of = [&](long long s) { return gnx_pending_update{steps[s].workspace, steps[s].workspace_bytes, steps[s].gf, steps[s].gf_out}; };
  // several steps per launch: replicas use blockIdx.y themselves; the widths and the batch must be ones with a run kernel (asked at the first candidate)
  // (the per-kernel profiler attributes time launch by launch, one step each: with it on every run is one step)
  bool can_fuse = valid && R == 1 && !(flags & GNX_FLAG_FORCE_GENERIC) && steps_run_max() > 1 && !profile_enabled();
  // a step joins a run only VALIDATED (the whole step's arguments and workspace): an invalid one starts a run of its own, whose chained
  // step reports the error once everything before it has been issued.  run_args: the launch's shared arguments, from the run's first step.
  auto slot_of = [&](const gnx_block_step& st, RunSlot& sl, BlockArgs* run_args) -> bool {
    Prepared q(call_of(st, str[0]));
    if (q.rc) return false;
    if (run_args) {
      if (!block_narrow_run_applies(h, q.a, bf16)) return can_fuse = false;
      *run_args = q.a;
    }
    sl = RunSlot{q.a.ef, q.a.nf, q.a.gf, q.a.ef_out, q.a.nf_out, q.a.gf_out, q.a.partials};
    return true;
  };
  // The two partial-row areas of a workspace: A, the block's own (BlockWs::part_off), and B, the head of the agg area, which no fused narrow
  // kernel touches.  A carrying run writes the one its predecessor did not, so the rows its front reads are not the rows its tiles write.
  const BlockWs bw = valid && !bf16 ? block_ws(h, p, R) : BlockWs{};
  const bool area_b_fits = valid && !bf16 && bw.part_off - bw.agg_off >= sizeof(float) * (size_t)partial_rows_of(h) * (size_t)((p->oe + p->on + 3) / 4 * 4);
  StepsPlanner planner(two, !bf16 && area_b_fits && steps_defer_on(), steps_run_max(), n_steps);
  // run j's table and shared arguments in [j & 1]: a deferred run is the one before the run being issued, never older
  RunTable tab[2];
  BlockArgs args[2];
  bool took = false;  // the last one-step launch left its graph update pending
  auto hip_rc = [](hipError_t e, const char* what) { return e == hipSuccess ? GNX_OK : hip_fail(e, what); };
  auto issue = [&](const StepsOp& op) -> int32_t {
    const hipStream_t s = str[op.stream];
    switch (op.kind) {
      case kOpFlushRun:
        if (const int32_t rc = launch_block_narrow_run(h, args[op.run & 1], tab[op.run & 1], op.n, s, false, GNX_PHASE_GRAPH)) return rc;
        // (the run's event again, now behind its graph updates: nothing waits for the earlier record yet)
        return hip_rc(hipEventRecord(aux->step[op.run & 3], s), "gnx_block_forward_steps: step event");
      case kOpFlushStep: return graph_update(h, p, elem, pending_of(op.step), R, flags, s);
      case kOpWaitRun: return hip_rc(hipStreamWaitEvent(s, aux->step[op.run & 3], 0), "gnx_block_forward_steps: ordering a step behind the step three before it");
      case kOpBehindOther: {
        hipEvent_t ev = op.stream == 0 ? aux->join : aux->fork;
        hipError_t e = hipEventRecord(ev, str[op.stream ^ 1]);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, ev, 0);
        return hip_rc(e, "gnx_block_forward_steps: ordering a step behind the other stream");
      }
      case kOpLaunchStep: {
        // (an argument error of this step: what is pending belongs to earlier steps, whose arguments were valid — finished at the end, then the error)
        const gnx_pending_update prev = op.ride >= 0 ? pending_of(op.ride) : gnx_pending_update{};
        gnx_pending_update next{};
        const int32_t rc = chained_step(call_of(steps[op.step], s), op.ride >= 0 ? &prev : nullptr, &next);
        took = next.workspace != nullptr;
        return rc;
      }
      case kOpLaunchRun: {
        // (validated before it was planned: a failure here is a launch failure; nothing of this run is pending afterwards)
        const BlockArgs& a = args[op.run & 1];
        RunTable& t = tab[op.run & 1];
        if (op.area == 1)
          for (int z = 0; z < op.n; ++z) t.slot[z].partials = reinterpret_cast<float*>(static_cast<char*>(steps[op.step + z].workspace) + bw.agg_off);
        if (op.form == kRunBlock) return launch_block_narrow_run(h, a, t, op.n, s, false, GNX_PHASE_EDGE_NODE);
        if (op.form == kRunWhole) return launch_block_narrow_run(h, a, t, op.n, s, bf16);
        const RunTable& pt = tab[(op.run & 1) ^ 1];
        PrevTable prev{};
        prev.n = op.ride_n;
        for (int z = 0; z < op.ride_n; ++z) prev.slot[z] = PrevSlot{pt.slot[z].gf, pt.slot[z].gf_out, pt.slot[z].partials};
        return launch_block_narrow_carry(h, a, t, op.n, prev, s);
      }
      case kOpRecordRun: return hip_rc(hipEventRecord(aux->step[op.run & 3], s), "gnx_block_forward_steps: step event");
      case kOpJoin: {
        const hipError_t e1 = hipEventRecord(aux->join, str[1]), e2 = hipStreamWaitEvent(str[0], aux->join, 0);
        GNX_HIP(e1);
        GNX_HIP(e2);
        return GNX_OK;
      }
    }
    return GNX_OK;
  };
  if (two) {
    GNX_HIP(hipEventRecord(aux->fork, str[0]));
    GNX_HIP(hipStreamWaitEvent(str[1], aux->fork, 0));
  }
  int32_t rc = GNX_OK;
  while (planner.first < n_steps && rc == GNX_OK) {
    const int64_t i = planner.first;
    const gnx_block_step& st = steps[i];
    RunTable& t = tab[planner.j & 1] = RunTable{};
    BlockArgs& a = args[planner.j & 1] = BlockArgs{};
    RunSpans cur;
    cur.step[0] = valid ? step_spans(h, p, R, st, elem_bytes, ws_extent) : StepSpans{};
    cur.n = 1;
    if (can_fuse && n_steps - i >= 2) {
      // a run or one step (gnx_step_hazard.h: group_run): the window by address ranges first, then every step of it validated
      RunSpans win = cur;
      while (i + win.n < n_steps) {
        const StepSpans sp = step_spans(h, p, R, steps[i + win.n], elem_bytes, ws_extent);
        if (!planner.takes(win, sp)) break;
        win.step[win.n++] = sp;
      }
      bool ok = planner.is_run(win.n);
      for (int z = 0; ok && z < win.n; ++z) ok = slot_of(steps[i + z], t.slot[z], z == 0 ? &a : nullptr);
      if (ok) cur = win;
    }
    const bool carry_kernel = planner.may_defer(cur) && block_narrow_carry_applies(h, a);
    const long long pnd = planner.pend[0];
    const bool aliases = pnd >= 0 && (steps[pnd].workspace == st.workspace || (p && p->og > 0 && steps[pnd].gf_out == st.gf_out));
    const StepsPlan plan = planner.next(cur, carry_kernel, aliases);
    int issued = 0;
    while (issued < plan.n && (rc = issue(plan.op[issued])) == GNX_OK) ++issued;
    planner.done(plan, cur, issued, took);
  }
  // what is still deferred or pending, then the join — on every path, so that a capture never ends with the side stream un-joined and an
  // error leaves everything issued so far complete when the caller's stream is.  The first error is the call's.
  const StepsPlan end = planner.close();
  for (int z = 0; z < end.n; ++z) {
    const int32_t erc = issue(end.op[z]);
    rc = rc ? rc : erc;
  }
  return rc;
}

int32_t gnx_block_forward_steps(const gnx_graphs* h, const gnx_block_params* p, const gnx_block_step* steps, int64_t n_steps, int64_t R, uint32_t flags,
                                void* stream) {
  if (n_steps < 0 || (n_steps > 0 && !steps)) return fail(GNX_ERR_INVALID_ARG, "gnx_block_forward_steps: steps is NULL / n_steps is negative");
  if (flags & GNX_FLAG_DEFER_GRAPH_UPDATE) return fail(GNX_ERR_INVALID_ARG, "gnx_block_forward_steps finishes every step's graph update itself");
  DeviceTurn turn((hipStream_t)stream, p && matrix_core_widths(*p));  // (one turn for the whole loop; the calls below nest inside it)
  FormScope forms(flags);
  return steps_schedule(h, p, GNX_ELEM_F32, steps, n_steps, R, flags, stream, n_steps > 1 && steps_overlap_applies(h, p, R, flags, (hipStream_t)stream));
}

int32_t gnx_block_forward_steps_typed(const gnx_graphs* h, const gnx_block_params* p, int32_t elem, const gnx_block_step* steps, int64_t n_steps, int64_t R,
                                      uint32_t flags, void* stream) {
  if (elem == GNX_ELEM_F32) return gnx_block_forward_steps(h, p, steps, n_steps, R, flags, stream);
  // every argument error below is found before the first launch (the fp32 loop reports a step's error once the steps before it are issued)
  if (elem != GNX_ELEM_BF16) return fail(GNX_ERR_INVALID_ARG, "elem must be GNX_ELEM_F32 or GNX_ELEM_BF16");
  if (flags & GNX_FLAG_DEFER_GRAPH_UPDATE) return fail(GNX_ERR_INVALID_ARG, "gnx_block_forward_steps_typed finishes every step's graph update itself");
  if (n_steps < 0 || (n_steps > 0 && !steps)) return fail(GNX_ERR_INVALID_ARG, "gnx_block_forward_steps_typed: steps is NULL / n_steps is negative");
  for (int64_t i = 0; i < n_steps; ++i) {
    const gnx_block_step& st = steps[i];
    const void* bufs[6] = {st.ef, st.nf, st.gf, st.ef_out, st.nf_out, st.gf_out};
    for (const void* b : bufs)
      if (((uintptr_t)b & 3) != 0) return fail(GNX_ERR_INVALID_ARG, "bf16 feature buffers must be 4-byte aligned (in every step)");
  }
  const hipStream_t s = (hipStream_t)stream;
  DeviceTurn turn(s, p && matrix_core_widths(*p));  // (one turn for the whole loop; the calls below nest inside it)
  FormScope forms(flags);
  if (!h || !p || check_block(h, p, R) != GNX_OK || !typed_native(h, p, flags, s)) {
    // matrix-core / generic widths, GNX_FLAG_FORCE_GENERIC, GNX_FLAG_NO_JIT, a failed specialisation: n typed forwards in order on the caller's
    // stream, each converting around the fp32 forward inside its own workspace (and the first invalid step reporting its error)
    for (int64_t i = 0; i < n_steps; ++i) {
      const gnx_block_step& st = steps[i];
      if (int32_t rc = gnx_block_forward_typed(h, p, GNX_ELEM_BF16, st.ef, st.nf, st.gf, R, st.ef_out, st.nf_out, st.gf_out, st.workspace, st.workspace_bytes,
                                               flags, stream))
        return rc;
    }
    return GNX_OK;
  }
  // a native bf16 kernel takes these widths (ahead of time, run-time specialised, pack form): the fp32 loop's schedule on bf16 rows
  return steps_schedule(h, p, GNX_ELEM_BF16, steps, n_steps, R, flags, stream, n_steps > 1 && !form(GNX_FLAG_NO_FORK) && !profile_enabled());
}

int32_t gnx_block_graph_update(const gnx_graphs* h, const gnx_block_params* p, const float* gf, int64_t R, float* gf_out, void* ws,
                               size_t ws_bytes, uint32_t flags, void* stream) {
  return graph_update(h, p, GNX_ELEM_F32, gnx_pending_update{ws, ws_bytes, gf, gf_out}, R, flags, (hipStream_t)stream);
}

// partial-sum rows per replica of the fused narrow block (gnx_narrow_launch.h: partial_rows)
static int partial_rows_of(const gnx_graphs* h) { return (int)(h->G == 1 ? (h->n_wtiles() + 3) / 4 : h->n_wtiles()); }

// FeedForward width from which the two Dense layers run on the matrix cores (hidden activations staged in HBM)
static bool ffn_on_mfma(int d) { return d >= 32; }

// Workspace of a core: per entity (edges, nodes, graphs) the outputs of LayerNorm ln1 and ln2, each the size of the entity's rows; the
// FeedForward's hidden buffer (the two-GEMM form; else scratch of the launch that holds it); then the block's workspace.  A form that never
// materialises a LayerNorm output uses that region for something else — the named accessors below are every such use:
struct CoreLayout {
  size_t ln1[3], ln2[3], hidden, block, total;
  float* at(void* ws, size_t off) const { return reinterpret_cast<float*>(static_cast<char*>(ws) + off); }
  float* gn1(void* ws, int t) const { return at(ws, ln1[t]); }
  float* gn2(void* ws, int t) const { return at(ws, ln2[t]); }
  // t = 0, 1: the row statistics of ef / nf (2 floats per row) that the matrix-core kernels normalise from on load
  float* stats(void* ws, int t) const { return gn1(ws, t); }
  // t = 0, 1: the split weight planes of k_ffn_x6 when that FeedForward normalises on load (gn2 of ef / nf is never written then)
  float* x6_planes(void* ws, int t) const { return gn2(ws, t); }
  // the bf16 core: the block's outputs in fp32, exactly the three tensors' sizes (its LayerNorm-on-load block never writes gn1)
  float* block_out(void* ws, int t) const { return gn1(ws, t); }
};
static CoreLayout core_layout(const gnx_graphs* h, const gnx_core_params* p, int64_t R) {
  const size_t rows[3] = {(size_t)R * h->E, (size_t)R * h->N, (size_t)R * h->G};
  const int d[3] = {p->block.de, p->block.dn, p->block.dg};
  CoreLayout L{};
  size_t o = 0, hidden = 0;
  for (int t = 0; t < 3; ++t) {
    L.ln1[t] = o; o += align_up(sizeof(float) * rows[t] * d[t], 256);
    L.ln2[t] = o; o += align_up(sizeof(float) * rows[t] * d[t], 256);
    if (ffn_on_mfma(d[t])) hidden = std::max(hidden, sizeof(float) * rows[t] * 4 * (size_t)d[t]);
  }
  L.hidden = o; o += align_up(hidden, 256);
  L.block = o;
  L.total = o + block_ws(h, &p->block, R).total;
  return L;
}

// ---- validation of a core forward (gnx_core_forward, gnx_core_forward_typed), in the order the fp32 entry has always reported it ----
// GNFeedForward / GNGraphNorm need all three widths > 0 and graphnetadd needs all three present
// (gnfeedforward.jl:18, gngraphnorm.jl:10, gncore.jl:61-68); the block maps dims => dims (gncore.jl:49).
static int32_t check_core_dims(const gnx_block_params& b) {
  if (b.de <= 0 || b.dn <= 0 || b.dg <= 0) return fail(GNX_ERR_DIMS, "GNCore needs all(dims .> 0) (gnfeedforward.jl:18)");
  if (b.oe != b.de || b.on != b.dn || b.og != b.dg) return fail(GNX_ERR_DIMS, "GNCore's block must map dims => dims (gncore.jl:49)");
  return GNX_OK;
}
// b: the core's block (p->block with the core's prepared planes)
static int32_t check_core(const gnx_graphs* h, const gnx_core_params* p, const gnx_block_params& b, int64_t R, const void* ef, const void* nf, const void* gf,
                          const void* ef_out, const void* nf_out, const void* gf_out, uint32_t flags) {
  int32_t rc = check_core_dims(b);
  if (rc) return rc;
  rc = check_block(h, &b, R);
  if (rc) return rc;
  if (((!ef || !ef_out) && h->E > 0) || !nf || !gf || !nf_out || !gf_out) return fail(GNX_ERR_INVALID_ARG, "GNCore needs ef, nf, gf and all outputs");
  for (int t = 0; t < 3; ++t) {
    if (!p->ln1[t].gamma || !p->ln1[t].beta || !p->ln2[t].gamma || !p->ln2[t].beta) return fail(GNX_ERR_INVALID_ARG, "LayerNorm parameter is NULL");
    if (!p->ff[t].fc1.weight || !p->ff[t].fc2.weight) return fail(GNX_ERR_INVALID_ARG, "FeedForward weight is NULL");
  }
  if (p->eps_mode != 0 && p->eps_mode != 1) return fail(GNX_ERR_INVALID_ARG, "eps_mode must be 0 or 1");
  const int dd[3] = {b.de, b.dn, b.dg};
  for (int t = 0; t < 3; ++t) {
    const bool generic = !ffn_on_mfma(dd[t]) || (flags & (GNX_FLAG_FORCE_GENERIC | GNX_FLAG_NO_MFMA));
    if (generic && (size_t)dd[t] * 5 * 4 * sizeof(float) > 64 * 1024)
      return fail(GNX_ERR_DIMS, "GNCore width too large for the generic FFN kernel (80*d bytes of LDS)");
  }
  return GNX_OK;
}

}  // extern "C"
namespace gnx {
// (gnx_launchers.h: what gnx_core_forward_train_typed checks before its own launches)
int32_t core_forward_check_dims(const gnx_core_params* p) { return check_core_dims(p->block); }
int32_t core_forward_check(const gnx_graphs* h, const gnx_core_params* p, int64_t R, const void* ef, const void* nf, const void* gf, const void* ef_out,
                           const void* nf_out, const void* gf_out, uint32_t flags) {
  gnx_block_params b = p->block;
  b.prepared = p->prepared;
  return check_core(h, p, b, R, ef, nf, gf, ef_out, nf_out, gf_out, flags);
}
}  // namespace gnx
extern "C" {

// ---- the GNCore forward: a validated call (CoreRun), what it does (CorePlan: decided before the first launch), the FeedForward step ----
// The form of an entity's FeedForward + residual: out = block(gn1 x) + x + fc2(act1(fc1(gn2 x)))   (gncore.jl:56-68, gnfeedforward.jl:27-31)
enum FfForm {
  FF_DONE,          // the block's edge launch was the edge form of k_ffn_x6: out[0] is final
  FF_LN_ON_LOAD,    // launch_ffn_fused normalises x as it loads it: from the statistics table, or (edges, inline_e) with the statistics in registers
  FF_MATERIALISED,  // launch_ffn_fused on gn2(x) in HBM, no scratch (node_mat's node rows)
  FF_HIDDEN,        // launch_ffn_fused on gn2(x), the hidden buffer its scratch; where it declines, two launch_dense_rows through the hidden buffer
  FF_POST,          // a narrow width: k_core_post (recomputes gn2)
  FF_RESIDUAL       // the generic kernel on gn2(x)
};
// Every decision of a core forward that its arguments alone determine.  What a LAUNCHER answers — whether the narrow block took the
// LayerNorm-on-load form and the edge FeedForward, whether k_core_post3 / launch_ffn_fused declined — is consumed where it is returned.
struct CorePlan {
  bool all_narrow = false;  // three narrow widths: the fused narrow block is asked to normalise on load; FeedForwards by k_core_post3 / k_core_post
  bool post3 = false;       // ... and the one-launch post kernel applies: the block is asked to leave its graph update (and take the edge FeedForward)
  bool wide_ln = false;     // the matrix-core block and FeedForwards normalise ef / nf on load: neither LayerNorm output of them exists in HBM
  bool inline_e = false, fuse_e = false, ln_on_load = false, node_x6_forms = false, node_mat = false;  // (core_plan)
  bool may_fork = false;    // the call may take a side stream of the handle
  FfForm ff[3] = {};
};
struct CoreRun {
  const gnx_graphs* h; const gnx_core_params* p; int64_t R; uint32_t flags;
  size_t rows[3]; int d[3];            // per entity: rows (all replicas), width
  const float* x[3]; float* out[3];    // the caller's tensors
  float *l1[3], *l2[3], *stats[2], *planes[2], *hidden;  // regions of the workspace (CoreLayout)
  CorePlan plan;
  int32_t make_plan(const BlockCall& wide, hipStream_t s);
  int32_t ffn(int t, hipStream_t st) const;
};

// wide: the core's block as the matrix-core form reads it (asked here, launched by gnx_core_forward)
int32_t CoreRun::make_plan(const BlockCall& wide, hipStream_t s) {
  CorePlan& pl = plan;
  // All three widths narrow: the fused block kernel normalises its inputs as it loads them (gn1 never materialised) when it
  // is available for this width set; gn2 is recomputed inside k_core_post either way.
  pl.all_narrow = core_narrow_width(d[0]) && core_narrow_width(d[1]) && core_narrow_width(d[2]) && !(flags & GNX_FLAG_FORCE_GENERIC);
  // (the graph level of a NARROW core on the handle's side stream — graph update + the G-row / N-row k_core_post launches behind the
  // edges' k_core_post — was measured: README ex.3 model 298 vs 271 us; two fork/join pairs cost more than the ~20 us they hide)
  // when the three FeedForwards go out as ONE launch (k_core_post3), the block's graph update runs inside it: the block is launched
  // without its k_graph_t
  pl.post3 = pl.all_narrow && h->E > 0 && !(flags & GNX_FLAG_DEFER_GRAPH_UPDATE) && core_post3_applies(rows, d, p->ff, true, s);
  // Wide edges and nodes: the matrix-core kernels normalise x as they load it (block: gn1, fused FeedForward: gn2) from one pass of
  // row statistics — neither LayerNorm output of ef / nf exists in HBM.  Taken when the block runs in the projected quad-row form
  // and both FeedForwards are the fused kernel's; gf (G rows) is normalised by the ordinary kernel.
  bool edge_x6 = false;
  if (!pl.all_narrow && !form(GNX_FLAG_NO_LN_FUSE) && !(flags & (GNX_FLAG_FORCE_GENERIC | GNX_FLAG_NO_MFMA)) && h->E > 0) {
    bool ok = true;
    for (int t = 0; t < 2; ++t)
      ok = ok && ln_stats_applies(x[t], d[t]) && ffn_fused_applies(x[t], d[t], p->ff[t], out[t], x[t], out[t]) &&
           (((uintptr_t)p->ln2[t].gamma | (uintptr_t)p->ln2[t].beta) & 15) == 0;
    if (ok)
      if (const int32_t rc = block_wide_ln_ask(wide, p->ln1, pl.wide_ln, edge_x6)) return rc;
  }
  // Both consumers of the edge rows' statistics hold whole rows in registers when they are the six-term kernels (k_edge_x6: gn1, k_ffn_x6: gn2) and
  // compute them there, bit-identical to k_ln_stats_v4 (gnx_x6_stats.h): the statistics pass over ef — 512 MB at 1M edges — is not launched.
  pl.inline_e = pl.wide_ln && edge_x6 && d[0] == 128 && rows[0] >= 4096 && !form(GNX_FLAG_LN_STATS_PASS) &&
                ffn_x6_applies(x[0], d[0], p->ff[0], out[0], x[0], out[0], sizeof(float) * rows[0] * d[0]);
  // ... and then ONE launch does both (the edge form of k_ffn_x6: ef' stays in the accumulator — never written, never read back; GNX_CORE_EDGE_SPLIT=1: two launches)
  pl.fuse_e = pl.inline_e && !form(GNX_FLAG_CORE_EDGE_SPLIT) && !(edge_n_enabled() && d[1] == 64);  // (the opt-in k_edge_n gathers RAW source rows: its projection tables are not the one-launch form's)
  // Round 6 (profiles/r06_overlap_hazard.log): the GENERAL kernels (k_rows_gemm, k_ffn_fused) came out wrong now and then beside another queue's
  // matrix kernel, but only in launches that normalise on load from a statistics table; the site was found later in the round (their LayerNorm
  // branch consumed an LDS read too early on a shared CU) and is guarded (GNX_LN_GUARD).  This rule predates the guard and stays as a second,
  // independent protection of the path small batches take: a statistics table is consumed by six-term kernels only — an entity whose rows a general
  // kernel would normalise on load gets its LayerNorms MATERIALISED instead (k_layernorm2, one more pass over rows that are few whenever this
  // happens: below 4096, or widths without a six-term kernel).  GNX_FLAG_LN_ON_LOAD restores the statistics-table forms (exact too since the guard).
  pl.ln_on_load = form(GNX_FLAG_LN_ON_LOAD) || form(GNX_FLAG_FP32_MFMA | GNX_FLAG_PROJ_FP32 | GNX_FLAG_LN_STATS_PASS | GNX_FLAG_CORE_EDGE_SPLIT);  // (the diagnostic forms keep their tables)
  if (pl.wide_ln && !pl.ln_on_load && !pl.inline_e) pl.wide_ln = false;  // the edge rows' table would feed k_rows_gemm / k_ffn_fused: everything materialised
  pl.node_x6_forms = d[0] == 128 && d[1] == 64 && h->N >= 4096 && p->block.nodefn.act <= GNX_ACT_RELU;  // k_proj_x6, k_node_x6, k_ffn_x6<64> take the node rows
  pl.node_mat = pl.wide_ln && !pl.ln_on_load && !pl.node_x6_forms;  // edges by the six-term kernels (statistics in registers), node LayerNorms materialised
  // A side stream is for the matrix-core form alone (the narrow core's measurement above).  GNX_NO_FORK=1, or the per-kernel profiler on:
  // everything on the caller's stream.
  pl.may_fork = pl.wide_ln && !form(GNX_FLAG_NO_FORK) && !profile_enabled();
  for (int t = 0; t < 3; ++t) {
    if (ffn_on_mfma(d[t]) && !(flags & (GNX_FLAG_FORCE_GENERIC | GNX_FLAG_NO_MFMA)))
      pl.ff[t] = !(pl.wide_ln && t < 2) ? FF_HIDDEN : (t == 0 && pl.fuse_e) ? FF_DONE : (t == 1 && pl.node_mat) ? FF_MATERIALISED : FF_LN_ON_LOAD;
    else
      pl.ff[t] = core_narrow_width(d[t]) && !(flags & GNX_FLAG_FORCE_GENERIC) ? FF_POST : FF_RESIDUAL;
  }
  return GNX_OK;
}

// The FeedForward + residual of entity t on stream st, in the form the plan names: the one copy of this dispatch.
int32_t CoreRun::ffn(int t, hipStream_t st) const {
  const gnx_ffn& ff = p->ff[t];
  switch (plan.ff[t]) {
    case FF_DONE: return GNX_OK;
    case FF_LN_ON_LOAD: {  // (the entity's gn2 region is unused in this form: room for the split weight planes of k_ffn_x6)
      const bool inl = t == 0 && plan.inline_e;
      return launch_ffn_fused(h, t, x[t], d[t], ff, out[t], x[t], out[t], R, st, inl ? nullptr : stats[t], &p->ln2[t], planes[t], sizeof(float) * rows[t] * d[t], inl, p->eps,
                              p->eps_mode);
    }
    case FF_MATERIALISED: return launch_ffn_fused(h, t, l2[t], d[t], ff, out[t], x[t], out[t], R, st);
    case FF_HIDDEN: {
      // hidden layer never leaves the chip (d = 64, 128); the edges' and nodes' launch may use the hidden buffer of the two-GEMM form as its scratch.
      // Not the G rows': their FeedForward may be the side stream's, where the hidden buffer belongs to its two-GEMM form alone.
      int32_t rc = launch_ffn_fused(h, t, l2[t], d[t], ff, out[t], x[t], out[t], R, st, nullptr, nullptr, t < 2 ? hidden : nullptr, sizeof(float) * rows[t] * 4 * (size_t)d[t]);
      if (rc != 1) return rc;
      if ((rc = launch_dense_rows(h, t, l2[t], d[t], ff.fc1, 4 * d[t], nullptr, nullptr, hidden, R, st, "k_rows_gemm_ff1"))) return rc;
      return launch_dense_rows(h, t, hidden, 4 * d[t], ff.fc2, d[t], out[t], x[t], out[t], R, st, "k_rows_gemm_ff2");
    }
    case FF_POST: return launch_core_post(x[t], rows[t], d[t], p->ln2[t], ff, p->eps, p->eps_mode, out[t], st);
    case FF_RESIDUAL: break;
  }
  return launch_ffn_residual(l2[t], x[t], rows[t], d[t], ff, out[t], st);
}

size_t gnx_core_workspace_bytes(const gnx_graphs* h, const gnx_core_params* p, int64_t R) {
  if (!h || !p || R <= 0) return 0;
  ensure_aux(h);
  warm_block_wide(h, &p->block, ffn_on_mfma(p->block.de) || ffn_on_mfma(p->block.dn) || ffn_on_mfma(p->block.dg));
  {  // run-time specialisation of a narrow core's combined FeedForward launch happens here (as for the block: never in a capture)
    const size_t rows[3] = {(size_t)R * h->E, (size_t)R * h->N, (size_t)R * h->G};
    const int d[3] = {p->block.de, p->block.dn, p->block.dg};
    if (h->E > 0 && core_narrow_width(d[0]) && core_narrow_width(d[1]) && core_narrow_width(d[2])) (void)core_post3_applies(rows, d, p->ff, true, nullptr);
  }
  return core_layout(h, p, R).total;
}

int32_t gnx_core_forward(const gnx_graphs* h, const gnx_core_params* p, const float* ef, const float* nf, const float* gf,
                         int64_t R, float* ef_out, float* nf_out, float* gf_out, void* ws, size_t ws_bytes, uint32_t flags,
                         void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!h || !p) return fail(GNX_ERR_INVALID_ARG, "NULL handle or params");
  DeviceTurn turn(s, matrix_core_widths(p->block));  // (one matrix-core call at a time per device: gnx_internal.h)
  FormScope forms(flags);  // the forms this call selected (gnx.h: GNX_FLAG_FFN_FP32 ...)
  gnx_block_params b = p->block;
  b.prepared = p->prepared;  // (the core's object holds its block's planes too; block.prepared is ignored)
  PreparedScope prepared(p->prepared);
  int32_t rc = check_core(h, p, b, R, ef, nf, gf, ef_out, nf_out, gf_out, flags);
  if (rc) return rc;
  const CoreLayout L = core_layout(h, p, R);
  if ((rc = check_ws(ws, ws_bytes, L.total, "workspace missing or smaller than gnx_core_workspace_bytes()"))) return rc;
  CoreRun c{h, p, R, flags, {(size_t)R * h->E, (size_t)R * h->N, (size_t)R * h->G}, {b.de, b.dn, b.dg}, {ef, nf, gf}, {ef_out, nf_out, gf_out}};
  for (int t = 0; t < 3; ++t) { c.l1[t] = L.gn1(ws, t); c.l2[t] = L.gn2(ws, t); }
  for (int t = 0; t < 2; ++t) { c.stats[t] = L.stats(ws, t); c.planes[t] = L.x6_planes(ws, t); }
  c.hidden = L.at(ws, L.hidden);
  const size_t* rows = c.rows;
  const int* d = c.d;
  const float* const* x = c.x;
  // the core's block as the forms see it; every call below is this one on its own inputs, stream and phase
  const BlockCall blk{h, &b, GNX_ELEM_F32, ef, nf, gf, R, ef_out, nf_out, gf_out, static_cast<char*>(ws) + L.block, ws_bytes - L.block, flags, s, GNX_PHASE_ALL};
  BlockCall wide = blk.with(ef, nf, c.l1[2]);  // the matrix-core form reads ef and nf raw (normalised on load) and gf normalised
  if ((rc = c.make_plan(wide, s))) return rc;
  const CorePlan& pl = c.plan;

  // ---- LayerNorms / statistics, then the block ----
  NarrowLnResult narrow;  // the narrow block's answers: it normalised on load (took); the edge FeedForward ran in its edge lanes (ffe_took)
  // A side stream and its pair of events from the handle's pool, held while this call enqueues its work (a second host thread in this section —
  // same handle, another stream, other buffers — takes the next set; with every set taken a caller runs everything on its own stream).
  const AuxHold hold = pl.may_fork ? take_aux(h, false) : AuxHold{};
  const gnx_graphs::AuxSet* aux = hold.set;
  if (pl.all_narrow) {
    // (the FeedForward moves into the block kernel only together with the one-launch post kernel, which then skips the edge rows)
    rc = block_narrow_ln(blk.on(s, pl.post3 ? GNX_PHASE_EDGE_NODE : GNX_PHASE_ALL), p->ln1, p->eps, p->eps_mode, pl.post3 ? &p->ff[0] : nullptr, p->ln2[0], narrow);
    if (rc) return rc;
  }
  const float* const stats[2] = {c.stats[0], pl.node_mat ? nullptr : c.stats[1]};  // what the matrix-core block normalises ef / nf from (NULL: used as it is)
  if (pl.wide_ln) {
    wide.nf = pl.node_mat ? c.l1[1] : x[1];  // node_mat: gn1(nf) itself (and l2[1] = gn2(nf) for the FeedForward)
    auto node_ln = [&](hipStream_t st) -> int32_t {
      return pl.node_mat ? launch_layernorm2(x[1], rows[1], d[1], p->ln1[1], p->ln2[1], p->eps, p->eps_mode, c.l1[1], c.l2[1], st)
                         : launch_ln_stats(x[1], rows[1], d[1], p->eps, p->eps_mode, c.stats[1], st);
    };
    auto edge_stats = [&]() -> int32_t { return pl.inline_e ? GNX_OK : launch_ln_stats(x[0], rows[0], d[0], p->eps, p->eps_mode, c.stats[0], s); };
    if ((rc = launch_layernorm2(x[2], rows[2], d[2], p->ln1[2], p->ln2[2], p->eps, p->eps_mode, c.l1[2], c.l2[2], s))) return rc;
    if (aux) {
      // side stream: node statistics, gf fold, node projections (latency / matrix-core work) beside the edge statistics pass (HBM-bound)
      auto node_side = [&](hipStream_t ax) -> int32_t {
        bool took0 = false;
        const int32_t r = node_ln(ax);
        return r ? r : block_wide_ln_run(wide.on(ax, GNX_PHASE_WIDE_PROJ_ONLY), p->ln1, p->eps, p->eps_mode, stats, WideLnEdges{}, took0);
      };
      if ((rc = fork_join(aux, s, node_side, edge_stats))) return rc;
    } else {
      if ((rc = edge_stats())) return rc;
      if ((rc = node_ln(s))) return rc;
    }
    // (two streams: the block's graph update is left to the side stream, below; the node projections are done)
    bool took = false;
    const WideLnEdges edges{pl.inline_e, pl.fuse_e ? &p->ff[0] : nullptr, pl.fuse_e ? &p->ln2[0] : nullptr, pl.fuse_e ? c.planes[0] : nullptr};
    rc = block_wide_ln_run(wide.on(s, aux ? GNX_PHASE_EDGE_NODE | GNX_PHASE_WIDE_PROJ_DONE : GNX_PHASE_ALL), p->ln1, p->eps, p->eps_mode, stats, edges, took);
    if (rc) return rc;
    if (!took) return fail(GNX_ERR_INVALID_ARG, "gnx_core_forward: the block declined the form it had accepted");
  } else if (!narrow.took) {
    for (int t = 0; t < 3; ++t) {
      // narrow widths (FeedForward by k_core_post, which recomputes gn2): only gn1(x) is materialised (the block needs it)
      if (pl.ff[t] == FF_POST) rc = launch_ln1_rows(x[t], rows[t], d[t], p->ln1[t], p->eps, p->eps_mode, c.l1[t], s);
      else rc = launch_layernorm2(x[t], rows[t], d[t], p->ln1[t], p->ln2[t], p->eps, p->eps_mode, c.l1[t], c.l2[t], s);
      if (rc) return rc;
    }
    rc = block_plain(blk.with(c.l1[0], c.l1[1], c.l1[2]));  // everything materialised: the plain block on gn1(x)
    if (rc) return rc;
  }

  // ---- FeedForward + residual per entity ----
  if (pl.all_narrow) {  // the three entities' FeedForward + residual in one launch when the width triple has the combined kernel
    const bool defer_gu = pl.post3 && narrow.took;  // ... with the graph update the block left
    rc = launch_core_post3(x, rows, d, p->ln2, p->ff, p->eps, p->eps_mode, c.out, s, defer_gu ? &narrow.args : nullptr, partial_rows_of(h), narrow.ffe_took);
    if (rc != 1) return rc;
    if (narrow.ffe_took) return fail(GNX_ERR_INVALID_ARG, "internal: the edge FeedForward ran in the block kernel but the one-launch post kernel declined");
  }
  if (!aux) {
    for (int t = 0; t < 3; ++t)
      if ((rc = c.ffn(t, s))) return rc;
    return GNX_OK;
  }
  // Two streams.  The graph level of the core — the block's graph update (four 5-us launches) and the G-row FeedForward — is independent of the
  // edge / node FeedForwards that follow the block: it runs on the handle's side stream beside them (fork after the node update, join
  // before returning; inside a capture the side stream joins the captured graph).
  // The node FeedForward rides on the side stream too: its workgroups fill the CUs that the edge FeedForward's last, partly filled round of
  // tiles leaves idle (7813 tiles on 512 slots: 15.26 rounds).
  static const bool node_ffn_main = getenv("GNX_NODE_FFN_MAIN") != nullptr;
  auto graph_side = [&](hipStream_t ax) -> int32_t {
    bool took = false;
    int32_t r = block_wide_ln_run(wide.on(ax, GNX_PHASE_GRAPH), p->ln1, p->eps, p->eps_mode, stats, WideLnEdges{}, took);
    if (r == GNX_OK) r = c.ffn(2, ax);
    return r == GNX_OK && !node_ffn_main ? c.ffn(1, ax) : r;
  };
  auto edge_main = [&]() -> int32_t {
    const int32_t r = c.ffn(0, s);
    return r == GNX_OK && node_ffn_main ? c.ffn(1, s) : r;
  };
  return fork_join(aux, s, graph_side, edge_main);
}

// ---- bfloat16 features (gnx_core_forward_typed) ----
// Does the core run natively on bf16 rows under the call's forms (FormScope open)?  Where the fp32 core takes the fused LayerNorm-on-load
// block kernel of the ahead-of-time set: README ex.3's widths at the default wave-tile size, a batch with edges.  Everything else — the
// matrix-core widths, other narrow triples (run-time specialised ones too), GNX_FLAG_FORCE_GENERIC, GNX_FLAG_NO_JIT — converts around
// gnx_core_forward.
static bool core_typed_native(const gnx_graphs* h, const gnx_core_params* p, uint32_t flags) {
  if ((flags & GNX_FLAG_FORCE_GENERIC) || form(GNX_FLAG_NO_JIT)) return false;
  const BlockArgs a = block_probe(h, &p->block);
  return p->block.og == 3 && a.n_wtiles > 0 && a.E > 0 && narrow_ln_aot(h, a, true);
}

// workspace of a bf16 core call: gnx_core_forward's, then (fallback only) fp32 copies of the six tensors (gnx_staging.h).  The native path
// stages the block's three outputs in fp32 too, but inside the fp32 layout (CoreLayout::block_out): no byte beyond the fp32 core's workspace.
static Staging core_typed_ws(const gnx_graphs* h, const gnx_core_params* p, int64_t R, bool native) {
  const int d[6] = {p->block.de, p->block.dn, p->block.dg, p->block.de, p->block.dn, p->block.dg};
  return stage_features(core_layout(h, p, R).total, h, R, d, native ? 0 : 6);
}

// The native path (validated call, core_typed_native): the fp32 narrow core's launches on bf16 rows.  The block normalises the bf16 rows as it
// loads them and hands ef' / nf' / gf' on in fp32 (st[]: intermediates of the core never pass through bf16); the post kernels read x as bf16,
// the block's rows from st[], and store the core's rows rounded once.  One-launch form (core_post3_applies): the block without its graph
// update — with the edge FeedForward in its edge lanes where block_narrow_ffe_applies, which then stores the core's edge rows itself and
// no edge-sized staging is written — then k_core_post3 with the graph update inside; else the block whole, then k_core_post per entity.
static int32_t core_forward_bf16_native(const gnx_graphs* h, const gnx_core_params* p, const gnx_block_params& b, const void* const x[3], int64_t R, void* const out[3],
                                        void* ws, size_t ws_bytes, uint32_t flags, hipStream_t s) {
  const CoreLayout L = core_layout(h, p, R);
  float* const st[3] = {L.block_out(ws, 0), L.block_out(ws, 1), L.block_out(ws, 2)};
  const size_t rows[3] = {(size_t)R * h->E, (size_t)R * h->N, (size_t)R * h->G};
  const int d[3] = {b.de, b.dn, b.dg};
  const bool post3 = core_post3_applies(rows, d, p->ff, true, s);
  const int phase = post3 ? GNX_PHASE_EDGE_NODE : GNX_PHASE_ALL;
  Prepared q(BlockCall{h, &b, GNX_ELEM_BF16, x[0], x[1], x[2], R, st[0], st[1], st[2], static_cast<char*>(ws) + L.block, ws_bytes - L.block, flags, s, phase});
  if (q.rc) return q.rc;
  BlockArgs& a = q.a;
  for (int t = 0; t < 3; ++t) { a.ln_g[t] = p->ln1[t].gamma; a.ln_b[t] = p->ln1[t].beta; }
  a.ln_eps = p->eps; a.ln_mode = p->eps_mode;
  const bool ffe = post3 && block_narrow_ffe_applies(h, a, p->ff[0].fc1.act, p->ff[0].fc2.act);
  if (ffe) {
    set_edge_ffn(a, p->ff[0], p->ln2[0]);
    a.ef_out = static_cast<float*>(out[0]);  // (bf16 rows in a float* field, as the inputs: the edge lanes store the core's edge rows)
  }
  int32_t rc = launch_block_narrow(h, a, R, s, phase, true);
  if (rc) return rc == 1 ? fail(GNX_ERR_INVALID_ARG, "internal: the bf16 core's block declined the form it had accepted") : rc;
  const float* xf[3];
  float* of[3];
  for (int t = 0; t < 3; ++t) { xf[t] = static_cast<const float*>(x[t]); of[t] = static_cast<float*>(out[t]); }
  if (post3) return launch_core_post3(xf, rows, d, p->ln2, p->ff, p->eps, p->eps_mode, of, s, &a, partial_rows_of(h), ffe, st);
  for (int t = 0; t < 3; ++t)
    if ((rc = launch_core_post(xf[t], rows[t], d[t], p->ln2[t], p->ff[t], p->eps, p->eps_mode, of[t], s, st[t]))) return rc;
  return GNX_OK;
}

static int32_t pad_impl(const gnx_graphs* h, int32_t kind, bool pad, const float* src, int32_t d, int64_t R, float* dst, void* stream) {
  if (!h) return fail(GNX_ERR_INVALID_ARG, "NULL argument");
  if (kind != 0 && kind != 1) return fail(GNX_ERR_INVALID_ARG, "kind must be 0 (edges) or 1 (nodes)");
  // the packed side of a batch without edges has no rows (its buffer may be NULL, as for the forwards); the padded side always exists
  const bool packed_empty = (kind == 0 ? h->E : h->N) == 0;
  if ((pad ? !dst : !src) || ((pad ? !src : !dst) && !packed_empty)) return fail(GNX_ERR_INVALID_ARG, "NULL argument");
  if (d <= 0 || R <= 0) return fail(GNX_ERR_INVALID_ARG, "d and n_replicas must be >= 1");
  if (R > 1 && h->G != 1) return fail(GNX_ERR_INVALID_ARG, "n_replicas > 1 needs a single-graph handle");
  return launch_pad(h, kind, pad, src, d, R, dst, (hipStream_t)stream);
}

size_t gnx_core_typed_workspace_bytes(const gnx_graphs* h, const gnx_core_params* p, int64_t R, int32_t elem, uint32_t flags) {
  if (elem == GNX_ELEM_F32) return gnx_core_workspace_bytes(h, p, R);
  if (elem != GNX_ELEM_BF16 || !h || !p || R <= 0 || (flags & GNX_FLAG_DEFER_GRAPH_UPDATE)) return 0;
  const size_t base = gnx_core_workspace_bytes(h, p, R);  // side streams, the matrix-core tables, the run-time specialisations of the fp32 core the fallback runs
  FormScope forms(flags);
  if (check_core_dims(p->block) != GNX_OK || check_block(h, &p->block, R) != GNX_OK) return base;  // (the forward reports it)
  const bool native = core_typed_native(h, p, flags);
  if (!native) (void)gnx_block_workspace_bytes(h, &p->block, R);  // ... and of its block
  return core_typed_ws(h, p, R, native).total;
}

int32_t gnx_core_forward_typed(const gnx_graphs* h, const gnx_core_params* p, int32_t elem, const void* ef, const void* nf, const void* gf, int64_t R,
                               void* ef_out, void* nf_out, void* gf_out, void* ws, size_t ws_bytes, uint32_t flags, void* stream) {
  if (elem == GNX_ELEM_F32)
    return gnx_core_forward(h, p, static_cast<const float*>(ef), static_cast<const float*>(nf), static_cast<const float*>(gf), R, static_cast<float*>(ef_out),
                            static_cast<float*>(nf_out), static_cast<float*>(gf_out), ws, ws_bytes, flags, stream);
  if (elem != GNX_ELEM_BF16) return fail(GNX_ERR_INVALID_ARG, "elem must be GNX_ELEM_F32 or GNX_ELEM_BF16");
  if (flags & GNX_FLAG_DEFER_GRAPH_UPDATE) return fail(GNX_ERR_INVALID_ARG, "GNX_FLAG_DEFER_GRAPH_UPDATE is not supported with bf16 features");
  // what needs no handle comes first: every refusal below happens before any GPU work
  if (!p) return fail(GNX_ERR_INVALID_ARG, "NULL handle or params");
  const void* bufs[6] = {ef, nf, gf, ef_out, nf_out, gf_out};
  int32_t rc = check_bf16_aligned(bufs, 6);
  if (rc) return rc;
  if ((rc = check_core_dims(p->block))) return rc;
  if (!h) return fail(GNX_ERR_INVALID_ARG, "NULL handle or params");
  const hipStream_t s = (hipStream_t)stream;
  FormScope forms(flags);
  gnx_block_params b = p->block;
  b.prepared = p->prepared;
  if ((rc = check_core(h, p, b, R, ef, nf, gf, ef_out, nf_out, gf_out, flags))) return rc;
  const bool native = core_typed_native(h, p, flags);
  const Staging w = core_typed_ws(h, p, R, native);
  if ((rc = check_ws(ws, ws_bytes, w.total, "workspace missing or smaller than gnx_core_typed_workspace_bytes()"))) return rc;
  if (native) {
    DeviceTurn turn(s, false);  // (narrow widths: no matrix instruction)
    PreparedScope prepared(p->prepared);
    const void* const x[3] = {ef, nf, gf};
    void* const out[3] = {ef_out, nf_out, gf_out};
    return core_forward_bf16_native(h, p, b, x, R, out, ws, w.base, flags, s);
  }
  // every other path: widen into the workspace, the fp32 core (its own dispatch, DeviceTurn included), round the outputs
  if ((rc = stage_widen(w, ws, bufs, 0, 3, s))) return rc;
  // (a batch without edges: its empty edge buffers may be NULL, for the fp32 core too)
  rc = gnx_core_forward(h, p, w.n[0] ? w.at(ws, 0) : nullptr, w.at(ws, 1), w.at(ws, 2), R, w.n[3] ? w.at(ws, 3) : nullptr, w.at(ws, 4), w.at(ws, 5), ws, w.base, flags,
                        stream);
  return rc ? rc : stage_round(w, ws, bufs, 3, 6, s);
}

int32_t gnx_row_stats(const float* x, int64_t rows, int32_t d, float eps, int32_t eps_mode, float* stats, void* stream) {
  if (!x || !stats || rows < 0) return fail(GNX_ERR_INVALID_ARG, "gnx_row_stats: NULL argument / negative row count");
  if (eps_mode != 0 && eps_mode != 1) return fail(GNX_ERR_INVALID_ARG, "eps_mode must be 0 or 1");
  return launch_ln_stats(x, (size_t)rows, d, eps, eps_mode, stats, (hipStream_t)stream);
}

int32_t gnx_pad_features(const gnx_graphs* h, int32_t kind, const float* packed, int32_t d, int64_t R, float* padded, void* stream) {
  return pad_impl(h, kind, true, packed, d, R, padded, stream);
}

size_t gnx_xent_workspace_bytes(int64_t cols) { return cols > 0 ? sizeof(float) * (size_t)xent_blocks(cols) + 16 : 0; }

int32_t gnx_logit_cross_entropy(const float* logits, const float* targets, int32_t d, int64_t cols, float* loss_out, void* ws,
                                size_t ws_bytes, void* stream) {
  if (!logits || !targets || !loss_out) return fail(GNX_ERR_INVALID_ARG, "NULL argument");
  if (d <= 0 || cols <= 0) return fail(GNX_ERR_INVALID_ARG, "d and cols must be >= 1");
  if (!ws || ws_bytes < gnx_xent_workspace_bytes(cols)) return fail(GNX_ERR_WORKSPACE, "workspace missing or too small");
  return launch_xent(logits, targets, d, cols, loss_out, static_cast<float*>(ws), (hipStream_t)stream);
}

int32_t gnx_logit_cross_entropy_backward(const float* logits, const float* targets, int32_t d, int64_t cols, const float* upstream,
                                         float* d_logits, void* stream) {
  if (!logits || !targets || !upstream || !d_logits) return fail(GNX_ERR_INVALID_ARG, "NULL argument");
  if (d <= 0 || cols <= 0) return fail(GNX_ERR_INVALID_ARG, "d and cols must be >= 1");
  return launch_xent_backward(logits, targets, d, cols, upstream, d_logits, (hipStream_t)stream);
}

int32_t gnx_collapse_edges(const gnx_graphs* h, const float* ef, int32_t d, int64_t R, float* out, void* stream) {
  if (!h) return fail(GNX_ERR_INVALID_ARG, "NULL argument");
  if (d <= 0 || R <= 0 || (R > 1 && h->G != 1) || R > 65535) return fail(GNX_ERR_INVALID_ARG, "bad d / n_replicas");
  int32_t rc = gnx_ensure_collapse(h);
  if (rc) return rc;
  if (h->E == 0) return GNX_OK;  // a batch without edges: no collapsed column, nothing to write (ef / out may be NULL)
  if (!ef || !out) return fail(GNX_ERR_INVALID_ARG, "NULL argument");
  return launch_collapse(h, ef, d, R, out, (hipStream_t)stream);
}

int32_t gnx_collapse_padded(const gnx_graphs* h, const float* ef, int32_t d, int64_t R, float* out, void* stream) {
  if (!h || !out || (!ef && h->E > 0)) return fail(GNX_ERR_INVALID_ARG, "NULL argument");
  if (d <= 0 || R <= 0 || (R > 1 && h->G != 1) || R > 65535 || h->G > 65535) return fail(GNX_ERR_INVALID_ARG, "bad d / n_replicas / more than 65535 graphs");
  if ((size_t)h->PN * (h->PN + 1) / 2 * (size_t)d >= ((size_t)1 << 31) * 256) return fail(GNX_ERR_TOO_LARGE, "padded triangle too large");
  return launch_collapse_padded(h, ef, d, R, out, (hipStream_t)stream);
}

int32_t gnx_fn_input(const gnx_graphs* h, int32_t kind, const float* ef, int32_t de, const float* nf, int32_t dn, const float* gf,
                     int32_t dg, int64_t R, float* out, void* stream) {
  if (!h) return fail(GNX_ERR_INVALID_ARG, "NULL handle or output");
  if (kind < 0 || kind > 2) return fail(GNX_ERR_INVALID_ARG, "kind must be 0 (edge), 1 (node) or 2 (graph)");
  if (kind == 0 && h->E == 0 && de >= 0 && dn >= 0 && dg >= 0) return GNX_OK;  // the edge function input of a batch without edges has no rows (out may be NULL)
  if (!out) return fail(GNX_ERR_INVALID_ARG, "NULL handle or output");
  if (de < 0 || dn < 0 || dg < 0) return fail(GNX_ERR_DIMS, "negative feature width");
  if (!ef && h->E > 0) de = 0;  // (a batch without edges: its (de, 0) edge features have no buffer — the sums over them are rows of de zeros, as in the reference)
  if (!nf) dn = 0;
  if (!gf) dg = 0;
  if (de + dn + dg == 0) return fail(GNX_ERR_ALL_NOTHING, "ef, nf and gf are all nothing");
  if (kind >= 1 && de == 0) return fail(GNX_ERR_INVALID_ARG, "node / graph function inputs need the updated edge features (nodefninput.jl, graphfninput.jl)");
  if (kind == 2 && dn == 0) return fail(GNX_ERR_INVALID_ARG, "the graph function input needs the updated node features (graphfninput.jl:1-13)");
  if (R <= 0 || (R > 1 && h->G != 1) || R > 65535) return fail(GNX_ERR_INVALID_ARG, "bad n_replicas");
  return launch_fn_input(h, kind, ef, de, nf, dn, gf, dg, R, out, (hipStream_t)stream);
}

int32_t gnx_profile_calibrate(int32_t n, void* stream) { return launch_calibration(n, (hipStream_t)stream); }

int32_t gnx_unpad_features(const gnx_graphs* h, int32_t kind, const float* padded, int32_t d, int64_t R, float* packed, void* stream) {
  return pad_impl(h, kind, false, padded, d, R, packed, stream);
}

}  // extern "C"
