// Host plumbing the entry points of gnx_forward.hip, gnx_backward.hip and gnx_chain.cpp share: the workspace and bf16-alignment checks of a call, the
// staging of a bf16 call that converts around an fp32 path (widen into the workspace, run fp32, round the outputs), and what the Chain block's
// forward and pullback decide in common about a call (ChainPlan; defined in gnx_chain.cpp).  No kernel here.
#pragma once
#include <algorithm>

#include "gnx_launchers.h"

namespace gnx {

// the workspace of a call against `total`, the size its query returns (`message`: "workspace missing or smaller than <that query>()")
inline int32_t check_ws(const void* ws, size_t ws_bytes, size_t total, const char* message) {
  if (!ws || ws_bytes < total) return fail(GNX_ERR_WORKSPACE, message);
  if (((uintptr_t)ws & 15) != 0) return fail(GNX_ERR_WORKSPACE, "workspace must be 16-byte aligned");
  return GNX_OK;
}

// the feature buffers of a bf16 call (NULL passes): rows of odd width are then 2-byte aligned, which is all the kernels assume
inline int32_t check_bf16_aligned(const void* const* bufs, int n) {
  for (int i = 0; i < n; ++i)
    if (((uintptr_t)bufs[i] & 3) != 0) return fail(GNX_ERR_INVALID_ARG, "bf16 feature buffers must be 4-byte aligned");
  return GNX_OK;
}

// fp32 copies of up to 12 tensors behind a base layout (the fp32 path's own workspace, bytes [0, base)), each carve 256-B aligned
struct Staging {
  size_t base, off[12], n[12], total;  // n: elements of copy i (0: absent)
  float* at(void* ws, int i) const { return reinterpret_cast<float*>(static_cast<char*>(ws) + off[i]); }
};
// k == 0: a call that stages nothing (a native bf16 path) — its workspace is the base layout's, to the byte
inline Staging stage_layout(size_t base_total, const size_t* counts, int k) {
  Staging w{};
  w.base = base_total;
  size_t o = align_up(base_total, 256);
  for (int i = 0; i < k; ++i) {
    w.n[i] = counts[i];
    w.off[i] = o;
    o += align_up(sizeof(float) * counts[i], 256);
  }
  w.total = k ? o : base_total;
  return w;
}
// ... of feature tensors: copy i has the rows of entity i % 3 (edges, nodes, graphs; times R) and width[i] columns
inline Staging stage_features(size_t base_total, const gnx_graphs* h, int64_t R, const int* width, int k) {
  const int64_t rows[3] = {h->E, h->N, h->G};
  size_t counts[12];
  for (int i = 0; i < k; ++i) counts[i] = (size_t)R * (size_t)rows[i % 3] * (size_t)std::max(width[i], 0);
  return stage_layout(base_total, counts, k);
}
// widen bufs[first, last) into their copies / round the copies back into bufs[first, last); a NULL buffer or an empty tensor is skipped
inline int32_t stage_widen(const Staging& st, void* ws, const void* const* bufs, int first, int last, hipStream_t s) {
  for (int i = first; i < last; ++i)
    if (bufs[i] && st.n[i] > 0)
      if (const int32_t rc = launch_bf16_widen(bufs[i], st.n[i], st.at(ws, i), s)) return rc;
  return GNX_OK;
}
// (the outputs stand in the caller's one list of buffers, which is const for its inputs' sake)
inline int32_t stage_round(const Staging& st, void* ws, const void* const* bufs, int first, int last, hipStream_t s) {
  for (int i = first; i < last; ++i)
    if (bufs[i] && st.n[i] > 0)
      if (const int32_t rc = launch_bf16_round(st.at(ws, i), st.n[i], const_cast<void*>(bufs[i]), s)) return rc;
  return GNX_OK;
}

// ---- a call of a GNBlock with Chain update functions (gnx_chain.cpp: the forward entries; gnx_backward.hip: the pullbacks) ----
// What is decided about such a call from the handle's counts alone, decided once, by a query and by a call from the same arguments: the validation,
// the fused mask of `rule` (0 unless `narrow`), the LayerNorm-first rewrite (ChainLnFirst: a generic edge function that opens with a LayerNorm runs
// behind an identity Dense, a fused one as it stands; p: the parameters every launch works on, sh: their shape) and the query whose name the
// workspace refusal cites (query_of: the plain, the narrow, the typed entry's).  The forward and the pullback derive their plan from it
// (ChainFwPlan, ChainBwPlan) and add their layout, which sized() completes.  Not copyable (ChainLnFirst is not): `p` may point into `lnf`.
// `train`: the call came through a training entry (ChainTrain below) — its chains may hold Dropout entries.
struct ChainPlan {
  ChainPlan(const gnx_graphs* h, const gnx_chain_block_params* p0, int64_t R, int32_t elem, bool narrow, ChainRule rule, const char* const query_of[3],
            bool train = false);
  int32_t rc;  // the validation's; not GNX_OK: nothing below is set
  ChainLnFirst lnf;
  const gnx_chain_block_params* p = nullptr;
  ChainShape sh{};
  unsigned fused = 0;
  bool bf16 = false;
  Staging st{};                // a bf16 call: the fp32 carves behind the fp32 layout
  size_t base = 0, total = 0;  // the fp32 layout's total; what the entry's _workspace_bytes returns
  const char* query = nullptr;
  // a call binds the identity layer of the rewrite to its carve of the workspace: in the chain and in the one-layer block that is its copy
  void bind_ident(const float* ident) { if (lnf.on) { lnf.layers[0].weight = ident; sh.edge_block.edgefn.weight = ident; } }
  void sized(size_t fp32_total, const Staging& staging) { base = fp32_total; st = staging; total = bf16 ? st.total : base; }
};
// "an input with non-zero width is NULL": one check behind every Chain entry, each with its own message
int32_t chain_check_features(const ChainShape& sh, const void* ef, const void* nf, const void* gf, const char* message);

// What a training entry (gnx_chain_block_forward_train / _backward_train and their queries; include/gnx.h) makes of the caller's chains before it
// plans: the refusals of the record and of the Dropout entries in their documented order, then the library's own copy of the three chains — the
// entries with p = 0 (all of them without a record) removed, each entry that stays bound to its ChainDropSite (the seed, p and the stream id of
// the CALLER's indices) through its `bias` field.  active: an entry stayed — the call runs the training launches on `p`; otherwise `p` is the
// stripped chain and the call IS the mirrored test-mode entry on it.  every_entry: keep every Dropout entry whatever its p (the rule's query,
// gnx_chain_block_train_applies).  Not copyable: `p` points into it.  Defined in gnx_chain.cpp.
struct ChainTrain {
  ChainTrain(const gnx_chain_block_params* p0, const gnx_chain_dropout* d, bool every_entry = false);
  ChainTrain(const ChainTrain&) = delete;
  ChainTrain& operator=(const ChainTrain&) = delete;
  int32_t rc = GNX_OK;
  bool active = false;
  gnx_chain_block_params p{};
  gnx_dense layers[3][kChainMaxLayers];
  int32_t widths[3][kChainMaxLayers];
  int src[3][kChainMaxLayers];  // the caller's index of layer i of `p`
  ChainDropSite sites[3][kChainMaxLayers];
  gnx_dense_grad g[3][kChainMaxLayers];
  gnx_chain_block_grads grads{};
  // the caller's gradient slots in the order of `p` (a Dropout entry's: none)
  const gnx_chain_block_grads* map_grads(const gnx_chain_block_grads* g0);
};

}  // namespace gnx
