// Everything about a call of a GNBlock with Chain update functions that is arithmetic on counts and widths: the shape of the call, the two fused
// rules with the LDS plans behind them, the fused mask, the two native bf16 rules, and the workspace layouts.  Plain C++17 host code — no HIP, nothing of a handle but
// its three counts — so that tests/test_chain_plan_cpu.py compiles it alone.  The plans of a call (ChainPlan, gnx_staging.h) are built from these.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "gnx.h"

namespace gnx {

// a Chain's layer entries (include/gnx.h: gnx_dense.kind): Dense or a LayerNorm(d) layer value (gamma, beta in weight, bias; eps = Flux's default)
constexpr float kChainLnEps = 1e-5f;
constexpr int kChainMaxLayers = 16;
inline bool chain_layer_is_ln(const gnx_dense& l) { return (l.kind & 0xff) == GNX_LAYER_LAYERNORM; }
inline int chain_layer_ln_mode(const gnx_dense& l) { return (l.kind & GNX_LAYER_LN_SQRT_EPS) ? 1 : 0; }
// a `Dropout(p)` layer value (GNX_LAYER_DROPOUT): only the training entries admit it (include/gnx.h), with p > 0 — it has no parameters, its
// width is its input's.  In a training call's own copy of a chain the entry's `bias` points at its ChainDropSite.
inline bool chain_layer_is_dropout(const gnx_dense& l) { return (l.kind & 0xff) == GNX_LAYER_DROPOUT; }
struct ChainDropSite { uint64_t seed; float p; uint32_t stream; };  // stream: 16 + 16 * function + layer, indices of the CALLER's chain
inline const ChainDropSite* chain_drop_site(const gnx_dense& l) { return reinterpret_cast<const ChainDropSite*>(l.bias); }
inline bool chain_has_dropout(const gnx_chain& c) {
  for (int i = 0; c.layers && i < c.n_layers; ++i)
    if (chain_layer_is_dropout(c.layers[i])) return true;
  return false;
}

// ---- the shape of a call: built once from the counts, the (checked) parameters and the replicas ----
struct ChainShape {
  const gnx_chain* ch[3];  // edge, node, graph function
  int de, dn, dg;
  int ow[3];               // oe, on, og: the width of each function's last layer, 0 without layers
  int k0[3];               // Ke, Kn, Kg: the width of each function's input row
  int maxw[3];             // the largest layer width of each function
  size_t trows[3], rows[3];  // E, N, G and R times them
  int64_t R;
  bool wide;               // any input or layer width at matrix-core widths (> 32)
  gnx_block_params edge_block;  // the one-layer block that performs the edge function's first Dense (an edge function with layers)
};
inline ChainShape chain_shape(int64_t E, int64_t N, int64_t G, const gnx_chain_block_params& p, int64_t R) {
  ChainShape s{};
  s.ch[0] = &p.edgefn; s.ch[1] = &p.nodefn; s.ch[2] = &p.graphfn;
  s.de = p.de; s.dn = p.dn; s.dg = p.dg;
  s.R = R;
  s.wide = p.de > 32 || p.dn > 32 || p.dg > 32;
  const int64_t t[3] = {E, N, G};
  for (int i = 0; i < 3; ++i) {
    const gnx_chain& c = *s.ch[i];
    s.ow[i] = c.n_layers > 0 ? c.widths[c.n_layers - 1] : 0;
    for (int l = 0; l < c.n_layers; ++l) s.maxw[i] = std::max(s.maxw[i], (int)c.widths[l]);
    s.wide = s.wide || s.maxw[i] > 32;
    s.trows[i] = (size_t)t[i];
    s.rows[i] = (size_t)R * (size_t)t[i];
  }
  s.k0[0] = p.de + 2 * p.dn + p.dg; s.k0[1] = s.ow[0] + p.dn + p.dg; s.k0[2] = s.ow[0] + s.ow[1] + p.dg;
  if (p.edgefn.n_layers > 0) {
    s.edge_block.de = p.de; s.edge_block.dn = p.dn; s.edge_block.dg = p.dg;
    s.edge_block.oe = p.edgefn.widths[0];
    s.edge_block.edgefn = p.edgefn.layers[0];
  }
  return s;
}

// ---- the fused rules (include/gnx.h states them) ----
constexpr int kChainNarrowMaxWidth = 32;         // input width and every layer width of a fused function
constexpr size_t kChainNarrowLdsFloats = 10240;  // the forward's zero-padded parameters in LDS: 40 KB
constexpr int kChainBwLdsFloats = 16384;         // the pullback's parameters + every wave's tape and accumulators: 64 KB

constexpr int ceil4(int x) { return (x + 3) & ~3; }  // (constexpr: callable from the kernels as it stands)
// floats a layer's parameters take in LDS (chain_stage_params, gnx_chain_mlp.h)
constexpr int chain_layer_par_floats(int kin, int width, bool ln) { return ln ? 2 * ceil4(width) : ceil4(kin) * ceil4(width) + ceil4(width); }

// floats of LDS the parameters of `c` take in the forward kernel's layout (input width k_in)
inline size_t chain_narrow_lds_floats(const gnx_chain& c, int k_in) {
  size_t n = 0;
  int kin = k_in;
  for (int i = 0; i < c.n_layers; ++i) {
    const int OP = ceil4(c.widths[i]);
    if (!chain_layer_is_dropout(c.layers[i])) n += chain_layer_is_ln(c.layers[i]) ? 2 * (size_t)OP : (size_t)ceil4(kin) * OP + OP;  // (a Dropout entry stages nothing)
    kin = c.widths[i];
  }
  return n;
}
// is the function fused by gnx_chain_block_forward_narrow: >= 1 layer, a non-zero output width, k_in and every width <= 32, parameters within
// the LDS budget, rows to run on.  With Dropout entries (a training call): the training forward's rule — the same, an entry staging 0 floats
inline bool chain_narrow_takes(const gnx_chain& c, int k_in, size_t entity_rows) {
  if (c.n_layers < 1 || c.n_layers > kChainMaxLayers || !c.layers || !c.widths || entity_rows == 0) return false;
  if (c.widths[c.n_layers - 1] <= 0 || k_in > kChainNarrowMaxWidth) return false;
  for (int i = 0; i < c.n_layers; ++i)
    if (c.widths[i] > kChainNarrowMaxWidth) return false;
  return chain_narrow_lds_floats(c, k_in) <= kChainNarrowLdsFloats;
}

// the pullback kernel's LDS plan for a function: the staged parameters, then per wave 64 tape rows of `ld` floats (the input row, every layer's
// output but the last, the parked deltas) and P accumulators (one per parameter)
struct ChainBwNarrowShape {
  int ld, P, par_floats, waves, dslot;  // waves: per workgroup, as many as fit 64 KB of LDS, at most 4 — the rule takes a function from 2 on
  int par_off[kChainMaxLayers], part_off[kChainMaxLayers], tape_out[kChainMaxLayers];  // per layer: staged parameters / accumulators / output slot
  size_t nwg;                           // workgroups (= partial rows per layer) per replica: a wave takes 64 rows
};
inline ChainBwNarrowShape chain_bw_narrow_shape(const gnx_chain& c, int k_in, size_t rows) {
  ChainBwNarrowShape sh{};
  int kin = k_in, slots = k_in, dmax = 0;
  for (int i = 0; i < c.n_layers; ++i) {
    const bool ln = chain_layer_is_ln(c.layers[i]), drop = chain_layer_is_dropout(c.layers[i]);
    const int J = c.widths[i];
    sh.par_off[i] = sh.par_floats;
    sh.part_off[i] = sh.P;
    if (!drop) {  // (a Dropout entry: no parameters, no accumulators, nothing parked in the delta slot — only its tape slot)
      sh.par_floats += chain_layer_par_floats(kin, J, ln);
      sh.P += ln ? 2 * J : J * (kin + 1);
      dmax = std::max(dmax, ln ? 2 * J : J);
    }
    sh.tape_out[i] = slots;
    if (i + 1 < c.n_layers) slots += J;
    kin = J;
  }
  sh.dslot = slots;
  sh.ld = (slots + dmax) | 1;
  const int per_wave = 64 * sh.ld + sh.P;
  sh.waves = std::min(4, std::max(0, (kChainBwLdsFloats - sh.par_floats) / per_wave));
  if (sh.waves > 0) sh.nwg = (rows + 64 * (size_t)sh.waves - 1) / (64 * (size_t)sh.waves);
  return sh;
}
// (with Dropout entries: the training pullback's rule, include/gnx.h)
// the rule of gnx_chain_block_backward_narrow for one function: the forward's rule and two waves per workgroup at least.  The one-wave class (a
// tape and accumulators beyond 28 KB) is cut — measured, it re-stages its parameters for every 64 rows, writes a partial row per 64 rows and
// misses the generic pullback's time (profiles/chain_bw_narrow.json)
inline bool chain_bw_narrow_takes(const gnx_chain& c, int k_in, size_t entity_rows) {
  return chain_narrow_takes(c, k_in, entity_rows) && chain_bw_narrow_shape(c, k_in, entity_rows).waves >= 2;
}

// The class CUT from the training pullback's rule: an EDGE function with Dropout entries at register width 32 (k_in or a layer width beyond
// 16).  Measured (profiles/chain_train_narrow.json): k_chain_mlp_bw_train<32, SRC_EDGE> takes 256 VGPRs and both of its measured cases —
// [16,do,3] at k_in 20 on the 1M-edge batch and on C2 — were slower than the generic test-mode pullback beyond its spread (2.02 against 1.02 ms,
// 5.18 against 4.16 ms).  Such a function runs the generic training launches.
inline bool chain_train_bw_cut(const gnx_chain& c, int k_in, int function) {
  if (function != 0 || !chain_has_dropout(c)) return false;
  int w = k_in;
  for (int i = 0; i < c.n_layers; ++i) w = std::max(w, (int)c.widths[i]);
  return w > 16;
}

enum ChainRule { CHAIN_RULE_FW, CHAIN_RULE_BW };
inline bool chain_rule_takes(ChainRule rule, const gnx_chain& c, int k_in, size_t rows) { return rule == CHAIN_RULE_FW ? chain_narrow_takes(c, k_in, rows) : chain_bw_narrow_takes(c, k_in, rows); }
// the functions of a block that `rule` runs in one kernel each: bit 0 edge, 1 node, 2 graph.  `s`: the shape of the caller's own parameters
// (a LayerNorm-first edge function is asked as it stands, before the identity layer of ChainLnFirst)
inline unsigned chain_fused_mask(const ChainShape& s, ChainRule rule) {
  unsigned m = 0;
  for (int t = 0; t < 3; ++t)
    if (chain_rule_takes(rule, *s.ch[t], s.k0[t], s.trows[t]) && !(rule == CHAIN_RULE_BW && chain_train_bw_cut(*s.ch[t], s.k0[t], t))) m |= 1u << t;
  return m;
}

// bfloat16 features, the forward's native path: every update function with an output and rows to run on is inside the fused rule — then each
// runs as one k_chain_mlp_bf16 launch on the bf16 rows and nothing of the block is widened or rounded by a pass of its own
inline bool chain_typed_native(const ChainShape& s, unsigned fused) {
  for (int t = 0; t < 3; ++t)
    if (s.ow[t] > 0 && s.trows[t] > 0 && !(fused & (1u << t))) return false;
  return true;
}
// ... and the fp32 rows it keeps behind the fp32 layout for a later function of the call — 0: ef' for the node / graph function, 1: nf' and 2: the
// widened gf for the graph function
inline void chain_native_counts(const ChainShape& s, size_t counts[3]) {
  const int oe = s.ow[0], on = s.ow[1], og = s.ow[2];
  counts[0] = on > 0 || og > 0 ? s.rows[0] * oe : 0;
  counts[1] = og > 0 ? s.rows[1] * on : 0;
  counts[2] = og > 0 ? s.rows[2] * s.dg : 0;
}

// The pullback of a generic graph function behind a fused node function: nf' is recomputed by the generic launches (Xn and every layer's output
// kept), so that the graph function's input — and with it its parameter gradients — keeps gnx_chain_block_backward's bits.
inline bool chain_bw_node_fw_generic(unsigned fused, int og) { return (fused & 2) && og > 0 && !(fused & 4); }

// ---- the workspace layouts: every carve 256-B aligned, in the order taken ----
struct ChainCarve { size_t off, bytes; };
struct ChainCarver {
  size_t o = 0;
  static size_t up(size_t x) { return (x + 255) / 256 * 256; }
  ChainCarve bytes(size_t n) { const ChainCarve c{o, n}; o += up(n); return c; }
  ChainCarve floats(size_t n) { return bytes(sizeof(float) * n); }
};

// The forward (gnx_chain_block_forward: fused = 0; _narrow: the mask of CHAIN_RULE_FW).  A fused function has its rows in registers: none of the
// block workspace / e_buf, n_in / n_buf, g_buf.  block_bytes: gnx_block_workspace_bytes of s.edge_block for a generic edge function with an output, else 0.
struct ChainWs {
  ChainCarve block, e_buf[2], n_in, n_buf[2], g_in, g_buf[2];
  ChainCarve ident;  // the identity layer of a LayerNorm-first edge function (ChainLnFirst)
  size_t total;
};
inline ChainWs chain_fw_layout(const ChainShape& s, unsigned fused, size_t ident_floats, size_t block_bytes) {
  ChainWs w{};
  ChainCarver c;
  const int on = s.ow[1], og = s.ow[2];
  w.block = c.bytes(block_bytes);
  for (int i = 0; i < 2; ++i) w.e_buf[i] = c.floats(s.ch[0]->n_layers > 1 && !(fused & 1) ? s.rows[0] * s.maxw[0] : 0);
  w.n_in = c.floats(on > 0 && !(fused & 2) ? s.rows[1] * (size_t)s.k0[1] : 0);
  for (int i = 0; i < 2; ++i) w.n_buf[i] = c.floats(s.ch[1]->n_layers > 1 && !(fused & 2) ? s.rows[1] * s.maxw[1] : 0);
  w.g_in = c.floats(og > 0 ? s.rows[2] * (size_t)s.k0[2] : 0);
  for (int i = 0; i < 2; ++i) w.g_buf[i] = c.floats(s.ch[2]->n_layers > 1 && !(fused & 4) ? s.rows[2] * s.maxw[2] : 0);
  w.ident = c.floats(ident_floats);
  w.total = c.o + 256;
  return w;
}
// what the forward's row-wise layers read of the handle: the matrix-core tables (a fused edge function reads every edge's destination from them)
inline bool chain_fw_reads_wide_tables(const ChainShape& s, unsigned fused) {
  const bool rows_e = !(fused & 1) && (s.ch[0]->n_layers > 1 || s.ow[0] == 0);
  const bool rows_n = !(fused & 2) && s.ch[1]->n_layers > 1, rows_g = !(fused & 4) && s.ch[2]->n_layers > 1;
  return rows_e || rows_n || rows_g || (fused & 1);
}

// The pullback (gnx_chain_block_backward: fused = 0; _narrow: the mask of CHAIN_RULE_BW).  A fused function keeps no per-layer outputs, no delta
// buffers and (the edge function) no inner block workspaces; it adds its partial rows and (the edge function) the compact [R E][2 dn + dg] input
// gradient.  blk_fw_bytes / blk_bw_bytes: gnx_block_workspace_bytes / gnx_block_backward_workspace_bytes of s.edge_block unless the edge
// function is fused; chunk: BW_CH, the rows per partial of the generic weight-gradient reduction; dw_partial(rows, J, K): dw_mfma_partial_floats.
struct ChainBwLayout {
  ChainCarve act[3][kChainMaxLayers + 1];  // stored layer outputs per chain (a fused chain: its last layer's, where a level above reads it)
  ChainCarve Xn, dXn, Xg, dXg, gbuf[3], blk_fw, blk_bw, part, wt, off2, ident, dxe;
  size_t total;
};
template <class DwPartial>
inline ChainBwLayout chain_bw_layout(const ChainShape& s, unsigned fused, size_t ident_floats, size_t blk_fw_bytes, size_t blk_bw_bytes, size_t chunk, DwPartial dw_partial) {
  ChainBwLayout L{};
  ChainCarver c;
  const int oe = s.ow[0], on = s.ow[1], og = s.ow[2];
  const int Kn = s.k0[1], Kg = s.k0[2];
  size_t gmax = 1, pmax = 2048 * 4, wmax = 1;
  for (int t = 0; t < 3; ++t) {
    const gnx_chain& ch = *s.ch[t];
    if (fused & (1u << t)) {
      const bool crosses = t == 0 ? on > 0 || og > 0 : t == 1 && og > 0;  // ef' feeds the node / graph inputs, nf' the graph input
      if (t == 1 && chain_bw_node_fw_generic(fused, og)) {
        for (int i = 0; i < ch.n_layers; ++i) L.act[t][i] = c.floats(s.rows[t] * (size_t)ch.widths[i]);
      } else if (crosses) L.act[t][ch.n_layers - 1] = c.floats(s.rows[t] * (size_t)s.ow[t]);
      const ChainBwNarrowShape sh = chain_bw_narrow_shape(ch, s.k0[t], s.trows[t]);
      pmax = std::max(pmax, (size_t)sh.P * sh.nwg * (size_t)s.R);
      continue;
    }
    for (int i = 0; i < ch.n_layers; ++i) {
      L.act[t][i] = c.floats(s.rows[t] * (size_t)ch.widths[i]);
      const int J = ch.widths[i], K = i > 0 ? ch.widths[i - 1] : s.k0[t];
      const size_t chunks = (s.rows[t] + chunk - 1) / chunk;
      pmax = std::max({pmax, chunks * (size_t)J * (K + 1), (size_t)2048 * J, (size_t)dw_partial(s.rows[t], J, K)});
      wmax = std::max(wmax, (size_t)J * K);
    }
    gmax = std::max(gmax, s.rows[t] * (size_t)s.maxw[t]);
  }
  pmax = std::max(pmax, std::max(s.rows[2] * 256, (size_t)2048) * (size_t)std::max({s.dg, oe, 1}));  // column-sum slices
  L.Xn = c.floats(on > 0 && (!(fused & 2) || chain_bw_node_fw_generic(fused, og)) ? s.rows[1] * Kn : 0); L.dXn = c.floats(on > 0 ? s.rows[1] * Kn : 0);
  L.Xg = c.floats(og > 0 ? s.rows[2] * Kg : 0); L.dXg = c.floats(og > 0 ? s.rows[2] * Kg : 0);
  const bool all_fused = (oe == 0 || (fused & 1)) && (on == 0 || (fused & 2)) && (og == 0 || (fused & 4)) && fused != 0;
  for (int i = 0; i < 3; ++i) L.gbuf[i] = c.floats(all_fused ? 0 : gmax);
  L.blk_fw = c.bytes(blk_fw_bytes); L.blk_bw = c.bytes(blk_bw_bytes);
  L.part = c.floats(pmax); L.wt = c.floats(wmax); L.off2 = c.floats(16);
  L.ident = c.floats(ident_floats);
  L.dxe = c.floats((fused & 1) ? s.rows[0] * (size_t)(2 * s.dn + s.dg) : 0);
  L.total = c.o + 256;
  return L;
}

// bfloat16 features, the pullback's native path (gnx_chain_block_backward_narrow_typed): the edge function has an output and edges to run on
// (there is no pullback without), and every update function with an output and rows to run on is inside the pullback's fused rule (`fused`: the
// mask of CHAIN_RULE_BW).  Then every function is one k_chain_mlp_bw_bf16 launch on the bf16 rows, chain_bw_node_fw_generic cannot occur, and no
// E- or N-sized tensor is widened or rounded by a pass of its own.  A mixed mask stays staged.
inline bool chain_bw_typed_native(const ChainShape& s, unsigned fused, bool bf16) {
  return bf16 && s.ow[0] > 0 && s.trows[0] > 0 && chain_typed_native(s, fused);
}
// ... and its workspace: the fp32 narrow layout (chain_bw_layout with the same mask, fp32_total bytes) and behind it two graph-sized fp32 carves
// of R G dg floats — the widened gf, which the graph function's input rows (Xg) are assembled from, and the fp32 d_gf the per-graph column sums
// accumulate into before it is rounded once.  (The upstream gradients are read as bf16 by the kernels: none is widened.)
struct ChainBwNativeWs { ChainCarve gf32, dgf32; size_t total; };
inline ChainBwNativeWs chain_bw_native_layout(const ChainShape& s, size_t fp32_total) {
  ChainBwNativeWs w{};
  ChainCarver c;
  c.o = ChainCarver::up(fp32_total);
  w.gf32 = c.floats(s.ow[2] > 0 ? s.rows[2] * (size_t)s.dg : 0);
  w.dgf32 = c.floats(s.rows[2] * (size_t)s.dg);
  w.total = c.o;
  return w;
}

}  // namespace gnx
