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

// ---- the wide form (gnx_chain_block_forward_wide; gnx_chain_wide.hip): one update function at matrix-core widths in one kernel ----
constexpr int kChainWideMaxWidth = 128;    // input width and every layer width of a function the kernel takes
constexpr int kChainWideLdsFloats = 16384; // the weight chunk, the bias row and every wave's slice: 64 KB
constexpr int kChainWideRows = 32;         // rows a wave owns through all layers
constexpr int ceil16(int x) { return (x + 15) & ~15; }
constexpr int ceil32(int x) { return (x + 31) & ~31; }
// The LDS plan of k_chain_wide, in floats: the weight chunk — 16 reduction steps of the widest Dense as three bf16 planes [3][np][16] — then the
// bias row [np], then per wave a slice [32][ld] fp32 that holds the wave's rows through all layers.  ld: odd, from the largest 16-padded width.
// waves: per workgroup, as many slices as fit 64 KB, at most 4 — the rule takes a function from 2 on.  nb: 32-column accumulator blocks of the
// widest Dense (the kernel's template class: 1 or 2 inside the rule; 3 and 4 count as 4, the class chain_wide_cut cuts).
struct ChainWideShape {
  int ld, waves, nb, np, chunk_floats, bias_off, slice_off, floats;
  size_t nwg;  // workgroups per replica: a wave takes 32 rows
};
inline ChainWideShape chain_wide_shape(const gnx_chain& c, int k_in, size_t rows) {
  ChainWideShape w{};
  int maxw = k_in, maxd = 1;
  for (int i = 0; i < c.n_layers; ++i) {
    maxw = std::max(maxw, (int)c.widths[i]);
    if (!chain_layer_is_ln(c.layers[i]) && !chain_layer_is_dropout(c.layers[i])) maxd = std::max(maxd, (int)c.widths[i]);
  }
  w.ld = ceil16(maxw) | 1;
  w.np = ceil32(maxd);
  w.nb = w.np / 32 == 3 ? 4 : w.np / 32;
  w.chunk_floats = 3 * w.np * 8;  // (16 bf16 = 8 floats per column and plane)
  w.bias_off = w.chunk_floats;
  w.slice_off = w.bias_off + w.np;
  w.waves = std::min(4, std::max(0, (kChainWideLdsFloats - w.slice_off) / (kChainWideRows * w.ld)));
  w.floats = w.slice_off + w.waves * kChainWideRows * w.ld;
  if (w.waves > 0) w.nwg = (rows + (size_t)kChainWideRows * w.waves - 1) / ((size_t)kChainWideRows * w.waves);
  return w;
}
// The class CUT from the wide rule: a widest Dense beyond 64 columns (three or four accumulator blocks), in either source form, on one graph and
// on several.  Measured (profiles/chain_wide.json, whole calls, cache-cold, medians of 15, against the parent's gnx_chain_block_forward; the
// record was taken before the cut): its instantiation took 200 VGPRs + 64 AGPRs — one workgroup of three waves per CU — and on the 512-graph
// 1M-edge batch (10,5,3) [128,ln,128,3]/[128,4]/[5] took 2.152 against 1.135 ms (spread 0.024), (32,32,8) [128,128,32]/[128,32]/[64,8] 3.563
// against 1.619 (0.035); on the one-graph 1M-edge batch 5.344 against 4.395 (0.131) and 49.94 against 48.04 (0.93).  The two-block class stays:
// (10,5,0) [64,3]/[64,4]/[32,5] 0.251 against 0.263 ms (0.027) and 3.457 against 3.453 (0.102), (10,5,3) [64,64,3]/[64,4]/[16,5] 0.371 against
// 0.416 (0.030) and 3.560 against 3.615 (0.090).  Not measured: the one-block class (every Dense at most 32 columns behind a wider input or
// LayerNorm), and the graph function's rows form on its own (its only case sat in a block whose edge and node function are of the cut class).
inline bool chain_wide_cut(const gnx_chain& c, int k_in) { return chain_wide_shape(c, k_in, 1).np > 64; }
// is the function run by k_chain_wide (gnx_chain_block_forward_wide; include/gnx.h states the rule): outside chain_narrow_takes; at least two
// Dense / LayerNorm entries and no Dropout entry; a non-zero output width and rows to run on; 1 <= k_in <= 128 and every layer width <= 128; the
// LDS plan above at two waves at least; not of the class chain_wide_cut names.
inline bool chain_wide_takes(const gnx_chain& c, int k_in, size_t entity_rows) {
  if (c.n_layers < 2 || c.n_layers > kChainMaxLayers || !c.layers || !c.widths || entity_rows == 0) return false;
  if (chain_narrow_takes(c, k_in, entity_rows) || chain_has_dropout(c)) return false;
  if (c.widths[c.n_layers - 1] <= 0 || k_in < 1 || k_in > kChainWideMaxWidth) return false;
  for (int i = 0; i < c.n_layers; ++i)
    if (c.widths[i] < 1 || c.widths[i] > kChainWideMaxWidth) return false;
  return chain_wide_shape(c, k_in, entity_rows).waves >= 2 && !chain_wide_cut(c, k_in);
}
// the functions of a block the wide kernel runs: bit 0 edge, 1 node, 2 graph.  `s`: the shape of the caller's own parameters
inline unsigned chain_wide_mask(const ChainShape& s) {
  unsigned m = 0;
  for (int t = 0; t < 3; ++t)
    if (chain_wide_takes(*s.ch[t], s.k0[t], s.trows[t])) m |= 1u << t;
  return m;
}

// ---- the wide form on bfloat16 features (gnx_chain_block_forward_wide_typed; gnx_chain_wide_bf16.hip) ----
// The LDS plan is ChainWideShape as it stands: the gathered bf16 row of an edge function that opens with a Dense lives in the memory of the wave's
// fp32 slice, which the first Dense overwrites only after its last chunk is read.  Its row stride, in bf16 elements: the 16-padded input width
// plus 8.  Why: a lane's A fragment is 8 consecutive reduction steps of row c31 at element 16 c + 8 hi, i.e. 16 bytes — the stride must be a
// multiple of 8 elements for that to be ONE aligned 16-byte read; and KP + 8 = 8 (2 j + 1) elements = 16 (2 j + 1) bytes is an ODD number of 16-byte
// columns, so the sixteen consecutive lanes (one hi, sixteen rows) that a 16-byte LDS read serves per pass fall on sixteen different 16-byte
// columns of the 64 four-byte banks (256 bytes): no conflict.  It fits: 32 (KP + 8) 2 bytes <= 32 (KP | 1) 4 bytes from KP = 6 on, and KP >= 16.
// (The pass model — 16 consecutive lanes per pass — is the assumption; the stride was not measured against another.)
constexpr int chain_wide_bf16_stride(int k_in) { return ceil16(k_in) + 8; }

// ---- the wide form of the pullback (gnx_chain_block_backward_wide; gnx_chain_bw_wide.hip): one update function at matrix-core widths pulled
//      back in one kernel ----
constexpr int kChainBwWideLdsFloats = 16384;  // the weight chunk, the bias row and every wave's tape: 64 KB, the project's budget — two such
                                              // workgroups share a CU's 160 KB, and no launch raises the dynamic-LDS attribute
constexpr int kChainBwWideGrid = 512;         // the persistent grid: workgroups per replica at the most, two per CU of an MI355X — the partial
                                              // rows of the parameter gradients are bounded by it, whatever the entity's rows
constexpr int kChainBwWideMaxLayers = 8;      // entries of a function (the kernel keeps four vector accumulators per entry in registers)
constexpr int kChainBwWideAcc = 4;            // 32 x 32 dW blocks a wave keeps in registers across tiles
constexpr int kChainBwWideMaxItems = 24;
// The plan of k_chain_bw_wide.  The tape of a row, in floats: the input row zero-padded to 16, then per entry its output padded to 16 (the
// entry's delta is later written over it), a gelu Dense's pre-activation padded to 16 or a LayerNorm's (mu, sigma + eps, q, -); 16 floats of
// slack (a 32-column fragment read of the last slot stays on the tape); ld odd.  LDS: the staged chunk [3][np][16] bf16, the bias row [np], then
// `waves` tapes of [32][ld].  block[]: the dW blocks (entry, 32 rows k, 32 columns j), block b kept by wave b % waves in register slot b / waves.
// item[]: the runs of staged chunks in the order the kernel consumes them — forward: a Dense's [kin][width] in chunks of 16 k; way back: its
// transpose in chunks of 16 j, one run per pass of np input columns (entry 0 only where the caller wants the input gradient: `with_dx0`).
struct ChainBwWideShape {
  int ld, P, waves, nb, np, chunk_floats, bias_off, tape_off, floats, n_blocks, n_items, n_items_dx0;
  int in_off[kChainBwWideMaxLayers], out_off[kChainBwWideMaxLayers], aux_off[kChainBwWideMaxLayers], part_off[kChainBwWideMaxLayers];
  unsigned char block[4 * kChainBwWideAcc][3];  // entry, kb, jb
  unsigned char item[kChainBwWideMaxItems][4];  // entry, transposed, pass, chunks; the first n_items without entry 0's way back, n_items_dx0 with it
  size_t ntiles, nwg;  // tiles of 32 * waves rows; workgroups (= partial rows per entry) per replica: min(ntiles, kChainBwWideGrid)
};
inline ChainBwWideShape chain_bw_wide_shape(const gnx_chain& c, int k_in, size_t rows) {
  ChainBwWideShape w{};
  if (c.n_layers > kChainBwWideMaxLayers) return w;  // (waves 0: outside)
  const ChainWideShape f = chain_wide_shape(c, k_in, rows);
  w.nb = f.nb; w.np = f.np;
  int slots = ceil16(k_in), kin = k_in, nblocks = 0;
  for (int i = 0; i < c.n_layers; ++i) {
    const bool ln = chain_layer_is_ln(c.layers[i]);
    const int J = c.widths[i];
    w.in_off[i] = i ? w.out_off[i - 1] : 0;
    w.out_off[i] = slots; slots += ceil16(J);
    w.aux_off[i] = slots;
    if (ln) slots += 4; else if (c.layers[i].act == GNX_ACT_GELU) slots += ceil16(J);
    w.part_off[i] = w.P;
    w.P += ln ? 2 * J : J * (kin + 1);
    if (!ln)
      for (int kb = 0; kb < ceil32(kin) / 32; ++kb)
        for (int jb = 0; jb < ceil32(J) / 32; ++jb, ++nblocks)
          if (nblocks < 4 * kChainBwWideAcc) { w.block[nblocks][0] = (unsigned char)i; w.block[nblocks][1] = (unsigned char)kb; w.block[nblocks][2] = (unsigned char)jb; }
    kin = J;
  }
  w.ld = (slots + 16) | 1;
  w.chunk_floats = 3 * w.np * 8;
  w.bias_off = w.chunk_floats;
  w.tape_off = w.bias_off + w.np;
  w.waves = std::min(4, std::max(0, (kChainBwWideLdsFloats - w.tape_off) / (kChainWideRows * w.ld)));
  if (w.waves < 2 || nblocks > w.waves * kChainBwWideAcc) { w.waves = 0; return w; }
  w.n_blocks = nblocks;
  w.floats = w.tape_off + w.waves * kChainWideRows * w.ld;
  auto item = [&](int i, int t, int pass, int chunks) {
    if (w.n_items_dx0 < kChainBwWideMaxItems) { unsigned char* it = w.item[w.n_items_dx0]; it[0] = (unsigned char)i; it[1] = (unsigned char)t; it[2] = (unsigned char)pass; it[3] = (unsigned char)chunks; }
    ++w.n_items_dx0;
  };
  kin = k_in;
  for (int i = 0; i < c.n_layers; kin = c.widths[i++])
    if (!chain_layer_is_ln(c.layers[i])) item(i, 0, 0, ceil16(kin) / 16);
  for (int i = c.n_layers - 1; i >= 0; --i) {
    if (i == 0) w.n_items = w.n_items_dx0;
    if (chain_layer_is_ln(c.layers[i])) continue;
    const int K = i ? c.widths[i - 1] : k_in;
    for (int pass = 0; pass * w.np < K; ++pass) item(i, 1, pass, ceil16(c.widths[i]) / 16);
  }
  if (w.n_items_dx0 > kChainBwWideMaxItems) { w.waves = 0; return w; }
  w.ntiles = (rows + (size_t)kChainWideRows * w.waves - 1) / ((size_t)kChainWideRows * w.waves);
  w.nwg = std::min(w.ntiles, (size_t)kChainBwWideGrid);
  return w;
}
// The rule of gnx_chain_block_backward_wide for one function (include/gnx.h states it): the forward's wide rule (chain_wide_takes, the class of
// chain_wide_cut outside), at most eight entries, and the plan above — two tapes at least within 64 KB, every dW block in a register slot.
// Measured classes and what was not measured: DESIGN.md, profiles/chain_bw_wide.json.
inline bool chain_bw_wide_takes(const gnx_chain& c, int k_in, size_t entity_rows) {
  return chain_wide_takes(c, k_in, entity_rows) && chain_bw_wide_shape(c, k_in, entity_rows).waves >= 2;
}
// the functions of a block the wide pullback kernel runs: bit 0 edge, 1 node, 2 graph (no pullback without an edge output)
inline unsigned chain_bw_wide_mask(const ChainShape& s) {
  unsigned m = 0;
  for (int t = 0; t < 3 && s.ow[0] > 0; ++t)
    if (chain_bw_wide_takes(*s.ch[t], s.k0[t], s.trows[t])) m |= 1u << t;
  return m;
}

// ---- the wave form (gnx_chain_block_forward_wave; gnx_chain_wave.hip): the edge and the node function in one wave-per-tile kernel ----
constexpr int kChainWaveLdsFloats = 16384;  // both functions' parameters + every wave's ef' rows: 64 KB
// floats between two ef' rows of a wave's LDS slice: odd, so that 64 lanes on 64 different rows of one column meet in no bank
constexpr int chain_wave_stride(int oe) { return oe | 1; }
// waves per workgroup: 4 where the parameters of both functions and four slices of [cap][stride(oe)] floats fit the LDS, else 2; 0: not even 2
inline int chain_wave_waves(const ChainShape& s, int cap) {
  const size_t par = chain_narrow_lds_floats(*s.ch[0], s.k0[0]) + chain_narrow_lds_floats(*s.ch[1], s.k0[1]);
  const size_t slice = (size_t)cap * chain_wave_stride(s.ow[0]);
  if (slice == 0 || par > kChainWaveLdsFloats) return 0;
  const size_t fit = (kChainWaveLdsFloats - par) / slice;
  return fit >= 4 ? 4 : (fit >= 2 ? 2 : 0);
}
// The class CUT from the wave rule: register width 32 (an input or layer width of the edge or the node function beyond 16) on a batch of SEVERAL
// graphs.  Measured (profiles/chain_wave.json, whole calls, cache-cold, against the parent's narrow entry): k_chain_wave<32> takes 179 VGPRs
// (two waves per SIMD) and on the 512-graph 1M-edge batch its three cases were slower than the parent beyond its spread — 0.207 against 0.107 ms
// (spread 0.004), 0.388 against 0.199 (0.005), 0.265 against 0.141 (0.006).  On the one-graph 1M-edge batch the same cases took 0.188 against
// 3.278 ms, 0.352 against 3.354, 0.241 against 3.294: there the class stays.  Register width 8 passed on both batches (0.066 against 0.077 ms,
// 0.075 against 2.106); register width 16 and the two-wave classes were not measured.
inline bool chain_wave_cut(const ChainShape& s) {
  return std::max({s.k0[0], s.k0[1], s.maxw[0], s.maxw[1]}) > 16 && s.trows[2] > 1;
}
// The rule (include/gnx.h states it).  `s`: the shape of the caller's own parameters; bf16: the call's features; max_in_degree / cap: the handle's
// largest in-degree and wave-tile edge cap — every wave tile is ONE chunk of at most `cap` edges exactly when no node has more in-edges.
inline bool chain_wave_takes(const ChainShape& s, bool bf16, int64_t max_in_degree, int cap) {
  if (bf16 || cap <= 0 || s.trows[0] == 0 || s.ow[0] <= 0 || s.ow[1] <= 0) return false;
  for (int t = 0; t < 3; ++t)
    if (chain_has_dropout(*s.ch[t])) return false;
  if (!chain_narrow_takes(*s.ch[0], s.k0[0], s.trows[0]) || !chain_narrow_takes(*s.ch[1], s.k0[1], s.trows[1])) return false;
  if (s.ch[2]->n_layers > 0 && !chain_narrow_takes(*s.ch[2], s.k0[2], s.trows[2])) return false;
  return max_in_degree <= cap && chain_wave_waves(s, cap) >= 2 && !chain_wave_cut(s);
}
// its partial rows: R x wave tiles x (oe + on) floats at the head of the workspace (a block without a graph function writes none)
inline size_t chain_wave_partial_floats(const ChainShape& s, int64_t n_wtiles) {
  return s.ow[2] > 0 ? (size_t)s.R * (size_t)n_wtiles * (size_t)(s.ow[0] + s.ow[1]) : 0;
}

// ---- the wave form on bfloat16 features (gnx_chain_block_forward_wave_typed; gnx_chain_wave_bf16.hip) ----
// A wave's LDS slice holds its ef' rows [cap][stride(oe)] and then, written over them, its nf' rows [64][stride(on)] on their way to the flat store
inline size_t chain_wave_typed_slice(const ChainShape& s, int cap) {
  return std::max((size_t)cap * chain_wave_stride(s.ow[0]), (size_t)64 * chain_wave_stride(s.ow[1]));
}
// waves per workgroup: chain_wave_waves with that slice
inline int chain_wave_typed_waves(const ChainShape& s, int cap) {
  const size_t par = chain_narrow_lds_floats(*s.ch[0], s.k0[0]) + chain_narrow_lds_floats(*s.ch[1], s.k0[1]);
  if (cap <= 0 || s.ow[0] <= 0 || par > kChainWaveLdsFloats) return 0;
  const size_t fit = (kChainWaveLdsFloats - par) / chain_wave_typed_slice(s, cap);
  return fit >= 4 ? 4 : (fit >= 2 ? 2 : 0);
}
// The rule: the fp32 form's conditions with the larger slice in the LDS term.  Measured (profiles/chain_wave_bf16.json, whole calls, cache-cold,
// against the parent's gnx_chain_block_forward_typed(narrow = 1)): register width 8 at four waves on the 512-graph 1M-edge batch 0.071 against
// 0.081 ms (spread 0.005) and on the one-graph batch 0.081 against 2.125; register width 32 at four waves on the one-graph batch 0.201 against
// 3.304 ms, 0.364 against 3.397, 0.255 against 3.326 — every measured class meets the bar, none is cut for its own figures.  chain_wave_cut
// (register width 32 on several graphs) applies as it stands, inherited from the fp32 form's measurement and NOT measured on bf16 features;
// register width 16 and the two-wave classes were not measured either.
inline bool chain_wave_typed_takes(const ChainShape& s, int64_t max_in_degree, int cap) {
  return chain_wave_takes(s, false, max_in_degree, cap) && chain_wave_typed_waves(s, cap) >= 2;
}
// its workspace: the partial rows alone (256 bytes where there are none: a query's 0 is a refusal)
inline size_t chain_wave_typed_bytes(const ChainShape& s, int64_t n_wtiles) {
  return std::max((size_t)256, sizeof(float) * chain_wave_partial_floats(s, n_wtiles));
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
// wide: the mask of chain_wide_mask (gnx_chain_block_forward_wide) — such a function has its rows in LDS: none of those buffers either; the
// node function keeps its materialised input rows n_in.
inline ChainWs chain_fw_layout(const ChainShape& s, unsigned fused, size_t ident_floats, size_t block_bytes, unsigned wide = 0) {
  ChainWs w{};
  ChainCarver c;
  const int on = s.ow[1], og = s.ow[2];
  const unsigned narrow = fused;
  fused |= wide;
  w.block = c.bytes(block_bytes);
  for (int i = 0; i < 2; ++i) w.e_buf[i] = c.floats(s.ch[0]->n_layers > 1 && !(fused & 1) ? s.rows[0] * s.maxw[0] : 0);
  w.n_in = c.floats(on > 0 && !(narrow & 2) ? s.rows[1] * (size_t)s.k0[1] : 0);
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

// ---- the wide form on bfloat16 features (gnx_chain_block_forward_wide_typed), its native rule and workspace ----
// The native rule of a bf16 call: some function is inside the wide rule, and every update function with an output and rows to run on is inside
// the wide mask or the narrow fused mask.  Then each wide function is one k_chain_wide_bf16 launch and each narrow one a k_chain_mlp_bf16 launch
// on the bf16 rows; nothing E-sized is widened or rounded by a pass of its own.  No class is cut from it for its own figures.  Measured
// (profiles/chain_wide_bf16.json, whole calls, cache-cold, medians of 15, against the parent's gnx_chain_block_forward_typed(narrow = 1) on the
// same bf16 tensors): the two-block class on the 512-graph 1M-edge batch, (10,5,3) [64,64,3]/[64,4]/[16,5] 0.372 against 0.429 ms (spreads 0.004 /
// 0.023; the fp32 wide entry on fp32 tensors 0.371), (10,5,0) [64,3]/[64,4]/[32,5] 0.244 against 0.281 (0.003 / 0.006; fp32 0.252) — both beat the
// parent by more than the larger spread; workspace 15.7 against 657 MiB.  On the one-graph 1M-edge batch 3.566 against 3.631 (0.077 / 0.079) and
// 3.448 against 3.481 (0.071 / 0.085): inside the spread, not slower.  Before k_chain_wide_bf16 was held to three waves per SIMD (168 registers)
// the same cases took 0.500 and 0.323 ms on the 512-graph batch: slower than the parent.  Not measured: the one-block class, a LayerNorm-first edge
// function (the widening path), a narrow edge function in front of a wide node function, and the graph function's rows form on its own.
inline bool chain_wide_typed_native(const ChainShape& s, unsigned fused, unsigned wide) {
  return wide != 0 && chain_typed_native(s, fused | wide);
}
// ... and its workspace: chain_fw_layout with both masks (n_in for a wide node function, g_in; no block workspace, no e_buf / n_buf / g_buf of a
// function that runs) and behind it the three carves of chain_native_counts (the unrounded ef' and nf' for the later functions of the call, the
// widened gf for the graph function's input rows).  No copy of ef, nf or of an output: a wide node function's input rows are assembled from the
// fp32 ef' and the bf16 nf / gf directly (k_chain_node_rows_bf16).
inline size_t chain_wide_typed_native_bytes(const ChainShape& s, unsigned fused, unsigned wide, size_t ident_floats) {
  ChainCarver c;
  c.o = ChainCarver::up(chain_fw_layout(s, fused, ident_floats, 0, wide).total);
  size_t counts[3];
  chain_native_counts(s, counts);
  for (int i = 0; i < 3; ++i) c.floats(counts[i]);
  return c.o;
}

// The pullback (gnx_chain_block_backward: fused = 0; _narrow: the mask of CHAIN_RULE_BW).  A fused function keeps no per-layer outputs, no delta
// buffers and (the edge function) no inner block workspaces; it adds its partial rows and (the edge function) the compact [R E][2 dn + dg] input
// gradient.  blk_fw_bytes / blk_bw_bytes: gnx_block_workspace_bytes / gnx_block_backward_workspace_bytes of s.edge_block unless the edge
// function is fused; chunk: BW_CH, the rows per partial of the generic weight-gradient reduction; dw_partial(rows, J, K): dw_mfma_partial_floats.
// wide: the mask of chain_bw_wide_mask (gnx_chain_block_backward_wide), disjoint from `fused` — such a function has its rows on the kernel's LDS tape: no
// per-layer outputs, no delta buffers and no transposed weights are sized for it; the node and the graph function keep their input rows Xn / Xg.
struct ChainBwLayout {
  ChainCarve act[3][kChainMaxLayers + 1];  // stored layer outputs per chain (a fused chain: its last layer's, where a level above reads it)
  ChainCarve Xn, dXn, Xg, dXg, gbuf[3], blk_fw, blk_bw, part, wt, off2, ident, dxe;
  size_t total;
};
template <class DwPartial>
inline ChainBwLayout chain_bw_layout(const ChainShape& s, unsigned fused, size_t ident_floats, size_t blk_fw_bytes, size_t blk_bw_bytes, size_t chunk, DwPartial dw_partial,
                                     unsigned wide = 0) {
  ChainBwLayout L{};
  ChainCarver c;
  const int oe = s.ow[0], on = s.ow[1], og = s.ow[2];
  const int Kn = s.k0[1], Kg = s.k0[2];
  size_t gmax = 1, pmax = 2048 * 4, wmax = 1;
  for (int t = 0; t < 3; ++t) {
    const gnx_chain& ch = *s.ch[t];
    if (wide & (1u << t)) {  // its last layer's output where a level above reads it (launch_chain_wide), and its partial rows: nothing else
      if (t == 0 ? on > 0 || og > 0 : t == 1 && og > 0) L.act[t][ch.n_layers - 1] = c.floats(s.rows[t] * (size_t)s.ow[t]);
      const ChainBwWideShape sh = chain_bw_wide_shape(ch, s.k0[t], s.trows[t]);
      pmax = std::max(pmax, (size_t)sh.P * sh.nwg * (size_t)s.R);
      continue;
    }
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
  const unsigned one = fused | wide;  // the functions that run in one kernel
  const bool all_fused = (oe == 0 || (one & 1)) && (on == 0 || (one & 2)) && (og == 0 || (one & 4)) && one != 0;
  for (int i = 0; i < 3; ++i) L.gbuf[i] = c.floats(all_fused ? 0 : gmax);
  L.blk_fw = c.bytes(blk_fw_bytes); L.blk_bw = c.bytes(blk_bw_bytes);
  L.part = c.floats(pmax); L.wt = c.floats(wmax); L.off2 = c.floats(16);
  L.ident = c.floats(ident_floats);
  L.dxe = c.floats((one & 1) ? s.rows[0] * (size_t)(2 * s.dn + s.dg) : 0);
  L.total = c.o + 256;
  return L;
}

// ---- the wave form of the pullback (gnx_chain_block_backward_wave; gnx_chain_bw_wave.hip): the node and the edge function's pullbacks in one
//      wave-per-tile kernel ----
// The LDS plan of k_chain_wave_bw: both functions' staged parameters (the edge function's first), then per wave a tape of 64 rows at
// ld = max(ld_e, ld_n) (each function under its own ChainBwNarrowShape), P_e + P_n accumulators and a slice [cap][oe | 1] — the tile's ef' rows,
// later the node rows' input-gradient columns [0, oe).  waves: per workgroup, as many as fit 64 KB, at most 4 — the rule takes a block from 2 on.
struct ChainBwWaveShape {
  ChainBwNarrowShape e, n;
  int ld, stride, par_e, par_all, per_wave, waves;
  size_t nwg;  // workgroups (= partial rows per layer) per replica
};
inline ChainBwWaveShape chain_bw_wave_shape(const ChainShape& s, int cap, int64_t n_wtiles) {
  ChainBwWaveShape w{};
  w.e = chain_bw_narrow_shape(*s.ch[0], s.k0[0], s.trows[0]);
  w.n = chain_bw_narrow_shape(*s.ch[1], s.k0[1], s.trows[1]);
  w.ld = std::max(w.e.ld, w.n.ld);
  w.stride = chain_wave_stride(s.ow[0]);
  w.par_e = w.e.par_floats; w.par_all = w.e.par_floats + w.n.par_floats;
  w.per_wave = 64 * w.ld + w.e.P + w.n.P + cap * w.stride;
  w.waves = std::min(4, std::max(0, (kChainBwLdsFloats - w.par_all) / w.per_wave));
  if (w.waves > 0) w.nwg = ((size_t)n_wtiles + w.waves - 1) / w.waves;
  return w;
}
// The class CUT from the pullback's wave rule: register width 8 (every input and layer width of the edge and the node function at most 8) on a
// batch of SEVERAL graphs.  Measured (profiles/chain_bw_wave.json, whole calls, cache-cold, all gradients wanted, against the parent's
// gnx_chain_block_backward_narrow): on the 512-graph 1M-edge batch its case (3,2,1) [8,8,2]/[8,3]/[8,2] took 0.443 against 0.396 ms (spread
// 0.006).  On the one-graph 1M-edge batch the same case took 0.458 against 2.424 ms and the register-width-32 case (10,5,0) [16,3]/[8,4]/[6,5]
// 2.726 against 3.992 (spread 0.088): there both classes stay.  Register width 32 on several graphs is the forward's cut (chain_wave_cut);
// register width 16 was not measured on either batch; the other two measured blocks are outside the rule by its LDS term.
inline bool chain_bw_wave_cut(const ChainShape& s) {
  return std::max({s.k0[0], s.k0[1], s.maxw[0], s.maxw[1]}) <= 8 && s.trows[2] > 1;
}
// The rule (include/gnx.h states it): the forward's wave rule (fp32, no Dropout entry, E > 0, oe > 0, on > 0, no node with more in-edges than
// the wave-tile edge cap, the forward's cut class), every function that runs inside the narrow pullback's rule, the LDS plan above at two waves.
// bf16 (gnx_chain_block_backward_wave_typed; gnx_chain_bw_wave_bf16.hip): the fp32 rule with nothing added — the tape, the accumulators and the
// slice stay fp32, so the LDS plan is chain_bw_wave_shape as it stands.  chain_wave_cut and chain_bw_wave_cut apply by inheritance from the fp32
// measurements; they were NOT measured on bf16 features.
inline bool chain_bw_wave_takes(const ChainShape& s, bool bf16, int64_t max_in_degree, int cap, int64_t n_wtiles) {
  if (!chain_wave_takes(s, false, max_in_degree, cap)) return false;
  for (int t = 0; t < 3; ++t)
    if ((t < 2 || s.ch[t]->n_layers > 0) && !chain_bw_narrow_takes(*s.ch[t], s.k0[t], s.trows[t])) return false;
  if (chain_bw_wave_shape(s, cap, n_wtiles).waves < 2 || chain_bw_wave_cut(s)) return false;
  // bf16: no class is cut for its own figures.  Measured (profiles/chain_bw_wave_bf16.json, whole calls, cache-cold, all gradients wanted, against
  // the parent's gnx_chain_block_backward_narrow_typed on the same bf16 tensors), on the one-graph 1M-edge batch: register width 8, (3,2,1)
  // [8,8,2]/[8,3]/[8,2], 0.489 against 2.431 ms (spread 0.061; the fp32 wave pullback on fp32 tensors 0.458); register width 32, (10,5,0)
  // [16,3]/[8,4]/[6,5], 2.767 against 3.972 ms (spread 0.081; fp32 2.719).  Not measured on bf16 features: register width 16 on either batch, and
  // any class on several graphs (there the two measured classes are cut by inheritance, the other measured blocks are outside the LDS term).
  (void)bf16;
  return true;
}
// Its workspace: the tiles' partial rows and the graph level's rows (a block with a graph function), the node rows' input-gradient columns
// [oe, Kn) as [R N][dn + dg], the edge rows' node / graph columns [R E][2 dn + dg], the partial rows of the parameter gradients (shared with
// the column-sum slices, as in chain_bw_layout).  No ef', no nf', no columns [0, oe) of dXn.
struct ChainBwWaveLayout { ChainCarve partials, Xg, dXg, dXn, dxe, part; size_t total; };
inline ChainBwWaveLayout chain_bw_wave_layout(const ChainShape& s, int cap, int64_t n_wtiles) {
  ChainBwWaveLayout L{};
  ChainCarver c;
  const int oe = s.ow[0], og = s.ow[2], Kg = s.k0[2];
  const ChainBwWaveShape w = chain_bw_wave_shape(s, cap, n_wtiles);
  size_t pmax = std::max((size_t)2048 * 4, (size_t)(w.e.P + w.n.P) * w.nwg * (size_t)s.R);
  if (og > 0) {
    const ChainBwNarrowShape g = chain_bw_narrow_shape(*s.ch[2], Kg, s.trows[2]);
    pmax = std::max(pmax, (size_t)g.P * g.nwg * (size_t)s.R);
  }
  pmax = std::max(pmax, std::max(s.rows[2] * 256, (size_t)2048) * (size_t)std::max({s.dg, oe, 1}));  // column-sum slices
  L.partials = c.floats(chain_wave_partial_floats(s, n_wtiles));
  L.Xg = c.floats(og > 0 ? s.rows[2] * Kg : 0); L.dXg = c.floats(og > 0 ? s.rows[2] * Kg : 0);
  L.dXn = c.floats(s.rows[1] * (size_t)(s.dn + s.dg));
  L.dxe = c.floats(s.rows[0] * (size_t)(2 * s.dn + s.dg));
  L.part = c.floats(pmax);
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
// The wave pullback on bf16 features: chain_bw_wave_layout and behind it the same two graph-sized carves (R G dg floats each: the widened gf,
// which k_chain_graph_rows_wave assembles Xg from, and the fp32 d_gf accumulator).  Nothing E- or N-sized is added.
struct ChainBwWaveTypedLayout { ChainBwWaveLayout W; ChainBwNativeWs nw; size_t total; };
inline ChainBwWaveTypedLayout chain_bw_wave_typed_layout(const ChainShape& s, int cap, int64_t n_wtiles) {
  ChainBwWaveTypedLayout L{};
  L.W = chain_bw_wave_layout(s, cap, n_wtiles);
  L.nw = chain_bw_native_layout(s, L.W.total);
  L.total = L.nw.total;
  return L;
}

}  // namespace gnx
