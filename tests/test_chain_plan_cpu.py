"""The host arithmetic of a Chain block call (graphnets.jl_amd/csrc/gnx_chain_plan.h), compiled on its own with g++ against include/gnx.h: the two
fused rules and their masks on the widths of tests/chain_bw_cases.py's CASES (written out as a plain table, with the masks this file's Python
restatements of include/gnx.h give), the rules' limits, and the two workspace layouts."""
import os
import subprocess

from tests import chain_bw_cases as CC
from tests.test_chain_bw_narrow_abi import ceil4, formula_takes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def forward_takes(k_in, widths, ln=(), rows=1):
    """include/gnx.h, gnx_chain_block_forward_narrow: >= 1 layer, output, widths <= 32, zero-padded parameters within 10240 floats of LDS"""
    if not 1 <= len(widths) <= 16 or rows == 0 or widths[-1] <= 0 or k_in > 32 or any(w > 32 for w in widths):
        return False
    par, k = 0, k_in
    for i, w in enumerate(widths):
        par += 2 * ceil4(w) if i in ln else ceil4(k) * ceil4(w) + ceil4(w)
        k = w
    return par <= 10240


# chains found by search: (k_in, widths, LayerNorm layers); par = the forward's floats, two = par + 2 (64 ld + P), the pullback's with two waves
ON_FW_BUDGET = (20, [20, 24, 20, 27, 31, 31, 22, 29, 23, 28, 23, 28, 21, 28, 26, 31], (0, 5))     # par = 10240
OVER_FW_BUDGET = (32, [25, 27, 30, 30, 26, 24, 23, 23, 22, 24, 26, 27, 22, 22, 32], (7, 13))      # par = 10244 (par is a multiple of 4)
ON_BW_BUDGET = (31, [31, 1], (0,))                                                                 # two = 16384
OVER_BW_BUDGET = (4, [14, 17, 23, 32], ())                                                         # two = 16386 (two is even)
LIMITS = (ON_FW_BUDGET, OVER_FW_BUDGET, ON_BW_BUDGET, OVER_BW_BUDGET, (32, [32], ()), (32, [33, 3], ()), (33, [8], ()), (32, [32, 33], ()))


def _fn(k_in, layers):
    """C initialiser of one function: {k_in, n, {widths}, {0 Dense / 1 LayerNorm / 2 sqrt-eps LayerNorm}}"""
    ws = [l[0] for l in layers]
    kinds = [{"dense": 0, "ln": 1, "ln_sqrt": 2}[l[2]] for l in layers]
    return "{%d, %d, {%s}, {%s}}" % (k_in, len(ws), ", ".join(map(str, ws)) or "0", ", ".join(map(str, kinds)) or "0")


def case_table():
    rows = []
    for cid in CC.CASE_IDS:
        c = CC.CASE[cid]
        fw = bw = 0
        for t, ((k_in, layers), T) in enumerate(zip(CC.shape(cid), CC.rows(cid))):
            ln = tuple(i for i, l in enumerate(layers) if l[2] != "dense")
            ws = [l[0] for l in layers]
            fw |= (1 << t) if layers and forward_takes(k_in, ws, ln, T) else 0
            bw |= (1 << t) if layers and formula_takes(k_in, ws, ln, T) else 0
        assert bw == CC.formula_mask(cid) and (c["family"] != "narrow" or bw == CC.want_mask(cid)), cid
        E, N, G = CC.rows(cid)
        rows.append('  {"%s", {%d, %d, %d}, {%d, %d, %d}, %d, {%s}, %du, %du},' % (
            cid, *c["in_dims"], E, N, G, c["R"], ", ".join(_fn(k_in, layers) for k_in, layers in CC.shape(cid)), fw, bw))
    return "\n".join(rows)


def limit_table():
    rows = []
    for k_in, ws, ln in LIMITS:
        layers = [(w, None, "ln" if i in ln else "dense") for i, w in enumerate(ws)]
        rows.append("  {%s, %d, %d}," % (_fn(k_in, layers), forward_takes(k_in, ws, ln), formula_takes(k_in, ws, ln)))
    return "\n".join(rows)


DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "gnx_chain_plan.h"
using namespace gnx;
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL line %d: %s [%s]\n", __LINE__, #c, ctx); ++fails; } } while (0)
static const char* ctx = "";
struct Fn { int k_in, n, w[16], kind[16]; };
struct Case { const char* id; int d[3]; long long cnt[3]; int R; Fn f[3]; unsigned fw, bw; };
struct Limit { Fn f; int fw, bw; };
static const Case cases[] = {
@CASES@
};
static const Limit limits[] = {
@LIMITS@
};
static const float one = 1.f;
struct Built { gnx_dense layers[3][16]; int32_t widths[3][16]; gnx_chain_block_params p; };
static gnx_chain chain_of(const Fn& f, gnx_dense* layers, int32_t* widths) {
  for (int i = 0; i < f.n; ++i) {
    widths[i] = f.w[i];
    layers[i] = gnx_dense{&one, &one, GNX_ACT_IDENTITY, f.kind[i] == 0 ? GNX_LAYER_DENSE : f.kind[i] == 1 ? GNX_LAYER_LAYERNORM : (GNX_LAYER_LAYERNORM | GNX_LAYER_LN_SQRT_EPS)};
  }
  gnx_chain c{};
  c.layers = layers; c.widths = widths; c.n_layers = f.n;
  return c;
}
static void build(const int d[3], const Fn f[3], Built& b) {
  std::memset(&b.p, 0, sizeof b.p);
  b.p.de = d[0]; b.p.dn = d[1]; b.p.dg = d[2];
  b.p.edgefn = chain_of(f[0], b.layers[0], b.widths[0]);
  b.p.nodefn = chain_of(f[1], b.layers[1], b.widths[1]);
  b.p.graphfn = chain_of(f[2], b.layers[2], b.widths[2]);
}
static void check_carves(const std::vector<ChainCarve>& v, size_t total) {
  for (size_t i = 0; i < v.size(); ++i) {
    EXPECT(v[i].off % 256 == 0 && v[i].off + v[i].bytes <= total);
    for (size_t j = 0; j < i; ++j)
      if (v[i].bytes && v[j].bytes) EXPECT(v[i].off + v[i].bytes <= v[j].off || v[j].off + v[j].bytes <= v[i].off);
  }
}
static size_t up(size_t x) { return (x + 255) / 256 * 256; }
// both layouts of one shape under one mask; the inner block's workspaces and the matrix-core partials are inputs: any sizes will do
static void check_layouts(const ChainShape& s, unsigned m, size_t ident) {
  const size_t blk = s.ow[0] > 0 && !(m & 1) ? 12345 : 0;
  const ChainWs w = chain_fw_layout(s, m, ident, blk);
  check_carves({w.block, w.e_buf[0], w.e_buf[1], w.n_in, w.n_buf[0], w.n_buf[1], w.g_in, w.g_buf[0], w.g_buf[1], w.ident}, w.total);
  if (m & 1) EXPECT(!w.block.bytes && !w.e_buf[0].bytes && !w.e_buf[1].bytes);
  if (m & 2) EXPECT(!w.n_in.bytes && !w.n_buf[0].bytes && !w.n_buf[1].bytes);
  if (m & 4) EXPECT(!w.g_buf[0].bytes && !w.g_buf[1].bytes);
  EXPECT(w.ident.bytes == 4 * ident && w.block.bytes == blk);
  // what a carve must hold: rows x width floats
  EXPECT(w.g_in.bytes == (s.ow[2] > 0 ? 4 * s.rows[2] * (size_t)s.k0[2] : 0));
  if (!(m & 2)) EXPECT(w.n_in.bytes == (s.ow[1] > 0 ? 4 * s.rows[1] * (size_t)s.k0[1] : 0));
  for (int t = 0; t < 3; ++t) {
    const ChainCarve* buf = t == 0 ? w.e_buf : t == 1 ? w.n_buf : w.g_buf;
    const size_t want = !((m >> t) & 1) && s.ch[t]->n_layers > 1 ? 4 * s.rows[t] * (size_t)s.maxw[t] : 0;
    EXPECT(buf[0].bytes == want && buf[1].bytes == want);
  }
  // bf16: the native path's three fp32 carves, or the six staged copies, stand behind the fp32 layout
  size_t counts[3], native = up(w.total), staged = up(w.total);
  chain_native_counts(s, counts);
  for (int i = 0; i < 3; ++i) native += up(4 * counts[i]);
  const int d6[6] = {s.de, s.dn, s.dg, s.ow[0], s.ow[1], s.ow[2]};
  for (int i = 0; i < 6; ++i) staged += up(4 * s.rows[i % 3] * (size_t)d6[i]);
  EXPECT(native >= w.total && staged >= native);
  bool all_in = true;  // the native plan exists exactly when every function with an output and rows is in the mask
  for (int t = 0; t < 3; ++t) all_in = all_in && !(s.ow[t] > 0 && s.trows[t] > 0 && !((m >> t) & 1));
  EXPECT(chain_typed_native(s, m) == all_in);

  const size_t bf = (m & 1) || s.ch[0]->n_layers == 0 ? 0 : 777, bb = (m & 1) || s.ch[0]->n_layers == 0 ? 0 : 4099;
  const ChainBwLayout L = chain_bw_layout(s, m, ident, bf, bb, 2048, [](size_t rows, int J, int K) { return rows / 128 * (size_t)J * K; });
  std::vector<ChainCarve> v = {L.Xn, L.dXn, L.Xg, L.dXg, L.gbuf[0], L.gbuf[1], L.gbuf[2], L.blk_fw, L.blk_bw, L.part, L.wt, L.off2, L.ident, L.dxe};
  for (int t = 0; t < 3; ++t)
    for (int i = 0; i <= kChainMaxLayers; ++i) v.push_back(L.act[t][i]);
  check_carves(v, L.total);
  for (int t = 0; t < 3; ++t) {
    const bool keeps_all = !((m >> t) & 1) || (t == 1 && chain_bw_node_fw_generic(m, s.ow[2]));
    const bool crosses = t == 0 ? s.ow[1] > 0 || s.ow[2] > 0 : t == 1 && s.ow[2] > 0;
    for (int i = 0; i < s.ch[t]->n_layers; ++i)
      EXPECT(L.act[t][i].bytes == (keeps_all || (crosses && i + 1 == s.ch[t]->n_layers) ? 4 * s.rows[t] * (size_t)s.ch[t]->widths[i] : 0));
  }
  const size_t xn = s.ow[1] > 0 ? 4 * s.rows[1] * (size_t)s.k0[1] : 0, xg = s.ow[2] > 0 ? 4 * s.rows[2] * (size_t)s.k0[2] : 0;
  EXPECT(L.dXn.bytes == xn && L.Xg.bytes == xg && L.dXg.bytes == xg);
  EXPECT(L.Xn.bytes == (!(m & 2) || chain_bw_node_fw_generic(m, s.ow[2]) ? xn : 0));
  if (m & 1) EXPECT(!L.blk_fw.bytes && !L.blk_bw.bytes && L.dxe.bytes == 4 * s.rows[0] * (size_t)(2 * s.dn + s.dg));
  else EXPECT(!L.dxe.bytes && L.blk_fw.bytes == bf && L.blk_bw.bytes == bb);
  bool all_fused = m != 0;
  for (int t = 0; t < 3; ++t) all_fused = all_fused && (s.ow[t] == 0 || ((m >> t) & 1));
  EXPECT((L.gbuf[0].bytes == 0) == all_fused && L.part.bytes >= 4 * 2048 * 4 && L.ident.bytes == 4 * ident);
}
int main() {
  Built b;
  // ---- the masks of both rules on the cases ----
  for (const Case& c : cases) {
    ctx = c.id;
    build(c.d, c.f, b);
    const ChainShape s = chain_shape(c.cnt[0], c.cnt[1], c.cnt[2], b.p, c.R);
    for (int t = 0; t < 3; ++t) EXPECT(s.k0[t] == c.f[t].k_in && s.ow[t] == (c.f[t].n ? c.f[t].w[c.f[t].n - 1] : 0));
    EXPECT(chain_fused_mask(s, CHAIN_RULE_FW) == c.fw);
    EXPECT(chain_fused_mask(s, CHAIN_RULE_BW) == c.bw);
    EXPECT((chain_fused_mask(s, CHAIN_RULE_BW) & ~chain_fused_mask(s, CHAIN_RULE_FW)) == 0);  // the pullback's rule is the forward's and more
    EXPECT(s.wide == (c.id[0] == 'W'));
  }
  // ---- the limits: width 33, one step over either LDS budget refused; exactly on the budget taken ----
  ctx = "limits";
  for (const Limit& l : limits) {
    gnx_dense layers[16]; int32_t widths[16];
    const gnx_chain c = chain_of(l.f, layers, widths);
    EXPECT(chain_narrow_takes(c, l.f.k_in, 1031) == (bool)l.fw);
    EXPECT(chain_bw_narrow_takes(c, l.f.k_in, 1031) == (bool)l.bw);
    EXPECT(!chain_narrow_takes(c, l.f.k_in, 0) && !chain_bw_narrow_takes(c, l.f.k_in, 0));  // no rows to run on
  }
  {
    gnx_dense layers[16]; int32_t widths[16];
    const gnx_chain on_fw = chain_of(limits[0].f, layers, widths);
    EXPECT(chain_narrow_lds_floats(on_fw, limits[0].f.k_in) == kChainNarrowLdsFloats && limits[0].fw == 1 && limits[1].fw == 0);
    const gnx_chain over_fw = chain_of(limits[1].f, layers, widths);
    EXPECT(chain_narrow_lds_floats(over_fw, limits[1].f.k_in) == kChainNarrowLdsFloats + 4);
    const gnx_chain on_bw = chain_of(limits[2].f, layers, widths);
    ChainBwNarrowShape sh = chain_bw_narrow_shape(on_bw, limits[2].f.k_in, 1031);
    EXPECT(sh.par_floats + 2 * (64 * sh.ld + sh.P) == kChainBwLdsFloats && sh.waves == 2 && sh.nwg == (1031 + 127) / 128 && limits[2].bw == 1);
    const gnx_chain over_bw = chain_of(limits[3].f, layers, widths);
    sh = chain_bw_narrow_shape(over_bw, limits[3].f.k_in, 1031);
    // the one-wave class: the forward takes it, the pullback does not
    EXPECT(sh.par_floats + 2 * (64 * sh.ld + sh.P) == kChainBwLdsFloats + 2 && sh.waves == 1 && limits[3].fw == 1 && limits[3].bw == 0);
    EXPECT(limits[4].fw == 1 && limits[5].fw == 0 && limits[6].fw == 0 && limits[7].fw == 0);
  }
  // ---- the layouts: every mask that fuses only functions with an output (the rule gives no other), each output in turn of width 0 ----
  static const Fn base[3] = {{23, 2, {16, 3}, {0, 0}}, {11, 2, {8, 4}, {0, 0}}, {10, 2, {6, 5}, {0, 0}}};
  static const Fn ln_first[3] = {{23, 3, {23, 16, 3}, {2, 0, 0}}, {11, 2, {8, 4}, {0, 0}}, {10, 2, {6, 5}, {0, 0}}};
  const int d[3] = {10, 5, 3};
  const long long counts[3][3] = {{4099, 1031, 1}, {4099, 1031, 131}, {0, 1031, 131}};  // the last: a batch without edges
  for (const auto& cnt : counts)
    for (int R = 1; R <= 2; ++R)
      for (int zero = -1; zero < 3; ++zero)
        for (int lnf = 0; lnf < 2; ++lnf) {
          Fn f[3];
          for (int t = 0; t < 3; ++t) { f[t] = (lnf ? ln_first : base)[t]; if (t == zero) f[t].n = 0; }
          if (zero == 0) { f[1].k_in -= 3; f[2].k_in -= 3; }
          if (zero == 1) f[2].k_in -= 4;
          build(d, f, b);
          const ChainShape s = chain_shape(cnt[0], cnt[1], cnt[2], b.p, R);
          for (int t = 0; t < 3; ++t) EXPECT(s.k0[t] == f[t].k_in);
          unsigned live = 0;
          for (int t = 0; t < 3; ++t) live |= s.ow[t] > 0 ? 1u << t : 0;
          char name[96];
          for (unsigned m = 0; m < 8; ++m) {
            if (m & ~live) continue;
            std::snprintf(name, sizeof name, "layout E=%lld G=%lld R=%d zero=%d ln_first=%d mask=%u", cnt[0], cnt[2], R, zero, lnf, m);
            ctx = name;
            // the identity layer of a LayerNorm-first edge function exists for the generic form alone
            check_layouts(s, m, lnf && !(m & 1) && zero != 0 ? 23 * 23 : 0);
          }
          // ---- a batch without edges: nothing divides by the edge count; no edge function is fused without rows ----
          if (cnt[0] == 0) EXPECT(!(chain_fused_mask(s, CHAIN_RULE_FW) & 1) && !(chain_fused_mask(s, CHAIN_RULE_BW) & 1) && chain_bw_narrow_shape(*s.ch[1], s.k0[1], 0).nwg == 0);
        }
  if (fails) return 1;
  std::printf("chain plan ok\n");
  return 0;
}
"""


def test_chain_plan_header(tmp_path):
    src = tmp_path / "chain_plan.cpp"
    src.write_text(DRIVER.replace("@CASES@", case_table()).replace("@LIMITS@", limit_table()))
    exe = tmp_path / "chain_plan"
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "graphnets.jl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr
    assert "chain plan ok" in out.stdout
