"""The host arithmetic of the native bf16 Chain pullback (graphnets.jl_amd/csrc/gnx_chain_plan.h: chain_bw_typed_native, chain_bw_native_layout),
compiled on its own with g++ against include/gnx.h: the native rule on hand-written shapes — the README block, a batch without edges, an edge
function the one-wave class cuts, mixed masks, absent outputs — and the native workspace, which is the fp32 narrow layout plus the two
graph-sized carves, to the byte."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "gnx_chain_plan.h"
using namespace gnx;
static int fails = 0;
static const char* ctx = "";
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL line %d: %s [%s]\n", __LINE__, #c, ctx); ++fails; } } while (0)
struct Fn { int n, w[16], kind[16]; };  // kind: 0 Dense, 1 LayerNorm
struct Case { const char* id; int d[3]; long long cnt[3]; int R; Fn f[3]; unsigned mask; int native; };
static const Case cases[] = {
  // the README block on the 1M-edge batch: [16,ln,16,3] [8,4] [6,5] behind (10,5,3)
  {"readme", {10, 5, 3}, {1000000, 100000, 512}, 1, {{4, {16, 16, 16, 3}, {0, 1, 0, 0}}, {2, {8, 4}, {0, 0}}, {2, {6, 5}, {0, 0}}}, 7u, 1},
  {"one-graph-replicas", {10, 5, 3}, {4099, 1031, 1}, 3, {{2, {16, 3}, {0, 0}}, {2, {8, 4}, {0, 0}}, {2, {6, 5}, {0, 0}}}, 7u, 1},
  // E = 0: the node and graph functions are inside the rule, but there is no edge level to pull back through
  {"no-edges", {10, 5, 3}, {0, 1031, 131}, 1, {{2, {16, 3}, {0, 0}}, {2, {8, 4}, {0, 0}}, {2, {6, 5}, {0, 0}}}, 6u, 0},
  // the one-wave class: [14,17,23,32] at k_in 4 needs 16386 floats with two waves (tests/test_chain_plan_cpu.py: OVER_BW_BUDGET): the forward fuses
  // it, the pullback does not -> mixed (mask 2: the graph function's input, 32 + 4 wide, is outside the rule as well)
  {"edge-cut-by-the-one-wave-class", {4, 0, 0}, {4099, 1031, 7}, 1, {{4, {14, 17, 23, 32}, {0, 0, 0, 0}}, {1, {4}, {0}}, {1, {3}, {0}}}, 2u, 0},
  // ... and alone, the only function of its block: still not native
  {"edge-cut-alone", {4, 0, 0}, {4099, 1031, 7}, 1, {{4, {14, 17, 23, 32}, {0, 0, 0, 0}}, {0, {0}, {0}}, {0, {0}, {0}}}, 0u, 0},
  // mixed masks: a 33-wide layer in the node function (mask 5), in the graph function (mask 3)
  {"mixed-node-wide", {10, 5, 3}, {4099, 1031, 7}, 1, {{2, {16, 3}, {0, 0}}, {2, {33, 4}, {0, 0}}, {2, {6, 5}, {0, 0}}}, 5u, 0},
  {"mixed-graph-wide", {10, 5, 3}, {4099, 1031, 7}, 1, {{2, {16, 3}, {0, 0}}, {2, {8, 4}, {0, 0}}, {2, {33, 5}, {0, 0}}}, 3u, 0},
  // absent outputs do not stand in the way: the edge function alone; no graph output
  {"edge-only", {6, 0, 0}, {4099, 1031, 7}, 1, {{2, {4, 3}, {0, 0}}, {0, {0}, {0}}, {0, {0}, {0}}}, 1u, 1},
  {"no-graph-output", {0, 4, 2}, {4099, 1031, 7}, 1, {{2, {8, 5}, {0, 0}}, {1, {5}, {0}}, {0, {0}, {0}}}, 3u, 1},
  // an edge function without output: no pullback at all
  {"no-edge-output", {10, 5, 3}, {4099, 1031, 7}, 1, {{0, {0}, {0}}, {2, {8, 4}, {0, 0}}, {2, {6, 5}, {0, 0}}}, 6u, 0},
};
static const float one = 1.f;
struct Built { gnx_dense layers[3][16]; int32_t widths[3][16]; gnx_chain_block_params p; };
static gnx_chain chain_of(const Fn& f, gnx_dense* layers, int32_t* widths) {
  for (int i = 0; i < f.n; ++i) {
    widths[i] = f.w[i];
    layers[i] = gnx_dense{&one, &one, GNX_ACT_IDENTITY, f.kind[i] == 0 ? GNX_LAYER_DENSE : GNX_LAYER_LAYERNORM};
  }
  gnx_chain c{};
  c.layers = layers; c.widths = widths; c.n_layers = f.n;
  return c;
}
static size_t up(size_t x) { return (x + 255) / 256 * 256; }
int main() {
  Built b;
  for (const Case& c : cases) {
    ctx = c.id;
    std::memset(&b.p, 0, sizeof b.p);
    b.p.de = c.d[0]; b.p.dn = c.d[1]; b.p.dg = c.d[2];
    b.p.edgefn = chain_of(c.f[0], b.layers[0], b.widths[0]);
    b.p.nodefn = chain_of(c.f[1], b.layers[1], b.widths[1]);
    b.p.graphfn = chain_of(c.f[2], b.layers[2], b.widths[2]);
    const ChainShape s = chain_shape(c.cnt[0], c.cnt[1], c.cnt[2], b.p, c.R);
    const unsigned m = chain_fused_mask(s, CHAIN_RULE_BW);
    EXPECT(m == c.mask);
    EXPECT(chain_bw_typed_native(s, m, true) == (bool)c.native);
    EXPECT(!chain_bw_typed_native(s, m, false));  // fp32 features: never
    // the rule restated: an edge output, edges, and every function with an output and rows in the mask
    bool want = s.ow[0] > 0 && c.cnt[0] > 0;
    for (int t = 0; t < 3; ++t) want = want && !(s.ow[t] > 0 && c.cnt[t] > 0 && !((m >> t) & 1));
    EXPECT(want == (bool)c.native);
    if (!c.native) continue;
    EXPECT(!chain_bw_node_fw_generic(m, s.ow[2]));  // all functions are fused: nf' is never recomputed by the generic launches
    // the native layout: the fp32 narrow layout, then the widened gf (a graph function alone reads it), then the fp32 d_gf
    const ChainBwLayout L = chain_bw_layout(s, m, 0, 0, 0, 2048, [](size_t rows, int J, int K) { return rows / 128 * (size_t)J * K; });
    const ChainBwNativeWs w = chain_bw_native_layout(s, L.total);
    const size_t g = 4 * (size_t)c.R * (size_t)c.cnt[2] * (size_t)c.d[2];
    EXPECT(L.total % 256 == 0);
    EXPECT(w.gf32.off == L.total && w.gf32.bytes == (s.ow[2] > 0 ? g : 0));
    EXPECT(w.dgf32.off == L.total + up(w.gf32.bytes) && w.dgf32.bytes == g);
    EXPECT(w.total == L.total + up(w.gf32.bytes) + up(g));
    // ... within the narrow workspace plus three carves of R G max(dg, og) floats, and no E- or N-sized carve among them
    EXPECT(w.total <= L.total + 3 * up(4 * (size_t)c.R * (size_t)c.cnt[2] * (size_t)(c.d[2] > s.ow[2] ? c.d[2] : s.ow[2])));
    // ... and below the staged call's nine copies behind the same layout
    const int d9[9] = {s.de, s.dn, s.dg, s.ow[0], s.ow[1], s.ow[2], s.de, s.dn, s.dg};
    size_t staged = L.total;
    for (int i = 0; i < 9; ++i) staged += up(4 * s.rows[i % 3] * (size_t)d9[i]);
    EXPECT(w.total < staged);
  }
  if (fails) return 1;
  std::printf("chain native pullback plan ok\n");
  return 0;
}
"""


def test_native_rule_and_layout(tmp_path):
    src = tmp_path / "chain_bw_native_plan.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "chain_bw_native_plan"
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "graphnets.jl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr
    assert "chain native pullback plan ok" in out.stdout
