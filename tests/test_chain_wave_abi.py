"""CPU-side checks of gnx_chain_block_forward_wave and its two queries: declared, exported and bound with the narrow trio's parameter lists, a NULL
handle refused; the rule chain_wave_takes (csrc/gnx_chain_plan.h) compiled alone as plain C++ on the LDS boundaries, the in-degree cap and the
class cut after measurement (register width 32 on several graphs)."""
import os
import re
import subprocess

import graphnets_jl_amd as gn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_chain_block_forward_wave_applies", "gnx_chain_block_forward_wave_workspace_bytes", "gnx_chain_block_forward_wave")


def test_entries_declared_exported_bound_and_refuse_null():
    import __graft_entry__ as ge
    ge.build()
    lib, S = gn._lib.load(), gn._lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "gnx.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        m = re.search(r"GNX_API [\w\s\*]+?\b" + name + r"\(([^;]*?)\);", text, flags=re.S)
        assert m and hasattr(lib, name) and name in S, name
        assert m.group(1).count(",") + 1 == len(S[name][1]), name
        assert S[name] == S[name.replace("_wave", "_narrow")], name
    assert lib.gnx_version() == 130
    assert lib.gnx_chain_block_forward_wave_applies(None, None, 1) == 0 and lib.gnx_chain_block_forward_wave_workspace_bytes(None, None, 1) == 0
    assert lib.gnx_chain_block_forward_wave(None, None, None, None, None, 1, None, None, None, None, 0, 0, None) == gn._lib.ERR_INVALID_ARG


# par = the zero-padded parameter floats of the edge and the node function; cap = 128, oe = 32: a slice of 128 * 33 = 4224 floats per wave
DRIVER = r"""
#include <cstdio>
#include "gnx_chain_plan.h"
using namespace gnx;
static const float one = 1.f;
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
struct Fn { int n, w[16], ln[16]; };
static gnx_dense layers[3][16];
static int32_t widths[3][16];
static ChainShape shape(int de, const Fn& e, const Fn& nd, const Fn& g, long long E = 4099, long long G = 1) {
  static gnx_chain_block_params p;
  p = gnx_chain_block_params{};
  p.de = de;
  const Fn* f[3] = {&e, &nd, &g};
  gnx_chain* c[3] = {&p.edgefn, &p.nodefn, &p.graphfn};
  for (int t = 0; t < 3; ++t) {
    for (int i = 0; i < f[t]->n; ++i) { widths[t][i] = f[t]->w[i]; layers[t][i] = gnx_dense{&one, &one, GNX_ACT_IDENTITY, f[t]->ln[i] ? GNX_LAYER_LAYERNORM : GNX_LAYER_DENSE}; }
    c[t]->layers = layers[t]; c[t]->widths = widths[t]; c[t]->n_layers = f[t]->n;
  }
  return chain_shape(E, 1031, G, p, 1);
}
int main() {
  const Fn none{}, n32{1, {32}, {0}}, n8{1, {8}, {0}};
  // edge: 6 -> 32 (288 floats), six 32 -> 32 Dense (1056 each), k LayerNorms (64 each); node: 32 -> 32 (1056): par = 7680 + 64 k
  Fn e{7, {32, 32, 32, 32, 32, 32, 32}, {0}};
  for (int k = 0; k < 6; ++k) { e.w[e.n] = 32; e.ln[e.n] = 1; ++e.n; const ChainShape s = shape(6, e, n32, none);
    const size_t par = chain_narrow_lds_floats(*s.ch[0], s.k0[0]) + chain_narrow_lds_floats(*s.ch[1], s.k0[1]);
    EXPECT(par == 7680 + 64 * (size_t)(k + 1));
    EXPECT(chain_wave_waves(s, 128) == (par + 2 * 4224 <= 16384 ? 2 : 0));          // k = 3: par = 7936 = 16384 - 2 * 4224, the last one inside
    EXPECT(chain_wave_takes(s, false, 128, 128) == (k <= 3)); }
  // the rule's other terms, on a block of register width 16; the cut: register width 32 (here K_e = 17) on more than one graph
  { const Fn small{2, {16, 8}, {0, 0}};
    const ChainShape s = shape(6, small, n8, none);
    EXPECT(chain_wave_waves(s, 128) == 4 && chain_wave_stride(8) == 9 && chain_wave_stride(3) == 3 && chain_wave_takes(s, false, 128, 128));
    EXPECT(chain_wave_waves(s, 256) == 4 && chain_wave_takes(s, false, 256, 256) && !chain_wave_takes(s, false, 129, 128));   // in-degree: cap | cap + 1
    EXPECT(!chain_wave_takes(s, true, 128, 128));                                       // bf16 features
    EXPECT(!chain_wave_takes(shape(6, small, n8, none, 0), false, 0, 128));             // no edges
    EXPECT(!chain_wave_takes(shape(6, small, none, none), false, 128, 128));            // no node function
    const Fn wide{1, {33}, {0}};
    EXPECT(!chain_wave_takes(shape(6, small, n8, wide), false, 128, 128));              // a graph function outside the narrow rule
    EXPECT(chain_wave_takes(shape(6, small, n8, none, 4099, 3), false, 128, 128) && !chain_wave_cut(shape(16, small, n8, none, 4099, 3)));
    EXPECT(chain_wave_takes(shape(17, small, n8, none), false, 128, 128) && !chain_wave_takes(shape(17, small, n8, none, 4099, 3), false, 128, 128));
    EXPECT(chain_wave_partial_floats(s, 77) == 0 && chain_wave_partial_floats(shape(6, small, n8, n8), 77) == 77 * 16); }
  // four waves | two: oe = 8 (slice 128 * 9 = 1152): par to either side of 16384 - 4 * 1152 = 11776
  { const Fn big{10, {32, 32, 32, 32, 32, 32, 32, 32, 32, 8}, {0}};             // 288 + 8 * 1056 + 264 = 9000 floats
    const Fn nd1{5, {32, 32, 32, 32, 8}, {0, 1, 0, 0, 0}};                         // 288 + 64 + 2 * 1056 + 264 = 2728: par = 11728 <= 11776
    const Fn nd2{6, {32, 32, 32, 32, 32, 8}, {0, 1, 1, 0, 0, 0}};                  // one LayerNorm more: par = 11792
    EXPECT(chain_wave_waves(shape(6, big, nd1, none), 128) == 4 && chain_wave_waves(shape(6, big, nd2, none), 128) == 2);
    EXPECT(chain_wave_takes(shape(6, big, nd2, none), false, 128, 128)); }
  if (fails) return 1;
  std::printf("chain wave rule ok\n");
  return 0;
}
"""


def test_the_rule_compiled_alone(tmp_path):
    src = tmp_path / "chain_wave_rule.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "chain_wave_rule"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "graphnets.jl_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "chain wave rule ok" in out.stdout, out.stdout[-4000:] + out.stderr
