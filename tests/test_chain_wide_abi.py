"""CPU-side checks of gnx_chain_block_forward_wide and its two queries: declared, exported and bound with the narrow trio's parameter lists, NULL
arguments refused as the narrow entry refuses them; the rule chain_wide_takes and its LDS plan (csrc/gnx_chain_plan.h) compiled alone as plain C++."""
import os
import re
import subprocess

import graphnets_jl_amd as gn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_chain_block_forward_wide_applies", "gnx_chain_block_forward_wide_workspace_bytes", "gnx_chain_block_forward_wide")


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
        assert S[name] == S[name.replace("_wide", "_narrow")], name
    assert lib.gnx_version() == 130
    null = (None, None, None, None, None, 1, None, None, None, None, 0, 0, None)
    assert lib.gnx_chain_block_forward_wide_applies(None, None, 1) == lib.gnx_chain_block_forward_narrow_applies(None, None, 1) == 0
    assert lib.gnx_chain_block_forward_wide_workspace_bytes(None, None, 1) == lib.gnx_chain_block_forward_narrow_workspace_bytes(None, None, 1) == 0
    assert lib.gnx_chain_block_forward_wide(*null) == lib.gnx_chain_block_forward_narrow(*null) == gn._lib.ERR_INVALID_ARG


# the plan in floats: 24 np of weight chunk + np of bias + waves * 32 * ld of slices; np = the widest Dense up to 32, ld = (widest width up to 16) | 1
DRIVER = r"""
#include <cstdio>
#include "gnx_chain_plan.h"
using namespace gnx;
static const float one = 1.f;
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
struct Fn { int n, w[16], kind[16]; };  // kind: 0 Dense, 1 LayerNorm, 2 Dropout
static gnx_dense layers[16];
static int32_t widths[16];
static gnx_chain chain(const Fn& f) {
  const int32_t kinds[3] = {GNX_LAYER_DENSE, GNX_LAYER_LAYERNORM, GNX_LAYER_DROPOUT};
  for (int i = 0; i < f.n; ++i) { widths[i] = f.w[i]; layers[i] = gnx_dense{&one, &one, GNX_ACT_IDENTITY, kinds[f.kind[i]]}; }
  return gnx_chain{layers, widths, f.n, 0};
}
static bool takes(const Fn& f, int k_in, size_t rows = 1000) { const gnx_chain c = chain(f); return chain_wide_takes(c, k_in, rows); }
static ChainWideShape plan(const Fn& f, int k_in, size_t rows = 1000) { const gnx_chain c = chain(f); return chain_wide_shape(c, k_in, rows); }
int main() {
  // inside the rule: [64, 64, 3] behind 20 inputs — ld 65, two blocks, 1536 + 64 floats in front of four slices of 2080: a tile of 128 rows
  { const Fn f{3, {64, 64, 3}, {0}};
    const ChainWideShape s = plan(f, 20);
    EXPECT(takes(f, 20) && s.ld == 65 && s.nb == 2 && s.np == 64 && s.chunk_floats == 1536 && s.slice_off == 1600 && s.waves == 4);
    EXPECT(s.floats == 1600 + 4 * 32 * 65 && s.nwg == 8 && plan(f, 20, 1025).nwg == 9);
    EXPECT(!takes(f, 20, 0) && !takes(f, 0) && !takes(f, 129)); }
  // the widest plan: k_in 128, [128, 128, 128] — ld 129, three waves, within 64 KB; the class is cut after measurement (a Dense beyond 64)
  { const Fn f{3, {128, 128, 128}, {0}}, g{2, {64, 64}, {0}};
    const ChainWideShape s = plan(f, 128);
    EXPECT(s.ld == 129 && s.nb == 4 && s.waves == 3 && s.floats == 3200 + 3 * 4128 && s.floats <= kChainWideLdsFloats);
    EXPECT(!takes(f, 128) && takes(g, 128) && plan(g, 128).ld == 129 && plan(g, 128).waves == 3); }
  // three blocks count as the four-block class: cut; a LayerNorm's width counts for ld, not for the weight chunk
  { const Fn f{3, {20, 65, 1}, {1, 0, 0}}, g{3, {20, 64, 1}, {1, 0, 0}};
    EXPECT(!takes(f, 20) && plan(f, 20).nb == 4 && plan(f, 20).np == 96 && plan(f, 20).ld == 81 && takes(g, 20)); }
  { const Fn f{2, {100, 8}, {1, 0}};
    EXPECT(takes(f, 100) && plan(f, 100).np == 32 && plan(f, 100).ld == 113); }
  // outside: by width, by a single layer, by a Dropout entry, and a function of the narrow rule is not wide
  { const Fn w129{2, {129, 3}, {0}}, one_layer{1, {64}, {0}}, drop{3, {64, 64, 3}, {0, 2, 0}}, narrow{2, {32, 3}, {0}}, hidden0{2, {64, 0}, {0}};
    EXPECT(!takes(w129, 20) && !takes(one_layer, 20) && !takes(drop, 20) && !takes(hidden0, 20));
    const gnx_chain c = chain(narrow);
    EXPECT(chain_narrow_takes(c, 32, 1000) && !chain_wide_takes(c, 32, 1000) && chain_wide_takes(c, 33, 1000)); }
  if (fails) return 1;
  std::printf("chain wide rule ok\n");
  return 0;
}
"""


def test_the_rule_compiled_alone(tmp_path):
    src = tmp_path / "chain_wide_rule.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "chain_wide_rule"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "graphnets.jl_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "chain wide rule ok" in out.stdout, out.stdout[-4000:] + out.stderr
