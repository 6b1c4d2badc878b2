"""CPU-side checks of gnx_chain_block_backward_wide and its two queries: declared, exported and bound with the narrow pullback trio's parameter
lists, NULL arguments refused as the narrow entry refuses them, the Python entry table; the rule chain_bw_wide_takes and its plan
(csrc/gnx_chain_plan.h) compiled alone as plain C++."""
import os
import re
import subprocess

import graphnets_jl_amd as gn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_chain_block_backward_wide_applies", "gnx_chain_block_backward_wide_workspace_bytes", "gnx_chain_block_backward_wide")


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
    null = (None,) * 8 + (1,) + (None,) * 5 + (0, None)
    assert lib.gnx_chain_block_backward_wide_applies(None, None, 1) == lib.gnx_chain_block_backward_narrow_applies(None, None, 1) == 0
    assert lib.gnx_chain_block_backward_wide_workspace_bytes(None, None, 1) == lib.gnx_chain_block_backward_narrow_workspace_bytes(None, None, 1) == 0
    assert lib.gnx_chain_block_backward_wide(*null) == lib.gnx_chain_block_backward_narrow(*null) == gn._lib.ERR_INVALID_ARG


def test_the_entry_table():
    F32, BF16, e = gn._lib.ELEM_F32, gn._lib.ELEM_BF16, gn.api._entry
    rest = {"wave_chain_backward", "narrow_chain_backward"}
    assert "wide_chain_backward" in gn.api._SWITCHES
    assert e("chain", "backward", F32, {"wide_chain_backward"} | rest).call == "gnx_chain_block_backward_wide"
    assert e("chain", "backward", F32, {"wide_chain"} | rest) == e("chain", "backward", F32, rest)  # (the forward's switch selects no pullback)
    both = rest | {"bf16_chain", "bf16_backward"}
    assert e("chain", "backward", BF16, both | {"wide_chain_backward"}) == e("chain", "backward", BF16, both)
    assert e("chain", "backward", F32, rest | {"wide_chain_backward", "chain_dropout"}, True) == e("chain", "backward", F32, rest | {"chain_dropout"}, True)
    blk = gn.GNBlock((3, 2, 1), (1, 1, 1), device="cpu", wide_chain_backward=True)
    assert blk.wide_chain_backward is True and gn.GNBlock((3, 2, 1), (1, 1, 1), device="cpu").wide_chain_backward is False


# The plan in floats.  [64, 64, 3] behind 20 inputs: the tape is 32 (the input row padded to 16) + 64 + 64 + 16 = 176 floats of slots and 16 of
# slack, ld = 193; P = 64 * 21 + 64 * 65 + 3 * 65 = 5699; 24 * 64 + 64 = 1600 floats in front of the tapes of 32 * 193 = 6176: two waves in
# 16384; dW blocks 1 * 2 + 2 * 2 + 2 * 1 = 8 = two waves of four slots; 3 forward runs of chunks + 3 on the way back (2 without entry 0's).
DRIVER = r"""
#include <cstdio>
#include "gnx_chain_plan.h"
using namespace gnx;
static const float one = 1.f;
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
struct Fn { int n, w[16], kind[16], act[16]; };  // kind: 0 Dense, 1 LayerNorm, 2 Dropout
static gnx_dense layers[16];
static int32_t widths[16];
static gnx_chain chain(const Fn& f) {
  const int32_t kinds[3] = {GNX_LAYER_DENSE, GNX_LAYER_LAYERNORM, GNX_LAYER_DROPOUT};
  for (int i = 0; i < f.n; ++i) { widths[i] = f.w[i]; layers[i] = gnx_dense{&one, &one, f.act[i], kinds[f.kind[i]]}; }
  return gnx_chain{layers, widths, f.n, 0};
}
static bool takes(const Fn& f, int k_in, size_t rows = 1000) { const gnx_chain c = chain(f); return chain_bw_wide_takes(c, k_in, rows); }
static ChainBwWideShape plan(const Fn& f, int k_in, size_t rows = 1000) { const gnx_chain c = chain(f); return chain_bw_wide_shape(c, k_in, rows); }
int main() {
  { const Fn f{3, {64, 64, 3}, {0}, {0}};
    const ChainBwWideShape s = plan(f, 20);
    EXPECT(takes(f, 20) && s.ld == 193 && s.P == 5699 && s.waves == 2 && s.nb == 2 && s.tape_off == 1600 && s.floats == 1600 + 2 * 6176);
    EXPECT(s.floats <= kChainBwWideLdsFloats && s.n_blocks == 8 && s.n_items == 5 && s.n_items_dx0 == 6);
    EXPECT(s.in_off[0] == 0 && s.out_off[0] == 32 && s.out_off[1] == 96 && s.out_off[2] == 160 && s.part_off[1] == 1344 && s.part_off[2] == 5504);
    EXPECT(s.ntiles == 16 && s.nwg == 16 && plan(f, 20, 64 * 512 + 1).ntiles == 513 && plan(f, 20, 64 * 512 + 1).nwg == 512);
    EXPECT(kChainBwWideGrid == 512 && plan(f, 20, 10000000).nwg == 512 && plan(f, 20, 100000000).nwg == 512);  // the grid stops growing with the rows
    EXPECT(!takes(f, 20, 0)); }
  // a gelu Dense keeps its pre-activation, a LayerNorm four floats of statistics
  { const Fn f{3, {20, 40, 3}, {1, 0, 0}, {0, GNX_ACT_GELU, 0}};
    const ChainBwWideShape s = plan(f, 20);
    EXPECT(takes(f, 20) && s.out_off[0] == 32 && s.aux_off[0] == 64 && s.out_off[1] == 68 && s.aux_off[1] == 116 && s.out_off[2] == 164 && s.ld == 197 && s.P == 40 + 40 * 21 + 3 * 41); }
  // outside: the forward's cut class, one layer, a Dropout entry, a function of the narrow rule, a width beyond 128, more than eight entries,
  // a tape beyond two waves' budget
  { const Fn cut{3, {128, 128, 128}, {0}, {0}}, one_layer{1, {64}, {0}, {0}}, drop{3, {64, 64, 3}, {0, 2, 0}, {0}}, narrow{2, {32, 3}, {0}, {0}}, w129{2, {129, 3}, {0}, {0}};
    const Fn nine{9, {40, 8, 8, 8, 8, 8, 8, 8, 3}, {0}, {0}}, tall{4, {64, 64, 64, 3}, {0}, {0}};
    EXPECT(!takes(cut, 128) && !takes(one_layer, 20) && !takes(drop, 20) && !takes(narrow, 32) && !takes(w129, 20) && !takes(nine, 20) && !takes(tall, 20));
    const gnx_chain c = chain(tall);
    EXPECT(chain_wide_takes(c, 20, 1000) && plan(tall, 20).waves == 0); }
  if (fails) return 1;
  std::printf("chain bw wide rule ok\n");
  return 0;
}
"""


def test_the_rule_compiled_alone(tmp_path):
    src = tmp_path / "chain_bw_wide_rule.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "chain_bw_wide_rule"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "graphnets.jl_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "chain bw wide rule ok" in out.stdout, out.stdout[-4000:] + out.stderr
