"""CPU-side checks of gnx_chain_block_forward_wave_typed and its two queries: declared, exported and bound with matching parameter counts, a NULL
handle refused; api._entry selects the call only with `wave_chain` and `bf16_chain` on bfloat16 features; the rule chain_wave_typed_takes /
chain_wave_typed_waves (csrc/gnx_chain_plan.h) compiled alone as plain C++ on its LDS boundaries, the nf' staging's included."""
import os
import re
import subprocess

import graphnets_jl_amd as gn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_chain_block_forward_wave_typed_applies", "gnx_chain_block_forward_wave_typed_workspace_bytes", "gnx_chain_block_forward_wave_typed")


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
    assert lib.gnx_version() == 130
    for elem in (gn._lib.ELEM_F32, gn._lib.ELEM_BF16, 99):
        assert lib.gnx_chain_block_forward_wave_typed_applies(None, None, 1, elem) == 0
        assert lib.gnx_chain_block_forward_wave_typed_workspace_bytes(None, None, 1, elem) == 0
        assert lib.gnx_chain_block_forward_wave_typed(None, None, elem, None, None, None, 1, None, None, None, None, 0, 0, None) == gn._lib.ERR_INVALID_ARG


def test_entry_selects_the_call_with_both_switches_on_bf16():
    F32, BF16 = gn._lib.ELEM_F32, gn._lib.ELEM_BF16
    e = gn.api._entry("chain", "forward", BF16, {"wave_chain", "bf16_chain", "narrow_chain"})
    assert e == gn.api._Entry(NEW[1], (BF16,), NEW[2], (BF16,), ("flags",), ("chain_wave_bf16", "in_dims", "widths", "R"))
    assert gn.api._entry("chain", "forward", BF16, {"bf16_chain", "narrow_chain"}).call == "gnx_chain_block_forward_typed"
    assert gn.api._entry("chain", "forward", F32, {"wave_chain", "bf16_chain"}).call == "gnx_chain_block_forward_wave"
    assert gn.api._entry("chain", "backward", BF16, {"wave_chain", "bf16_chain", "bf16_backward"}).call == "gnx_chain_block_backward_typed"


# cap = 128.  par: the zero-padded parameter floats of the edge and the node function; slice = max(128 (oe | 1), 64 (on | 1)) floats per wave
DRIVER = r"""
#include <cstdio>
#include "gnx_chain_plan.h"
using namespace gnx;
static const float one = 1.f;
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
struct Fn { int n, w[16]; };
static gnx_dense layers[3][16];
static int32_t widths[3][16];
static ChainShape shape(int de, const Fn& e, const Fn& nd, long long G = 1) {
  static gnx_chain_block_params p;
  p = gnx_chain_block_params{};
  p.de = de;
  const Fn* f[2] = {&e, &nd};
  gnx_chain* c[2] = {&p.edgefn, &p.nodefn};
  for (int t = 0; t < 2; ++t) {
    for (int i = 0; i < f[t]->n; ++i) { widths[t][i] = f[t]->w[i]; layers[t][i] = gnx_dense{&one, &one, GNX_ACT_IDENTITY, GNX_LAYER_DENSE}; }
    c[t]->layers = layers[t]; c[t]->widths = widths[t]; c[t]->n_layers = f[t]->n;
  }
  return chain_shape(4099, 1031, G, p, 1);
}
int main() {
  // oe = 8, on = 4: the ef' rows decide (128 * 9 = 1152 > 64 * 5) and the rule is the fp32 form's; the cut and the in-degree cap are inherited
  { const Fn e{2, {16, 8}}, nd{1, {4}};
    const ChainShape s = shape(6, e, nd);
    EXPECT(chain_wave_typed_slice(s, 128) == 1152 && chain_wave_typed_waves(s, 128) == 4 && chain_wave_typed_bytes(s, 77) == 256);
    EXPECT(chain_wave_typed_takes(s, 128, 128) && !chain_wave_typed_takes(s, 129, 128));
    EXPECT(chain_wave_typed_takes(shape(17, e, nd), 128, 128) && !chain_wave_typed_takes(shape(17, e, nd, 3), 128, 128)); }
  // oe = 4, on = 32: the nf' staging decides — 64 * 33 = 2112 > 128 * 5 = 640.  edge 6 -> 32 (288 floats), k x 32 -> 32 (1056 each), 32 -> 4 (132);
  // node 4 -> 32 (160), j x 32 -> 32: par = 580 + 1056 (k + j).  Four slices: par <= 16384 - 8448 = 7936; two: par <= 12160
  for (int k = 5; k <= 8; ++k) for (int j = 1; j <= 3; ++j) {
    Fn e{0, {0}}, nd{0, {0}};
    for (int i = 0; i <= k; ++i) e.w[e.n++] = 32;
    e.w[e.n++] = 4;
    for (int i = 0; i <= j; ++i) nd.w[nd.n++] = 32;
    const ChainShape s = shape(6, e, nd);
    const size_t par = chain_narrow_lds_floats(*s.ch[0], s.k0[0]) + chain_narrow_lds_floats(*s.ch[1], s.k0[1]);
    EXPECT(par == 580 + 1056 * (size_t)(k + j) && chain_wave_typed_slice(s, 128) == 2112);
    EXPECT(chain_wave_typed_waves(s, 128) == (par <= 7936 ? 4 : par <= 12160 ? 2 : 0) && chain_wave_waves(s, 128) == 4);  // (the fp32 slice: 640 floats)
    EXPECT(chain_wave_typed_takes(s, 128, 128) == (par <= 12160)); }
  if (fails) return 1;
  std::printf("chain wave typed rule ok\n");
  return 0;
}
"""


def test_the_rule_compiled_alone(tmp_path):
    src = tmp_path / "chain_wave_typed_rule.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "chain_wave_typed_rule"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "graphnets.jl_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "chain wave typed rule ok" in out.stdout, out.stdout[-4000:] + out.stderr
