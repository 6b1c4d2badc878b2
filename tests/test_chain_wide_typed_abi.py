"""CPU-side checks of gnx_chain_block_forward_wide_typed and its two queries: declared, exported and bound with the wave-typed trio's parameter
lists, NULL arguments and a bad `elem` refused as that trio refuses them; the native rule and the layout arithmetic of the bf16 wide form
(csrc/gnx_chain_plan.h) compiled alone as plain C++ and checked on a native, a staged and a mask-0 block."""
import os
import re
import subprocess

import graphnets_jl_amd as gn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_chain_block_forward_wide_typed_applies", "gnx_chain_block_forward_wide_typed_workspace_bytes", "gnx_chain_block_forward_wide_typed")


def test_entries_declared_exported_bound_and_refuse_null_and_bad_elem():
    import __graft_entry__ as ge
    ge.build()
    lib, S, L = gn._lib.load(), gn._lib.SIGNATURES, gn._lib
    with open(os.path.join(ROOT, "include", "gnx.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        m = re.search(r"GNX_API [\w\s\*]+?\b" + name + r"\(([^;]*?)\);", text, flags=re.S)
        assert m and hasattr(lib, name) and name in S, name
        assert m.group(1).count(",") + 1 == len(S[name][1]), name
        assert S[name] == S[name.replace("_wide_typed", "_wave_typed")], name
    assert lib.gnx_version() == 130
    null = lambda elem: (None, None, elem, None, None, None, 1, None, None, None, None, 0, 0, None)
    for kind in ("wide", "wave"):
        applies, query, call = (getattr(lib, f"gnx_chain_block_forward_{kind}_typed" + s) for s in ("_applies", "_workspace_bytes", ""))
        for elem in (L.ELEM_F32, L.ELEM_BF16, 7):
            assert applies(None, None, 1, elem) == 0 and query(None, None, 1, elem) == 0, (kind, elem)
            assert call(*null(elem)) == L.ERR_INVALID_ARG, (kind, elem)
        call(*null(7))
        assert b"elem must be GNX_ELEM_F32 or GNX_ELEM_BF16" in lib.gnx_last_error(), kind


# carves are 256-byte aligned; chain_fw_layout ends with 256 bytes of slack
DRIVER = r"""
#include <cstdio>
#include <initializer_list>
#include "gnx_chain_plan.h"
using namespace gnx;
static const float one = 1.f;
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
struct Block {
  gnx_dense layers[3][4];
  int32_t widths[3][4];
  gnx_chain_block_params p;
  Block(int de, int dn, int dg, std::initializer_list<int> e, std::initializer_list<int> n, std::initializer_list<int> g) : p{} {
    const std::initializer_list<int>* w[3] = {&e, &n, &g};
    gnx_chain* ch[3] = {&p.edgefn, &p.nodefn, &p.graphfn};
    for (int t = 0; t < 3; ++t) {
      int i = 0;
      for (int v : *w[t]) { widths[t][i] = v; layers[t][i] = gnx_dense{&one, &one, GNX_ACT_IDENTITY, GNX_LAYER_DENSE}; ++i; }
      *ch[t] = gnx_chain{i ? layers[t] : nullptr, i ? widths[t] : nullptr, i, 0};
    }
    p.de = de; p.dn = dn; p.dg = dg;
  }
};
static size_t up(size_t x) { return (x + 255) / 256 * 256; }
int main() {
  const int64_t E = 1000, N = 101, G = 5;
  // native: [64, 64, 3] / [64, 4] wide, [16, 5] narrow.  The workspace: n_in [N][3 + 5 + 3], g_in [G][3 + 4 + 3], then ef' [E][3], nf' [N][4], gf [G][3]
  { Block b(10, 5, 3, {64, 64, 3}, {64, 4}, {16, 5});
    const ChainShape s = chain_shape(E, N, G, b.p, 1);
    const unsigned fused = chain_fused_mask(s, CHAIN_RULE_FW), wide = chain_wide_mask(s);
    EXPECT(fused == 4 && wide == 3 && chain_wide_typed_native(s, fused, wide) && !chain_typed_native(s, fused));
    const size_t fp32 = chain_fw_layout(s, fused, 0, 0, wide).total;
    EXPECT(fp32 == up(4 * N * 11) + up(4 * G * 10) + 256);
    EXPECT(chain_wide_typed_native_bytes(s, fused, wide, 0) == up(fp32) + up(4 * E * 3) + up(4 * N * 4) + up(4 * G * 3));
    EXPECT(chain_wide_bf16_stride(23) == 40 && chain_wide_bf16_stride(33) == 56 && chain_wide_bf16_stride(128) == 136);
    for (int k = 1; k <= 128; ++k) {  // one aligned 16-byte read per fragment, an odd number of 16-byte columns per row, inside the fp32 slice
      const int ldb = chain_wide_bf16_stride(k);
      EXPECT(ldb % 8 == 0 && (ldb / 8) % 2 == 1 && ldb >= ceil16(k) && 2 * ldb <= 4 * (ceil16(k) | 1));
    } }
  // no graph function, a narrow node function: only ef' is kept; without a node function nothing is
  { Block b(10, 5, 0, {64, 3}, {8, 4}, {}), c(10, 5, 0, {64, 3}, {}, {});
    const ChainShape s = chain_shape(E, N, G, b.p, 2), t = chain_shape(E, N, G, c.p, 1);
    EXPECT(chain_wide_mask(s) == 1 && chain_fused_mask(s, CHAIN_RULE_FW) == 2 && chain_wide_typed_native(s, 2, 1));
    EXPECT(chain_wide_typed_native_bytes(s, 2, 1, 0) == 256 + up(4 * 2 * E * 3));
    EXPECT(chain_wide_typed_native(t, 0, 1) && chain_wide_typed_native_bytes(t, 0, 1, 0) == 256); }
  // staged: a one-layer node function at width 40 is in neither mask
  { Block b(10, 5, 3, {64, 3}, {40}, {});
    const ChainShape s = chain_shape(E, N, G, b.p, 1);
    const unsigned fused = chain_fused_mask(s, CHAIN_RULE_FW), wide = chain_wide_mask(s);
    EXPECT(fused == 0 && wide == 1 && !chain_wide_typed_native(s, fused, wide)); }
  // mask 0: narrow functions alone — the typed entry's native rule decides, the wide one never holds; and a function without rows does not count
  { Block b(10, 5, 3, {16, 3}, {8, 4}, {6, 5}), c(10, 5, 3, {64, 3}, {40}, {});
    const ChainShape s = chain_shape(E, N, G, b.p, 1), t = chain_shape(E, 0, G, c.p, 1);
    EXPECT(chain_wide_mask(s) == 0 && chain_fused_mask(s, CHAIN_RULE_FW) == 7 && chain_typed_native(s, 7) && !chain_wide_typed_native(s, 7, 0));
    EXPECT(chain_wide_mask(t) == 1 && chain_wide_typed_native(t, 0, 1)); }
  if (fails) return 1;
  std::printf("chain wide typed plan ok\n");
  return 0;
}
"""


def test_the_native_rule_and_layout_compiled_alone(tmp_path):
    src = tmp_path / "chain_wide_typed_plan.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "chain_wide_typed_plan"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "graphnets.jl_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "chain wide typed plan ok" in out.stdout, out.stdout[-4000:] + out.stderr
