"""The two training rules of a Chain block with Dropout entries (include/gnx.h, gnx_chain_block_forward_train / _backward_train) restated in
Python and checked against graphnets.jl_amd/csrc/gnx_chain_plan.h compiled on its own with g++, as tests/test_chain_plan_cpu.py does for the
test-mode rules: the forward rule (a Dropout entry stages 0 parameter floats), the pullback rule (an entry that is not last takes a tape slot of
its width, contributes 0 to par, 0 to P and nothing to the delta slot), the LDS plan behind it, and that the plans of chains without Dropout
entries are what they were."""
import os
import subprocess

from tests.test_chain_bw_narrow_abi import ceil4, formula_takes
from tests.test_chain_plan_cpu import forward_takes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE, LN, DROP = 0, 1, 2


def train_plan(k_in, entries):
    """(par, P, ld) of include/gnx.h's training formulas.  entries: [(width, DENSE | LN | DROP)] in the order of the call's chain"""
    par = P = dmax = 0
    k, slots, n = k_in, k_in, len(entries)
    for i, (w, kind) in enumerate(entries):
        if kind == DENSE:
            par += ceil4(k) * ceil4(w) + ceil4(w); P += w * (k + 1); dmax = max(dmax, w)
        elif kind == LN:
            par += 2 * ceil4(w); P += 2 * w; dmax = max(dmax, 2 * w)
        if i + 1 < n:
            slots += w  # (a Dropout entry too: the dropped row is the next Dense's input)
        k = w
    return par, P, (slots + dmax) | 1


def train_forward_takes(k_in, entries, rows=1):
    n = len(entries)
    if n < 1 or n > 16 or rows == 0 or entries[-1][0] <= 0 or k_in > 32 or any(w > 32 for w, _ in entries):
        return False
    return train_plan(k_in, entries)[0] <= 10240


def train_backward_takes(k_in, entries, rows=1):
    if not train_forward_takes(k_in, entries, rows):
        return False
    par, P, ld = train_plan(k_in, entries)
    return par + 2 * (64 * ld + P) <= 16384


def train_masks(in_dims, chains, counts):
    """(forward mask, pullback mask) of a block: chains = three entry lists, counts = (E, N, G)"""
    de, dn, dg = in_dims
    out = lambda es: es[-1][0] if es else 0
    k = (de + 2 * dn + dg, out(chains[0]) + dn + dg, out(chains[0]) + out(chains[1]) + dg)
    fw = sum(1 << t for t in range(3) if chains[t] and train_forward_takes(k[t], chains[t], counts[t]))
    # the cut class (include/gnx.h, measured): an edge function with Dropout entries at register width 32 runs the generic training pullback
    cut = lambda t: t == 0 and any(kind == DROP for _, kind in chains[t]) and max([k[t]] + [w for w, _ in chains[t]]) > 16
    bw = sum(1 << t for t in range(3) if chains[t] and train_backward_takes(k[t], chains[t], counts[t]) and not cut(t))
    return fw, (bw if out(chains[0]) > 0 else 0)


D, L_, X = DENSE, LN, DROP
CASES = [  # (name, k_in, entries)
    ("[16,do,3] at k_in 20", 20, [(16, D), (16, X), (3, D)]),
    ("[32,do,32,do,3]", 23, [(32, D), (32, X), (32, D), (32, X), (3, D)]),
    ("[32,do,32,do,3] at k_in 8", 8, [(32, D), (32, X), (32, D), (32, X), (3, D)]),
    ("a Dropout as last entry", 11, [(8, D), (4, D), (4, X)]),
    ("eight 8-wide layers, a Dropout after each", 8, [e for _ in range(8) for e in ((8, D), (8, X))]),
    ("behind a LayerNorm", 23, [(16, D), (16, L_), (16, X), (3, D)]),
    ("[32,do,4] at k_in 11", 11, [(32, D), (32, X), (4, D)]),
    ("width 33", 20, [(33, D), (33, X), (3, D)]),
    ("no rows", 20, [(16, D), (16, X), (3, D)]),
]
ROWS = {"no rows": 0}
STRIPPED = [(20, [16, 3], ()), (23, [32, 32, 3], ()), (11, [8, 4], ()), (8, [8] * 8, ()), (23, [16, 16, 3], (1,)), (4, [14, 17, 23, 32], ()), (31, [31, 1], (0,))]


def _table():
    rows = []
    for name, k_in, es in CASES:
        r = ROWS.get(name, 1031)
        par, P, ld = train_plan(k_in, es)
        rows.append('  {"%s", %d, %d, {%s}, {%s}, %d, %d, %d, %d, %d, %d},' % (
            name, k_in, len(es), ", ".join(str(w) for w, _ in es), ", ".join(str(k) for _, k in es), r, train_forward_takes(k_in, es, r),
            train_backward_takes(k_in, es, r), par, P, ld))
    return "\n".join(rows)


def _stripped_table():
    rows = []
    for k_in, ws, ln in STRIPPED:
        kinds = [LN if i in ln else DENSE for i in range(len(ws))]
        es = list(zip(ws, kinds))
        assert train_forward_takes(k_in, es) == forward_takes(k_in, ws, ln) and train_backward_takes(k_in, es) == formula_takes(k_in, ws, ln)
        rows.append("  {\"stripped\", %d, %d, {%s}, {%s}, 1031, %d, %d, %d, %d, %d}," % (
            k_in, len(ws), ", ".join(map(str, ws)), ", ".join(map(str, kinds)), forward_takes(k_in, ws, ln), formula_takes(k_in, ws, ln), *train_plan(k_in, es)))
    return "\n".join(rows)


DRIVER = r"""
#include <cstdio>
#include "gnx_chain_plan.h"
using namespace gnx;
static int fails = 0;
static const char* ctx = "";
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL line %d: %s [%s]\n", __LINE__, #c, ctx); ++fails; } } while (0)
struct Case { const char* name; int k_in, n, w[16], kind[16]; long long rows; int fw, bw, par, P, ld; };
static const Case cases[] = {
@CASES@
@STRIPPED@
};
static const float one = 1.f;
static const ChainDropSite site{7, 0.25f, 16};
int main() {
  for (const Case& c : cases) {
    ctx = c.name;
    gnx_dense layers[16]; int32_t widths[16];
    for (int i = 0; i < c.n; ++i) {
      widths[i] = c.w[i];
      layers[i] = c.kind[i] == 2 ? gnx_dense{nullptr, reinterpret_cast<const float*>(&site), GNX_ACT_IDENTITY, GNX_LAYER_DROPOUT}
                                 : gnx_dense{&one, &one, GNX_ACT_IDENTITY, c.kind[i] == 1 ? GNX_LAYER_LAYERNORM : GNX_LAYER_DENSE};
    }
    gnx_chain ch{};
    ch.layers = layers; ch.widths = widths; ch.n_layers = c.n;
    bool has = false;
    for (int i = 0; i < c.n; ++i) has = has || c.kind[i] == 2;
    EXPECT(chain_has_dropout(ch) == has);
    EXPECT(chain_narrow_takes(ch, c.k_in, (size_t)c.rows) == (bool)c.fw);
    EXPECT(chain_bw_narrow_takes(ch, c.k_in, (size_t)c.rows) == (bool)c.bw);
    EXPECT(chain_rule_takes(CHAIN_RULE_FW, ch, c.k_in, (size_t)c.rows) == (bool)c.fw && chain_rule_takes(CHAIN_RULE_BW, ch, c.k_in, (size_t)c.rows) == (bool)c.bw);
    EXPECT((int)chain_narrow_lds_floats(ch, c.k_in) == c.par);
    const ChainBwNarrowShape sh = chain_bw_narrow_shape(ch, c.k_in, (size_t)c.rows);
    EXPECT(sh.par_floats == c.par && sh.P == c.P && sh.ld == c.ld);
    // the tape: the input row, then every entry's output but the last in the order of the chain; a Dropout entry owns no parameters
    int slot = c.k_in;
    for (int i = 0; i < c.n; ++i) {
      EXPECT(sh.tape_out[i] == slot);
      if (i + 1 < c.n) slot += c.w[i];
      if (c.kind[i] == 2) EXPECT((i + 1 == c.n ? sh.par_floats : sh.par_off[i + 1]) == sh.par_off[i] && (i + 1 == c.n ? sh.P : sh.part_off[i + 1]) == sh.part_off[i]);
    }
    EXPECT(sh.dslot == slot && sh.ld > sh.dslot);
    if (c.bw) EXPECT(sh.waves >= 2 && sh.par_floats + sh.waves * (64 * sh.ld + sh.P) <= kChainBwLdsFloats);
  }
  if (fails) return 1;
  std::printf("chain train plan ok\n");
  return 0;
}
"""


def test_the_restatement_on_the_named_cases():
    by = {n: (k, es) for n, k, es in CASES}
    assert train_forward_takes(*by["[16,do,3] at k_in 20"]) and train_backward_takes(*by["[16,do,3] at k_in 20"])
    assert train_forward_takes(*by["[32,do,32,do,3]"]) and not train_backward_takes(*by["[32,do,32,do,3]"])  # two waves' tapes do not fit 64 KB
    assert train_backward_takes(*by["a Dropout as last entry"])
    # sixteen entries: the forward takes it; the tape of 8 + 15 * 8 + 8 floats per lane leaves no room for two waves (576 + 2 (64 * 137 + 576) = 19264)
    assert train_forward_takes(*by["eight 8-wide layers, a Dropout after each"]) and not train_backward_takes(*by["eight 8-wide layers, a Dropout after each"])
    assert train_plan(*by["eight 8-wide layers, a Dropout after each"]) == (576, 576, 137)
    assert not train_forward_takes(*by["width 33"]) and not train_forward_takes(*by["no rows"], rows=0)
    # a last Dropout adds a tape slot for the layer in front of it and nothing else
    assert train_plan(11, [(8, D), (4, D), (4, X)]) == (train_plan(11, [(8, D), (4, D)])[0], train_plan(11, [(8, D), (4, D)])[1], (11 + 8 + 4 + 8) | 1)
    assert train_masks((10, 5, 0), [[(16, D), (16, X), (3, D)], [(8, D), (8, X), (4, D)], [(6, D), (5, D)]], (100, 30, 5)) == (7, 6)  # k_in 20: the cut class
    assert train_masks((3, 2, 1), [[(16, D), (16, X), (3, D)], [(8, D), (8, X), (4, D)], [(6, D), (5, D)]], (100, 30, 5)) == (7, 7)
    assert train_masks((10, 5, 0), [[(16, D), (3, D)], [(8, D), (8, X), (4, D)], [(6, D), (5, D)]], (100, 30, 5)) == (7, 7)  # no Dropout: the test-mode rule
    assert train_masks((10, 5, 0), [[(16, D), (16, X), (3, D)], [], []], (0, 30, 5)) == (0, 0)


def test_chain_train_plan_header(tmp_path):
    src = tmp_path / "chain_train_plan.cpp"
    src.write_text(DRIVER.replace("@CASES@", _table()).replace("@STRIPPED@", _stripped_table()))
    exe = tmp_path / "chain_train_plan"
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "graphnets.jl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr
    assert "chain train plan ok" in out.stdout
