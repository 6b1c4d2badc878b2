"""The table of ahead-of-time narrow block kernels (graphnets.jl_amd/csrc/gnx_narrow_sets.h), compiled on its own with g++: every row's mask
against the table written out here, the wave-tile rule, and — from the printed rows and the rules stated below — the exact set of kernels
gnx_narrow.hip and gnx_narrow_bf16.hip must instantiate."""
import functools
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphnets.jl_amd", "csrc")

PLAIN, RUN1, RUNG, CARRY1, CARRYG, LN, FFE = (1 << i for i in range(7))
RUNS = PLAIN | RUN1 | RUNG
CARRIES = RUNS | CARRY1 | CARRYG
# (element, (de, dn, dg, oe, on)): forms
TABLE = {
    ("f32", (10, 5, 0, 3, 4)): CARRIES,
    ("f32", (3, 4, 5, 3, 4)): CARRIES,
    ("f32", (10, 5, 3, 3, 4)): CARRIES,
    ("f32", (0, 2, 0, 2, 2)): CARRIES,
    ("f32", (4, 3, 2, 3, 4)): CARRIES,
    ("f32", (2, 2, 2, 2, 2)): RUNS,
    ("f32", (8, 8, 8, 16, 8)): PLAIN,
    ("f32", (10, 5, 0, 10, 5)): PLAIN,
    ("f32", (10, 5, 3, 10, 5)): PLAIN | LN | FFE,
    ("bf16", (10, 5, 0, 3, 4)): PLAIN | RUN1,
    ("bf16", (3, 4, 5, 3, 4)): RUNS,
    ("bf16", (10, 5, 3, 10, 5)): LN | FFE,
}
# not listed: a permutation of a row, a row with one width off, sets only the other element type has, a run-time specialised set, zeros
UNLISTED = [("f32", (5, 10, 0, 3, 4)), ("f32", (10, 5, 0, 3, 5)), ("f32", (10, 5, 1, 3, 4)), ("f32", (7, 3, 2, 5, 6)), ("f32", (0, 0, 0, 0, 0)),
            ("bf16", (10, 5, 3, 3, 4)), ("bf16", (2, 2, 2, 2, 2)), ("bf16", (8, 8, 8, 16, 8)), ("bf16", (10, 5, 0, 10, 5)), ("bf16", (3, 4, 5, 4, 3))]
CAPS = (64, 128, 256, 100)
CAP_WIDTHS = [(10, 5), (8, 8), (9, 8), (16, 1), (0, 0), (32, 32), (3, 4)]  # 256 edges per wave tile: four rows of (de + dn) floats within 64

DRIVER = r"""
#include <cstdio>
#include "gnx_narrow_sets.h"
using namespace gnx;
static_assert(NF_PLAIN == 1 && NF_RUN1 == 2 && NF_RUNG == 4 && NF_CARRY1 == 8 && NF_CARRYG == 16 && NF_LN == 32 && NF_FFE == 64, "the bits the test names");
static_assert(narrow_forms(10, 5, 3, 10, 5, false) == (NF_PLAIN | NF_LN | NF_FFE) && !narrow_forms(10, 5, 3, 10, 6, true), "usable in constant expressions");
template <class... S>
static void rows(const char* elem, bool bf16, NarrowSetList<S...>) {
  (std::printf("row %s %d %d %d %d %d %u %u\n", elem, S::DE, S::DN, S::DG, S::OE, S::ON, S::forms, narrow_forms(S::DE, S::DN, S::DG, S::OE, S::ON, bf16)), ...);
}
int main() {
  rows("f32", false, NarrowSetsF32{});
  rows("bf16", true, NarrowSetsBF16{});
  static const int q[][6] = {@QUERIES@};
  for (const auto& s : q) std::printf("query %s %d %d %d %d %d %u\n", s[0] ? "bf16" : "f32", s[1], s[2], s[3], s[4], s[5], narrow_forms(s[1], s[2], s[3], s[4], s[5], s[0]));
  static const int w[][2] = {@WIDTHS@};
  static const int caps[] = {@CAPS@};
  for (const auto& d : w)
    for (int cap : caps) std::printf("cap %d %d %d %d\n", d[0], d[1], cap, (int)narrow_cap_ok(d[0], d[1], cap));
  return 0;
}
"""


@functools.lru_cache(None)
def printed():
    """the driver's output lines, split into fields (compiled and run once per session)"""
    queries = ", ".join("{%d, %s}" % (e == "bf16", ", ".join(map(str, s))) for e, s in list(TABLE) + UNLISTED)
    text = DRIVER.replace("@QUERIES@", queries).replace("@WIDTHS@", ", ".join("{%d, %d}" % w for w in CAP_WIDTHS)).replace("@CAPS@", ", ".join(map(str, CAPS)))
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "narrow_sets.cpp"), os.path.join(tmp, "narrow_sets")
        with open(src, "w") as f:
            f.write(text)
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr
    return [ln.split() for ln in out.stdout.splitlines()]


def table_rows():
    """{(element, widths): forms} of the header's two lists"""
    return {(f[1], tuple(map(int, f[2:7]))): int(f[7]) for f in printed() if f[0] == "row"}


def test_narrow_sets_header():
    lines = printed()
    rows = [f for f in lines if f[0] == "row"]
    assert len(rows) == len(TABLE) == len(table_rows()), "a width set is listed twice"
    assert table_rows() == TABLE
    assert all(f[7] == f[8] for f in rows), "narrow_forms disagrees with a row"
    queries = {(f[1], tuple(map(int, f[2:7]))): int(f[7]) for f in lines if f[0] == "query"}
    assert queries == {**TABLE, **{k: 0 for k in UNLISTED}}
    caps = {tuple(map(int, f[1:4])): int(f[4]) for f in lines if f[0] == "cap"}
    assert caps == {(de, dn, cap): int(cap in (64, 128) or (cap == 256 and (de + dn) * 4 <= 64)) for de, dn in CAP_WIDTHS for cap in CAPS}
    assert caps[(8, 8, 256)] == 1 and caps[(9, 8, 256)] == 0 and caps[(10, 5, 100)] == 0


def _mangle(kernel, ints, bools, args="NS_9BlockArgsEi"):
    return f"_ZN3gnx{len(kernel)}{kernel}I" + "".join(f"Li{v}E" for v in ints) + "".join(f"Lb{int(b)}E" for b in bools) + "EEv" + args


def expected_kernels(elem, rows):
    """What the file of `elem` instantiates for its rows.  Templates (gnx_wave_kernel.h), ONEG = one graph, every form in both unless stated:
      k_block_wave<widths, EPT, LN, ONEG, PACK, false, CHAIN, BF16>    k_graph_t<oe + on, ONEG, BF16, bf16 rows out>
      k_block_wave_ffe<widths, EPT, ONEG, BF16>   k_block_wave_run<widths, EPT, ONEG, BF16>   k_graph_run<oe + on, ONEG, BF16>   k_block_wave_carry<widths, EPT, ONEG>
    PLAIN: EPT 1, 2 and (narrow_cap_ok at 256) 4; at EPT 2 also PACK (several graphs only) and CHAIN; its graph update writes the rows' type.
    LN, FFE: EPT 2, fp32 out whatever the rows.  RUN1 / RUNG, CARRY1 / CARRYG: EPT 2, the one form each."""
    b = elem == "bf16"
    run_args, names = "NS_9BlockArgsENS_8RunTableEi", set()
    for (e, s), forms in rows.items():
        if e != elem:
            continue
        c = s[3] + s[4]
        if forms & PLAIN:
            for ept in (1, 2) + ((4,) if (s[0] + s[1]) * 4 <= 64 else ()):
                names |= {_mangle("k_block_wave", s + (ept,), (0, g, 0, 0, 0, b)) for g in (0, 1)}
            names.add(_mangle("k_block_wave", s + (2,), (0, 0, 1, 0, 0, b)))
            names |= {_mangle("k_block_wave", s + (2,), (0, g, 0, 0, 1, b)) for g in (0, 1)}
            names |= {_mangle("k_graph_t", (c,), (g, b, b)) for g in (0, 1)}
        if forms & LN:
            names |= {_mangle("k_block_wave", s + (2,), (1, g, 0, 0, 0, b)) for g in (0, 1)}
        if forms & FFE:
            names |= {_mangle("k_block_wave_ffe", s + (2,), (g, b)) for g in (0, 1)}
        if forms & (LN | FFE):
            names |= {_mangle("k_graph_t", (c,), (g, b, 0)) for g in (0, 1)}
        for g, run, carry in ((1, RUN1, CARRY1), (0, RUNG, CARRYG)):
            if forms & run:
                names |= {_mangle("k_block_wave_run", s + (2,), (g, b), run_args), _mangle("k_graph_run", (c,), (g, b), run_args)}
            if forms & carry:
                names.add(_mangle("k_block_wave_carry", s + (2,), (g,), "NS_9BlockArgsENS_8RunTableENS_9PrevTableEi"))
    return names


def test_the_two_files_instantiate_exactly_what_the_table_names():
    from tools.kernel_resources import HIPCC, remarks_many
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    rows = table_rows()
    assert not any(forms & (CARRY1 | CARRYG) for (e, _), forms in rows.items() if e == "bf16"), "the carrying kernel has no bf16 form"
    pat = re.compile(r"_ZN3gnx\d+(k_block_wave|k_graph_t|k_graph_run)")
    for elem, res in zip(("bf16", "f32"), remarks_many(["gnx_narrow_bf16.hip", "gnx_narrow.hip"])):
        got, want = {n for n in res if pat.match(n)}, expected_kernels(elem, rows)
        assert got == want, (elem, "missing:", sorted(want - got), "not in the table:", sorted(got - want))
