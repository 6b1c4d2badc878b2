"""Register / LDS / scratch use of the fused narrow edge pullback (k_bw_edge_wave, k_bw_edge_wave_bf16: csrc/gnx_bw_edge_wave_kernel.h) for a list
of width sets, read from hipcc's resource remarks — no GPU needed.  The kernel header is compiled for gfx950 with explicit instantiations of
the listed sets, with the options build.py gives gnx_backward_narrow.hip (the run-time specialiser of gnx_jit.cpp compiles the same text).

    python tools/bw_narrow_resources.py            # writes profiles/bw_narrow_resources.json

Default list: the five ahead-of-time sets, the sets tests/test_bw_narrow_abi.py precompiles, and the corners of the eligibility rule
(oe * Ke < 64, static LDS <= 64 KB): two pair slots per lane ((6,6,3)=>3: 66 pairs, (2,3,1)=>7: 70, (0,1,0)=>9: 27 ... (1,0,0)=>31: 62 pairs on one
slot, (0,0,1)=>62 is refused by the LDS rule), the widest rows ((20,16,10)=>1: Ke = 62)."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphnets.jl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
AOT_SETS = ((10, 5, 0, 3), (3, 4, 5, 3), (0, 2, 0, 2), (2, 2, 2, 2), (4, 3, 2, 3))  # (de, dn, dg, oe): gnx_backward_narrow.hip
SETS = AOT_SETS + ((3, 2, 4, 3), (2, 3, 1, 7), (6, 6, 3, 3), (5, 5, 5, 3), (20, 10, 4, 1), (20, 16, 10, 1), (1, 0, 0, 1), (0, 1, 0, 9), (0, 0, 1, 5),
                   (1, 0, 0, 31))


def eligible(de, dn, dg, oe):
    """the rule of jit_bw_edge_eligible (csrc/gnx_jit.cpp) with run-time specialisation enabled and no LDS padding"""
    ke = de + 2 * dn + dg
    if min(de, dn, dg) < 0 or oe < 1 or ke < 1 or oe * ke >= 64:
        return False
    return static_lds(de, dn, dg, oe) <= 64 * 1024


def static_lds(de, dn, dg, oe):
    ke = de + 2 * dn + dg
    ps = (oe * (ke + 1) + 63) // 64
    return 4 * 4 * (64 * ((oe + ke) | 1) + 64 * ps)


def resources(sets=SETS, hipcc=HIPCC):
    """{"(de, dn, dg, oe)": {"fp32": {sgpr, vgpr, scratch, lds, waves_per_simd}, "bf16": {...}}}"""
    for s in sets:
        assert eligible(*s), f"{s} is not an eligible width set"
    lines = ['#include "gnx_bw_edge_wave_kernel.h"', "namespace gnx {"]
    for de, dn, dg, oe in sets:
        lines.append(f"template __global__ void k_bw_edge_wave<{de}, {dn}, {dg}, {oe}>(BwEdgeWave);")
        lines.append(f"template __global__ void k_bw_edge_wave_bf16<{de}, {dn}, {dg}, {oe}>(BwEdgeWave);")
    lines.append("}")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "bw_narrow_sets.hip")
        with open(src, "w") as f:
            f.write("\n".join(lines) + "\n")
        cmd = [hipcc, "-x", "hip", "-c", "--cuda-device-only", "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
               "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, src]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        m = re.match(r"_ZN3gnx\d+k_bw_edge_wave(_bf16)?ILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEEv", blk.split()[0])
        if not m:
            continue
        g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))
        key = str(tuple(int(v) for v in m.groups()[1:]))
        out.setdefault(key, {})["bf16" if m.group(1) else "fp32"] = dict(
            sgpr=g("TotalSGPRs"), vgpr=g("VGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"), lds=g(r"LDS Size \[bytes/block\]"),
            waves_per_simd=g(r"Occupancy \[waves/SIMD\]"))
    return out


def main():
    res = resources()
    rec = dict(what="k_bw_edge_wave / k_bw_edge_wave_bf16 per (de, dn, dg, oe): hipcc -O3 --offload-arch=gfx950 resource remarks", sets={})
    for s in SETS:
        de, dn, dg, oe = s
        ke = de + 2 * dn + dg
        rec["sets"][str(s)] = dict(ke=ke, pairs=oe * (ke + 1), pair_slots=(oe * (ke + 1) + 63) // 64, ahead_of_time=s in AOT_SETS, **res[str(s)])
    path = os.path.join(ROOT, "profiles", "bw_narrow_resources.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    for k, v in rec["sets"].items():
        print(k, v["pairs"], {e: (v[e]["sgpr"], v[e]["vgpr"], v[e]["lds"], v[e]["scratch"], v[e]["waves_per_simd"]) for e in ("fp32", "bf16")})
    print("wrote", path)


if __name__ == "__main__":
    sys.exit(main())
