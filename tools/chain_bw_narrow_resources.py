"""Register / LDS / scratch use of the fused Chain pullback kernel (k_chain_mlp_bw<WMAX, SRC>, WMAX = 8, 16, 32 and the three source forms:
csrc/gnx_chain_bw_narrow.hip), read from hipcc's resource remarks — no GPU needed.  The file is compiled for gfx950 with the options build.py
gives it.  The kernel's LDS is dynamic (the staged parameters, then per wave the row tape and the accumulators, at most lds_budget_bytes): the
static figure must be 0.  The approach is tools/chain_narrow_resources.py's.

    python tools/chain_bw_narrow_resources.py            # writes profiles/chain_bw_narrow_resources.json
"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphnets.jl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
WMAX = (8, 16, 32)
SRC = ("edge", "node", "rows")
LDS_BUDGET_BYTES = 4 * 16384  # kChainBwLdsFloats (gnx_chain_plan.h)


def resources(hipcc=HIPCC):
    """{src: {WMAX: {sgpr, vgpr, agpr, scratch, lds_static, waves_per_simd}}} for every instantiation the file holds"""
    cmd = [hipcc, "-x", "hip", "-c", "--cuda-device-only", "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, os.path.join(CSRC, "gnx_chain_bw_narrow.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {s: {} for s in SRC}
    for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        m = re.match(r"_ZN3gnx\d+k_chain_mlp_bwILi(\d+)ELi(\d+)EEEv", blk.split()[0])
        if not m:
            continue
        g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))
        out[SRC[int(m.group(2))]][int(m.group(1))] = dict(sgpr=g("TotalSGPRs"), vgpr=g("VGPRs"), agpr=g("AGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"),
                                                          lds_static=g(r"LDS Size \[bytes/block\]"), waves_per_simd=g(r"Occupancy \[waves/SIMD\]"))
    return out


def main():
    res = resources()
    rec = dict(what="k_chain_mlp_bw<WMAX, SRC> per register width and source form: hipcc -O3 --offload-arch=gfx950 resource remarks",
               box="compiled without a GPU (resource remarks of the gfx950 code object)", lds_budget_bytes=LDS_BUDGET_BYTES, srcs={})
    for s in SRC:
        rec["srcs"][s] = {str(w): res[s][w] for w in WMAX}
    path = os.path.join(ROOT, "profiles", "chain_bw_narrow_resources.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    for s in SRC:
        for k, v in rec["srcs"][s].items():
            print(s, k, (v["sgpr"], v["vgpr"], v["lds_static"], v["scratch"], v["waves_per_simd"]))
    print("wrote", path)


if __name__ == "__main__":
    sys.exit(main())
