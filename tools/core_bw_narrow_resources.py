"""Register / LDS / scratch use of the fused FeedForward pullback of the narrow GNCore backward (k_core_bw_narrow<D>, D = 1..16:
csrc/gnx_core_bw_narrow.hip), read from hipcc's resource remarks — no GPU needed.  The file is compiled for gfx950 with the options build.py
gives it.

    python tools/core_bw_narrow_resources.py            # writes profiles/core_bw_narrow_resources.json
"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphnets.jl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
WIDTHS = tuple(range(1, 17))


def row_length(d):
    """floats of one parked row: [z ; 1 ; delta1] or [h ; 1 ; g], padded to an odd length"""
    return (5 * d + 1) | 1


def waves(d):
    """waves of a workgroup: four while their LDS slices fit 64 KB, else two"""
    return 4 if 4 * 64 * row_length(d) * 4 <= 65536 else 2


def resources(hipcc=HIPCC):
    """{D: {sgpr, vgpr, agpr, scratch, lds, waves_per_simd}} for every instantiation the file holds"""
    cmd = [hipcc, "-x", "hip", "-c", "--cuda-device-only", "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, os.path.join(CSRC, "gnx_core_bw_narrow.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        m = re.match(r"_ZN3gnx\d+k_core_bw_narrowILi(\d+)EEEv", blk.split()[0])
        if not m:
            continue
        g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))
        out[int(m.group(1))] = dict(sgpr=g("TotalSGPRs"), vgpr=g("VGPRs"), agpr=g("AGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"),
                                    lds=g(r"LDS Size \[bytes/block\]"), waves_per_simd=g(r"Occupancy \[waves/SIMD\]"))
    return out


def main():
    res = resources()
    rec = dict(what="k_core_bw_narrow<D> per width: hipcc -O3 --offload-arch=gfx950 resource remarks", widths={})
    for d in WIDTHS:
        rec["widths"][str(d)] = dict(hidden=4 * d, pairs_fc1=4 * d * (d + 1), pairs_fc2=d * (4 * d + 1), waves_per_workgroup=waves(d),
                                     workgroups_per_cu_by_lds=160 * 1024 // max(res[d]["lds"], 1), **res[d])
    path = os.path.join(ROOT, "profiles", "core_bw_narrow_resources.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    for k, v in rec["widths"].items():
        print(k, (v["sgpr"], v["vgpr"], v["lds"], v["scratch"], v["waves_per_simd"]))
    print("wrote", path)


if __name__ == "__main__":
    sys.exit(main())
