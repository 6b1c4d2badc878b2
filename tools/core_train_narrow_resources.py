"""Register / LDS / scratch use of the training-mode FeedForward + Dropout + residual kernel of the narrow GNCore (k_core_post_train<D, BF16>,
D = 1..16, fp32 and bf16 rows: csrc/gnx_core_train_narrow.hip), read from hipcc's resource remarks — no GPU needed.  The file is compiled for
gfx950 with the options build.py gives it.

    python tools/core_train_narrow_resources.py            # writes profiles/core_train_narrow_resources.json
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
ELEMS = ("f32", "bf16")
ROWS_PER_LANE = 2  # core_post_train_rows in the kernel file


def philox_blocks(d):
    """Philox blocks generated per row: a row of d elements starting at element offset 0..omax of a block"""
    omax = 0 if d % 4 == 0 else 2 if d % 2 == 0 else 3
    return (omax + d + 3) // 4


def resources(hipcc=HIPCC):
    """{elem: {D: {sgpr, vgpr, agpr, scratch, lds, waves_per_simd}}} for every instantiation the file holds"""
    cmd = [hipcc, "-x", "hip", "-c", "--cuda-device-only", "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, os.path.join(CSRC, "gnx_core_train_narrow.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {e: {} for e in ELEMS}
    for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        m = re.match(r"_ZN3gnx\d+k_core_post_trainILi(\d+)ELb([01])EEEv", blk.split()[0])
        if not m:
            continue
        g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))
        out[ELEMS[int(m.group(2))]][int(m.group(1))] = dict(sgpr=g("TotalSGPRs"), vgpr=g("VGPRs"), agpr=g("AGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"),
                                                            lds=g(r"LDS Size \[bytes/block\]"), waves_per_simd=g(r"Occupancy \[waves/SIMD\]"))
    return out


def main():
    res = resources()
    rec = dict(what="k_core_post_train<D, BF16> per width and element type: hipcc -O3 --offload-arch=gfx950 resource remarks",
               box="compiled without a GPU (resource remarks of the gfx950 code object)", rows_per_lane=ROWS_PER_LANE, elems={})
    for e in ELEMS:
        rec["elems"][e] = {str(d): dict(hidden=4 * d, philox_blocks_per_row=philox_blocks(d), **res[e][d]) for d in WIDTHS}
    path = os.path.join(ROOT, "profiles", "core_train_narrow_resources.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    for e in ELEMS:
        for k, v in rec["elems"][e].items():
            print(e, k, (v["sgpr"], v["vgpr"], v["lds"], v["scratch"], v["waves_per_simd"]))
    print("wrote", path)


if __name__ == "__main__":
    sys.exit(main())
