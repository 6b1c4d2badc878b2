"""Register / LDS / scratch use of the fused Chain pullback kernel on bfloat16 features (k_chain_mlp_bw_bf16<WMAX, SRC>, WMAX = 8, 16, 32 and the
three source forms: csrc/gnx_chain_bw_narrow_bf16.hip), read from hipcc's resource remarks — no GPU needed.  The twin of
tools/chain_bw_narrow_resources.py, whose fp32 kernel is the same text (csrc/gnx_chain_bw_kernel.h): the file is compiled for gfx950 with the
options build.py gives it, the kernel's LDS is dynamic (the staged parameters, then per wave the row tape and the accumulators, at most
lds_budget_bytes), so the static figure must be 0.  The record also says, per instantiation, whether it keeps the fp32 kernel's waves per SIMD
(the 32-wide fp32 kernel takes 235 VGPRs at 2 waves per SIMD; beyond 256 a kernel loses the second wave).

    python tools/chain_bw_narrow_bf16_resources.py            # writes profiles/chain_bw_narrow_bf16_resources.json
"""
import importlib.util
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphnets.jl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FILE = "gnx_chain_bw_narrow_bf16.hip"
WMAX = (8, 16, 32)
SRC = ("edge", "node", "rows")
LDS_BUDGET_BYTES = 4 * 16384  # kChainBwLdsFloats (gnx_chain_plan.h)


def _file_flags():
    """the per-file options of graphnets.jl_amd/build.py for FILE (the package directory's name has a dot: loaded by path)"""
    spec = importlib.util.spec_from_file_location("_gnx_build", os.path.join(ROOT, "graphnets.jl_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.FILE_FLAGS.get(FILE, []))


def resources(hipcc=HIPCC):
    """{src: {WMAX: {sgpr, vgpr, agpr, scratch, lds_static, waves_per_simd}}} for every instantiation the file holds"""
    cmd = [hipcc, "-x", "hip", "-c", "--cuda-device-only", "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, os.path.join(CSRC, FILE)] + _file_flags()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {s: {} for s in SRC}
    for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        m = re.match(r"_ZN3gnx\d+k_chain_mlp_bw_bf16ILi(\d+)ELi(\d+)EEEv", blk.split()[0])
        if not m:
            continue
        g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))
        out[SRC[int(m.group(2))]][int(m.group(1))] = dict(sgpr=g("TotalSGPRs"), vgpr=g("VGPRs"), agpr=g("AGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"),
                                                          lds_static=g(r"LDS Size \[bytes/block\]"), waves_per_simd=g(r"Occupancy \[waves/SIMD\]"))
    return out


def main():
    res = resources()
    with open(os.path.join(ROOT, "profiles", "chain_bw_narrow_resources.json")) as f:
        fp32 = json.load(f)["srcs"]
    rec = dict(what="k_chain_mlp_bw_bf16<WMAX, SRC> per register width and source form: hipcc -O3 --offload-arch=gfx950 resource remarks",
               box="compiled without a GPU (resource remarks of the gfx950 code object)", file_flags=_file_flags(), lds_budget_bytes=LDS_BUDGET_BYTES, srcs={})
    lost = []
    for s in SRC:
        rec["srcs"][s] = {str(w): res[s][w] for w in WMAX}
        lost += [f"{s}/{w}" for w in WMAX if res[s][w]["waves_per_simd"] < fp32[s][str(w)]["waves_per_simd"]]
    rec["fp32_vgpr"] = {s: {str(w): fp32[s][str(w)]["vgpr"] for w in WMAX} for s in SRC}
    rec["instantiations_with_fewer_waves_per_simd_than_fp32"] = lost
    rec["note"] = ("no instantiation goes over 256 VGPRs: each keeps the waves per SIMD of its fp32 twin (profiles/chain_bw_narrow_resources.json)" if not lost else
                   "these instantiations lose a wave per SIMD against their fp32 twins: " + ", ".join(lost))
    path = os.path.join(ROOT, "profiles", "chain_bw_narrow_bf16_resources.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    for s in SRC:
        for k, v in rec["srcs"][s].items():
            print(s, k, (v["sgpr"], v["vgpr"], v["lds_static"], v["scratch"], v["waves_per_simd"]))
    print("wrote", path)


if __name__ == "__main__":
    sys.exit(main())
