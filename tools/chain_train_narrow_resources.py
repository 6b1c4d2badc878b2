"""Register / LDS / scratch use of the two fused Chain TRAINING kernels (k_chain_mlp_train<WMAX, SRC>: csrc/gnx_chain_train_narrow.hip, and
k_chain_mlp_bw_train<WMAX, SRC>: csrc/gnx_chain_bw_train_narrow.hip; WMAX = 8, 16, 32 and the three source forms — 18 instantiations), read from
hipcc's resource remarks — no GPU needed.  The twin of tools/chain_narrow_resources.py and tools/chain_bw_narrow_resources.py, whose kernels
are the same layer code without the Dropout op: both files are compiled for gfx950 with the options build.py gives them; the kernels' LDS is
dynamic, so the static figure must be 0; no instantiation may use scratch (include/gnx.h: a class that does is cut from the training rule).
The record carries the test-mode twins' VGPRs (profiles/chain_narrow_resources.json, profiles/chain_bw_narrow_resources.json) next to each.

    python tools/chain_train_narrow_resources.py            # writes profiles/chain_train_narrow_resources.json
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
KERNELS = {"forward": ("gnx_chain_train_narrow.hip", "k_chain_mlp_train", "chain_narrow_resources.json"),
           "backward": ("gnx_chain_bw_train_narrow.hip", "k_chain_mlp_bw_train", "chain_bw_narrow_resources.json")}
WMAX = (8, 16, 32)
SRC = ("edge", "node", "rows")


def _file_flags(name):
    """the per-file options of graphnets.jl_amd/build.py for `name` (the package directory's name has a dot: loaded by path)"""
    spec = importlib.util.spec_from_file_location("_gnx_build", os.path.join(ROOT, "graphnets.jl_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.FILE_FLAGS.get(name, []))


def resources(direction, hipcc=HIPCC):
    """{src: {WMAX: {sgpr, vgpr, agpr, scratch, lds_static, waves_per_simd}}} for every instantiation of the direction's kernel"""
    name, kernel, _ = KERNELS[direction]
    cmd = [hipcc, "-x", "hip", "-c", "--cuda-device-only", "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, os.path.join(CSRC, name)] + _file_flags(name)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {s: {} for s in SRC}
    for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        m = re.match(r"_ZN3gnx\d+" + kernel + r"ILi(\d+)ELi(\d+)EEEv", blk.split()[0])
        if not m:
            continue
        g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))
        out[SRC[int(m.group(2))]][int(m.group(1))] = dict(sgpr=g("TotalSGPRs"), vgpr=g("VGPRs"), agpr=g("AGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"),
                                                          lds_static=g(r"LDS Size \[bytes/block\]"), waves_per_simd=g(r"Occupancy \[waves/SIMD\]"))
    return out


def main():
    rec = dict(what="k_chain_mlp_train / k_chain_mlp_bw_train <WMAX, SRC> per register width and source form: hipcc -O3 --offload-arch=gfx950 resource remarks",
               box="compiled without a GPU (resource remarks of the gfx950 code object)", kernels={})
    with_scratch = []
    for direction, (name, kernel, twin) in KERNELS.items():
        res = resources(direction)
        with open(os.path.join(ROOT, "profiles", twin)) as f:
            test_mode = json.load(f)["srcs"]
        rec["kernels"][direction] = dict(file=name, kernel=kernel, file_flags=_file_flags(name), srcs={s: {str(w): res[s][w] for w in WMAX} for s in SRC},
                                         test_mode_vgpr={s: {str(w): test_mode[s][str(w)]["vgpr"] for w in WMAX} for s in SRC})
        with_scratch += [f"{direction}/{s}/{w}" for s in SRC for w in WMAX if res[s][w]["scratch"] or res[s][w]["lds_static"]]
    rec["instantiations_with_scratch_or_static_lds"] = with_scratch
    rec["note"] = "no instantiation uses scratch or static LDS: no class is cut from the training rule for its resources" if not with_scratch else \
                  "these instantiations use scratch or static LDS: " + ", ".join(with_scratch)
    path = os.path.join(ROOT, "profiles", "chain_train_narrow_resources.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    for direction in KERNELS:
        for s in SRC:
            for k, v in rec["kernels"][direction]["srcs"][s].items():
                print(direction, s, k, (v["sgpr"], v["vgpr"], v["lds_static"], v["scratch"], v["waves_per_simd"]))
    print("wrote", path)


if __name__ == "__main__":
    sys.exit(main())
