"""Register / LDS / scratch use of the fused kernels, read from hipcc's resource remarks — no GPU needed.  The one place that compiles a file of
graphnets.jl_amd/csrc for a resource audit (with the line build.py gives that file) and parses the remarks; the tests and the timing tools read
remarks(), the committed records profiles/*_resources.json are written from the table of families below.

    python tools/kernel_resources.py FAMILY... | --all      # writes profiles/FAMILY_resources.json
    python tools/kernel_resources.py --all --check          # writes nothing: prints a diff of every record that would change, exits 1 if any
"""
import argparse
import concurrent.futures
import difflib
import functools
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphnets.jl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = dict(sgpr="TotalSGPRs", vgpr="VGPRs", agpr="AGPRs", scratch=r"ScratchSize \[bytes/lane\]", lds=r"LDS Size \[bytes/block\]",
              waves_per_simd=r"Occupancy \[waves/SIMD\]")
REMARKS_FLAG = "-Rpass-analysis=kernel-resource-usage"
_cache = {}


@functools.lru_cache(None)
def build_module():
    """graphnets.jl_amd/build.py (the package directory's name has a dot: loaded by path, once)"""
    spec = importlib.util.spec_from_file_location("_gnx_build", os.path.join(ROOT, "graphnets.jl_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def file_flags(file):
    """the per-file options of build.py for `file` of csrc"""
    return list(build_module().FILE_FLAGS.get(os.path.basename(file), [])) if file else []


def build_flags(file=None):
    """the options build.py compiles `file` of csrc with, read at call time (GNX_CXXFLAGS is left out: the records describe the default build)"""
    return list(build_module().FLAGS) + file_flags(file)


def parse_remarks(stderr):
    """{mangled name: {sgpr, vgpr, agpr, scratch, lds, waves_per_simd}} of every kernel in the remarks of REMARKS_FLAG"""
    out = {}
    for blk in re.split(r"remark: Function Name: ", stderr)[1:]:
        name, found = blk.split()[0], {k: re.search(label + r": (\d+)", blk) for k, label in FIELDS.items()}
        if not all(found.values()):
            raise ValueError(f"the remarks of {name} lack {[k for k, m in found.items() if not m]}")
        out[name] = {k: int(m.group(1)) for k, m in found.items()}
    return out


def demangle(name):
    """c++filt's reading of a mangled kernel name (the name itself where c++filt gives none)"""
    return subprocess.run(["c++filt", name], stdout=subprocess.PIPE, text=True).stdout.strip() or name


def remarks(source, like=None):
    """parse_remarks of one device-only compile for gfx950.  source: a file of csrc, or program text, which gets the per-file options of the
    csrc file `like`.  Cached in the process by source and options: a pytest session compiles each file once."""
    is_file = "\n" not in source and os.path.exists(os.path.join(CSRC, source))
    flags = build_flags(source if is_file else like)
    key = (source, tuple(flags))
    if key not in _cache:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(CSRC, source) if is_file else os.path.join(tmp, "kernel_resources.hip")
            if not is_file:
                with open(path, "w") as f:
                    f.write(source)
            cmd = [HIPCC, "-x", "hip", "-c", "--cuda-device-only"] + flags + [REMARKS_FLAG, "-o", os.devnull, path]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=1800)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {path}:\n" + r.stderr[-3000:])
        _cache[key] = parse_remarks(r.stderr)
    return _cache[key]


def remarks_many(sources, jobs=8):
    """remarks() of several sources (a file name, or (text, like)), at most `jobs` compilers at once; the results are then in the cache"""
    sources = list(dict.fromkeys(sources))
    build_module()
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        return list(ex.map(lambda s: remarks(*s) if isinstance(s, tuple) else remarks(s), sources))


# ---- the families: one entry per record.  file / text + like: what is compiled; name: the kernel's mangled name; key: the match's place in
# resources(); fields: record key -> parsed key; record: builds the record from resources() (and the twin records it cites) ----
WMAX = (8, 16, 32)  # the register widths of the Chain kernels
SRC = ("edge", "node", "rows")  # their source forms, in the order of the SRC template argument
ALL = {k: k for k in FIELDS}
NO_AGPR = {k: k for k in FIELDS if k != "agpr"}
STATIC = {("lds_static" if k == "lds" else k): k for k in FIELDS}  # a kernel whose LDS is dynamic: the static figure, which must be 0
BOX = "compiled without a GPU (resource remarks of the gfx950 code object)"
REMARKS = ": hipcc -O3 --offload-arch=gfx950 resource remarks"


def static_lds(de, dn, dg, oe):
    ke = de + 2 * dn + dg
    ps = (oe * (ke + 1) + 63) // 64
    return 4 * 4 * (64 * ((oe + ke) | 1) + 64 * ps)


def eligible(de, dn, dg, oe):
    """the rule of jit_bw_edge_eligible (csrc/gnx_jit.cpp) with run-time specialisation enabled and no LDS padding"""
    ke = de + 2 * dn + dg
    if min(de, dn, dg) < 0 or oe < 1 or ke < 1 or oe * ke >= 64:
        return False
    return static_lds(de, dn, dg, oe) <= 64 * 1024


def row_length(d):
    """floats of one parked row of k_core_bw_narrow: [z ; 1 ; delta1] or [h ; 1 ; g], padded to an odd length"""
    return (5 * d + 1) | 1


def waves(d):
    """waves of a k_core_bw_narrow workgroup: four while their LDS slices fit 64 KB, else two"""
    return 4 if 4 * 64 * row_length(d) * 4 <= 65536 else 2


def philox_blocks(d):
    """Philox blocks k_core_post_train generates per row: a row of d elements starting at element offset 0..omax of a block"""
    omax = 0 if d % 4 == 0 else 2 if d % 2 == 0 else 3
    return (omax + d + 3) // 4


def _bw_narrow_text(sets):
    """explicit instantiations of the kernel header for the listed sets (the run-time specialiser of gnx_jit.cpp compiles the same text)"""
    for s in sets:
        assert eligible(*s), f"{s} is not an eligible width set"
    inst = [f"template __global__ void k_bw_edge_wave{b}<{de}, {dn}, {dg}, {oe}>(BwEdgeWave);" for de, dn, dg, oe in sets for b in ("", "_bf16")]
    return "\n".join(['#include "gnx_bw_edge_wave_kernel.h"', "namespace gnx {"] + inst + ["}"]) + "\n"


def _rec_bw_narrow(f, res, twin):
    rec, r = dict(what="k_bw_edge_wave / k_bw_edge_wave_bf16 per (de, dn, dg, oe)" + REMARKS, sets={}), res()
    for s in f["SETS"]:
        de, dn, dg, oe = s
        ke = de + 2 * dn + dg
        rec["sets"][str(s)] = dict(ke=ke, pairs=oe * (ke + 1), pair_slots=(oe * (ke + 1) + 63) // 64, ahead_of_time=s in f["AOT_SETS"], **r[str(s)])
    return rec


def _rec_core_bw_narrow(f, res, twin):
    r = res()
    return dict(what="k_core_bw_narrow<D> per width" + REMARKS, widths={
        str(d): dict(hidden=4 * d, pairs_fc1=4 * d * (d + 1), pairs_fc2=d * (4 * d + 1), waves_per_workgroup=waves(d),
                     workgroups_per_cu_by_lds=160 * 1024 // max(r[d]["lds"], 1), **r[d]) for d in f["WIDTHS"]})


def _rec_core_train_narrow(f, res, twin):
    r = res()
    return dict(what="k_core_post_train<D, BF16> per width and element type" + REMARKS, box=BOX, rows_per_lane=f["ROWS_PER_LANE"], elems={
        e: {str(d): dict(hidden=4 * d, philox_blocks_per_row=philox_blocks(d), **r[e][d]) for d in f["WIDTHS"]} for e in f["ELEMS"]})


def _srcs(r):
    return {s: {str(w): r[s][w] for w in WMAX} for s in SRC}


def _rec_chain(f, res, twin):
    rec = dict(what=f["kernel"] + "<WMAX, SRC> per register width and source form" + REMARKS, box=BOX)
    if f["file"].endswith("_bf16.hip"):  # the bf16 records say which per-file options the compile had
        rec["file_flags"] = file_flags(f["file"])
    rec.update(lds_budget_bytes=f["LDS_BUDGET_BYTES"], srcs=_srcs(res()))
    if "twin" in f:  # does an instantiation lose its fp32 twin's waves per SIMD (beyond 256 VGPRs a kernel loses the second wave)?
        fp32 = twin(f["twin"])["srcs"]
        lost = [f"{s}/{w}" for s in SRC for w in WMAX if rec["srcs"][s][str(w)]["waves_per_simd"] < fp32[s][str(w)]["waves_per_simd"]]
        rec["fp32_vgpr"] = {s: {str(w): fp32[s][str(w)]["vgpr"] for w in WMAX} for s in SRC}
        rec["instantiations_with_fewer_waves_per_simd_than_fp32"] = lost
        rec["note"] = (f"no instantiation goes over 256 VGPRs: each keeps the waves per SIMD of its fp32 twin (profiles/{f['twin']}_resources.json)" if not lost else
                       "these instantiations lose a wave per SIMD against their fp32 twins: " + ", ".join(lost))
    return rec


def _rec_chain_train_narrow(f, res, twin):
    rec = dict(what="k_chain_mlp_train / k_chain_mlp_bw_train <WMAX, SRC> per register width and source form" + REMARKS, box=BOX, kernels={})
    bad = []
    for direction, (file, kernel, test_mode) in f["KERNELS"].items():
        srcs, tm = _srcs(res(direction)), twin(test_mode)["srcs"]
        rec["kernels"][direction] = dict(file=file, kernel=kernel, file_flags=file_flags(file), srcs=srcs,
                                         test_mode_vgpr={s: {str(w): tm[s][str(w)]["vgpr"] for w in WMAX} for s in SRC})
        bad += [f"{direction}/{s}/{w}" for s in SRC for w in WMAX if srcs[s][str(w)]["scratch"] or srcs[s][str(w)]["lds_static"]]
    rec["instantiations_with_scratch_or_static_lds"] = bad
    rec["note"] = "no instantiation uses scratch or static LDS: no class is cut from the training rule for its resources" if not bad else \
                  "these instantiations use scratch or static LDS: " + ", ".join(bad)
    return rec


def _chain(kernel, file, lds_budget, **more):
    """a Chain kernel k<WMAX, SRC> of one file: resources() is {src: {WMAX: {...}}}; the LDS is dynamic (at most LDS_BUDGET_BYTES)"""
    return dict(file=file, kernel=kernel, name=r"_ZN3gnx\d+" + kernel + r"ILi(\d+)ELi(\d+)EEEv", key=lambda m: (SRC[int(m.group(2))], int(m.group(1))),
                fields=STATIC, record=_rec_chain, WMAX=WMAX, SRC=SRC, LDS_BUDGET_BYTES=lds_budget, **more)


AOT_SETS = ((10, 5, 0, 3), (3, 4, 5, 3), (0, 2, 0, 2), (2, 2, 2, 2), (4, 3, 2, 3))  # (de, dn, dg, oe): gnx_backward_narrow.hip
FAMILIES = {
    # the fused narrow edge pullback (csrc/gnx_bw_edge_wave_kernel.h), fp32 and bf16, for a list of width sets: the five ahead-of-time sets, the sets
    # tests/test_bw_narrow_abi.py precompiles, and the corners of the eligibility rule (oe * Ke < 64, static LDS <= 64 KB): two pair slots per lane
    # ((6,6,3)=>3: 66 pairs, (2,3,1)=>7: 70, (0,1,0)=>9: 27 ... (1,0,0)=>31: 62 pairs on one slot, (0,0,1)=>62 is refused by the LDS rule), the widest
    # rows ((20,16,10)=>1: Ke = 62).  resources("bw_narrow", sets) takes another list.
    "bw_narrow": dict(
        text=_bw_narrow_text, like="gnx_backward_narrow.hip", name=r"_ZN3gnx\d+k_bw_edge_wave(_bf16)?ILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEEv",
        key=lambda m: (str(tuple(int(v) for v in m.groups()[1:])), "bf16" if m.group(1) else "fp32"), fields=NO_AGPR, record=_rec_bw_narrow, AOT_SETS=AOT_SETS,
        SETS=AOT_SETS + ((3, 2, 4, 3), (2, 3, 1, 7), (6, 6, 3, 3), (5, 5, 5, 3), (20, 10, 4, 1), (20, 16, 10, 1), (1, 0, 0, 1), (0, 1, 0, 9), (0, 0, 1, 5), (1, 0, 0, 31))),
    # the fused FeedForward pullback of the narrow GNCore backward, D = 1..16
    "core_bw_narrow": dict(file="gnx_core_bw_narrow.hip", name=r"_ZN3gnx\d+k_core_bw_narrowILi(\d+)EEEv", key=lambda m: (int(m.group(1)),), fields=ALL,
                           record=_rec_core_bw_narrow, WIDTHS=tuple(range(1, 17))),
    # the training-mode FeedForward + Dropout + residual kernel of the narrow GNCore, D = 1..16, fp32 and bf16 rows
    "core_train_narrow": dict(file="gnx_core_train_narrow.hip", name=r"_ZN3gnx\d+k_core_post_trainILi(\d+)ELb([01])EEEv",
                              key=lambda m: (("f32", "bf16")[int(m.group(2))], int(m.group(1))), fields=ALL, record=_rec_core_train_narrow,
                              WIDTHS=tuple(range(1, 17)), ELEMS=("f32", "bf16"), ROWS_PER_LANE=2),  # (core_post_train_rows in the kernel file)
    # the fused Chain update function: the LDS holds the function's zero-padded parameters (kChainNarrowLdsFloats: gnx_launchers.h)
    "chain_narrow": _chain("k_chain_mlp", "gnx_chain_narrow.hip", 4 * 10240),
    # the fused Chain pullback: the staged parameters, then per wave the row tape and the accumulators (kChainBwLdsFloats: gnx_chain_plan.h)
    "chain_bw_narrow": _chain("k_chain_mlp_bw", "gnx_chain_bw_narrow.hip", 4 * 16384),
    "chain_narrow_bf16": _chain("k_chain_mlp_bf16", "gnx_chain_narrow_bf16.hip", 4 * 10240),
    # the same text as the fp32 pullback (csrc/gnx_chain_bw_kernel.h), whose 32-wide kernel takes 235 VGPRs at 2 waves per SIMD
    "chain_bw_narrow_bf16": _chain("k_chain_mlp_bw_bf16", "gnx_chain_bw_narrow_bf16.hip", 4 * 16384, twin="chain_bw_narrow"),
    # the two Chain training kernels (the layer code of chain_narrow / chain_bw_narrow with the Dropout op), 18 instantiations: none may use scratch
    # (include/gnx.h: a class that does is cut from the training rule); the record carries the test-mode twins' VGPRs next to each.
    # resources("chain_train_narrow", direction)
    "chain_train_narrow": dict(
        KERNELS={"forward": ("gnx_chain_train_narrow.hip", "k_chain_mlp_train", "chain_narrow"),
                 "backward": ("gnx_chain_bw_train_narrow.hip", "k_chain_mlp_bw_train", "chain_bw_narrow")},
        name=r"_ZN3gnx\d+%sILi(\d+)ELi(\d+)EEEv", key=lambda m: (SRC[int(m.group(2))], int(m.group(1))), fields=STATIC, record=_rec_chain_train_narrow,
        WMAX=WMAX, SRC=SRC),
}


def sources(family, arg=None):
    """[(source, like, name)] of the family's compiles.  arg: the width sets of bw_narrow, the direction of chain_train_narrow (None: both)"""
    f = FAMILIES[family]
    if "text" in f:
        return [(f["text"](f["SETS"] if arg is None else arg), f["like"], f["name"])]
    if "KERNELS" in f:
        return [(file, None, f["name"] % kernel) for d, (file, kernel, _) in f["KERNELS"].items() if arg in (None, d)]
    return [(f["file"], None, f["name"])]


def pick(family, parsed, name=None):
    """the kernels of the family among parsed remarks, nested as its `key` says and with the names of its `fields`"""
    f, out = FAMILIES[family], {}
    for mangled, r in parsed.items():
        m = re.match(name or f["name"], mangled)
        if m:
            *path, last = f["key"](m)
            d = out
            for k in path:
                d = d.setdefault(k, {})
            d[last] = {k: r[v] for k, v in f["fields"].items()}
    return out


def resources(family, arg=None):
    """the figures of the family's kernels, e.g. {src: {WMAX: {sgpr, vgpr, agpr, scratch, lds_static, waves_per_simd}}} of a Chain kernel"""
    (source, like, name), = sources(family, arg)
    return pick(family, remarks(source, like), name)


def record_path(family, records=None):
    return os.path.join(records or os.path.join(ROOT, "profiles"), family + "_resources.json")


def record_text(family, records=None, built=None):
    """the text of the family's record; a twin it cites is taken from `built` ({family: record text} of this run), else from its file"""
    f = FAMILIES[family]

    def twin(name):
        if built and name in built:
            return json.loads(built[name])
        with open(record_path(name, records)) as fh:
            return json.load(fh)

    return json.dumps(f["record"](f, lambda arg=None: resources(family, arg), twin), indent=1) + "\n"


def print_table(rec, path=()):
    for k, v in rec.items():
        if not isinstance(v, dict):
            continue
        at = path if k in ("sets", "widths", "elems", "srcs", "kernels") else path + (k,)
        if "pairs" in v:
            print(k, v["pairs"], {e: (v[e]["sgpr"], v[e]["vgpr"], v[e]["lds"], v[e]["scratch"], v[e]["waves_per_simd"]) for e in ("fp32", "bf16")})
        elif "sgpr" in v:
            print(*at, (v["sgpr"], v["vgpr"], v.get("lds", v.get("lds_static")), v["scratch"], v["waves_per_simd"]))
        else:
            print_table(v, at)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("families", nargs="*", metavar="FAMILY", help=", ".join(FAMILIES))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--check", action="store_true", help="write nothing; print a diff of every record that would change and exit 1 if any")
    ap.add_argument("--records", default=None, metavar="DIR", help="the directory of the records (default: profiles/)")
    a = ap.parse_args()
    names = [n for n in FAMILIES if a.all or n in a.families]  # (the table's order has every twin ahead of the record that cites it)
    if not names or set(a.families) - set(FAMILIES):
        ap.error("name families of " + ", ".join(FAMILIES) + ", or --all")
    remarks_many([(s, like) if like else s for n in names for s, like, _ in sources(n)])
    built, changed = {}, 0
    for n in names:
        built[n] = text = record_text(n, a.records, built)
        path = record_path(n, a.records)
        print_table(json.loads(text))
        if a.check:
            with open(path) as f:
                old = f.read()
            diff = "".join(difflib.unified_diff(old.splitlines(True), text.splitlines(True), path, path + " (rebuilt)"))
            print(diff or f"{path} is up to date", end="" if diff else "\n")
            changed += bool(diff)
        else:
            with open(path, "w") as f:
                f.write(text)
            print("wrote", path)
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
