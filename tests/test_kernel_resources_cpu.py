"""tools/kernel_resources.py, the one place that compiles a file of csrc for a resource audit: the parser on remarks pasted from a compile, the
compile line (build.py's, read at call time), the cache (one compile per source and process), the committed records profiles/*_resources.json
(rebuilt in memory, they are the files' bytes) and --check on the command line."""
import glob
import json
import os
import shutil
import subprocess
import sys

import pytest

import tools.kernel_resources as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_hipcc = pytest.mark.skipif(not os.path.exists(kr.HIPCC), reason="hipcc not available")
# the remarks of a plain kernel, of one with static LDS and of one that keeps an array in scratch, as hipcc printed them for gfx950 at -O3
# ([FLAG]: the option that asks for the remarks, which the tool alone spells)
REMARKS = """\
k.hip:2:1: remark: Function Name: _Z7k_plainPf [FLAG]
    2 | __global__ void k_plain(float* x) { x[threadIdx.x] += 1.0f; }
      | ^
k.hip:2:1: remark:     TotalSGPRs: 8 [FLAG]
k.hip:2:1: remark:     VGPRs: 2 [FLAG]
k.hip:2:1: remark:     AGPRs: 0 [FLAG]
k.hip:2:1: remark:     ScratchSize [bytes/lane]: 0 [FLAG]
k.hip:2:1: remark:     Dynamic Stack: False [FLAG]
k.hip:2:1: remark:     Occupancy [waves/SIMD]: 8 [FLAG]
k.hip:2:1: remark:     SGPRs Spill: 0 [FLAG]
k.hip:2:1: remark:     VGPRs Spill: 0 [FLAG]
k.hip:2:1: remark:     LDS Size [bytes/block]: 0 [FLAG]
k.hip:3:1: remark: Function Name: _Z5k_ldsPf [FLAG]
    3 | __global__ void k_lds(float* x) {
      | ^
k.hip:3:1: remark:     TotalSGPRs: 8 [FLAG]
k.hip:3:1: remark:     VGPRs: 3 [FLAG]
k.hip:3:1: remark:     AGPRs: 0 [FLAG]
k.hip:3:1: remark:     ScratchSize [bytes/lane]: 0 [FLAG]
k.hip:3:1: remark:     Dynamic Stack: False [FLAG]
k.hip:3:1: remark:     Occupancy [waves/SIMD]: 8 [FLAG]
k.hip:3:1: remark:     SGPRs Spill: 0 [FLAG]
k.hip:3:1: remark:     VGPRs Spill: 0 [FLAG]
k.hip:3:1: remark:     LDS Size [bytes/block]: 1024 [FLAG]
k.hip:9:1: remark: Function Name: _Z9k_scratchPfPKi [FLAG]
    9 | __global__ void k_scratch(float* x, const int* idx) {
      | ^
k.hip:9:1: remark:     TotalSGPRs: 106 [FLAG]
k.hip:9:1: remark:     VGPRs: 11 [FLAG]
k.hip:9:1: remark:     AGPRs: 0 [FLAG]
k.hip:9:1: remark:     ScratchSize [bytes/lane]: 272 [FLAG]
k.hip:9:1: remark:     Dynamic Stack: False [FLAG]
k.hip:9:1: remark:     Occupancy [waves/SIMD]: 7 [FLAG]
k.hip:9:1: remark:     SGPRs Spill: 17 [FLAG]
k.hip:9:1: remark:     VGPRs Spill: 0 [FLAG]
k.hip:9:1: remark:     LDS Size [bytes/block]: 0 [FLAG]
""".replace("[FLAG]", f"[{kr.REMARKS_FLAG}]")


def test_parse_remarks_on_a_literal():
    assert kr.parse_remarks(REMARKS) == {
        "_Z7k_plainPf": dict(sgpr=8, vgpr=2, agpr=0, scratch=0, lds=0, waves_per_simd=8),
        "_Z5k_ldsPf": dict(sgpr=8, vgpr=3, agpr=0, scratch=0, lds=1024, waves_per_simd=8),
        "_Z9k_scratchPfPKi": dict(sgpr=106, vgpr=11, agpr=0, scratch=272, lds=0, waves_per_simd=7)}
    assert kr.parse_remarks("") == {} and kr.parse_remarks("k.hip:2:1: warning: unused variable 'a' [-Wunused-variable]\n1 warning generated.\n") == {}
    for field in ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"):
        cut = "".join(ln for ln in REMARKS.splitlines(True) if not ln.startswith(f"k.hip:3:1: remark:     {field}: "))
        assert len(cut.splitlines()) == len(REMARKS.splitlines()) - 1
        with pytest.raises(ValueError, match="_Z5k_ldsPf"):  # a block with a field missing is not skipped
            kr.parse_remarks(cut)


def test_build_flags_are_build_py_s_at_call_time(monkeypatch):
    b = kr.build_module()
    assert b.__file__ == os.path.join(ROOT, "graphnets.jl_amd", "build.py")
    assert kr.build_flags("gnx_chain_narrow.hip") == b.FLAGS == kr.build_flags()
    assert kr.build_flags("gnx_narrow_bf16.hip") == b.FLAGS + ["-fno-slp-vectorize"]
    assert kr.build_flags(os.path.join(kr.CSRC, "gnx_narrow_bf16.hip"))[-1] == "-fno-slp-vectorize"
    monkeypatch.setattr(b, "FILE_FLAGS", {"gnx_chain_narrow.hip": ["-DX=1"]})
    assert kr.build_flags("gnx_chain_narrow.hip") == b.FLAGS + ["-DX=1"] and kr.build_flags("gnx_narrow_bf16.hip") == b.FLAGS
    monkeypatch.setattr(b, "FLAGS", ["-O1"])
    assert kr.build_flags("gnx_chain_narrow.hip") == ["-O1", "-DX=1"]
    monkeypatch.setenv("GNX_CXXFLAGS", "-DY=2")  # (a diagnostic build's options are not the record's)
    assert kr.build_flags("gnx_chain_narrow.hip") == ["-O1", "-DX=1"]


@needs_hipcc
def test_remarks_compiles_a_source_once(monkeypatch):
    text = '#include <hip/hip_runtime.h>\n__global__ void k_cache_probe(float* x) {\n  __shared__ float s[64];\n  s[threadIdx.x] = x[threadIdx.x];\n' \
           '  __syncthreads();\n  x[threadIdx.x] = s[63 - threadIdx.x];\n}\n'
    calls, run = [], subprocess.run

    def counted(cmd, *a, **k):
        calls.append(cmd)
        return run(cmd, *a, **k)

    monkeypatch.setattr(kr.subprocess, "run", counted)
    first = kr.remarks(text)
    assert kr.remarks(text) is first and len(calls) == 1, calls
    assert list(first) == ["_Z13k_cache_probePf"] and first["_Z13k_cache_probePf"]["lds"] == 256 and first["_Z13k_cache_probePf"]["scratch"] == 0
    cmd = calls[0]
    assert cmd[0] == kr.HIPCC and "--cuda-device-only" in cmd and cmd.count(kr.REMARKS_FLAG) == 1
    assert [c for c in cmd if c in kr.build_flags()] == kr.build_flags()  # build.py's line
    # the per-file options of `like` are part of the line and of the key: another compile
    assert kr.remarks(text, like="gnx_narrow_bf16.hip") == first and len(calls) == 2 and "-fno-slp-vectorize" in calls[1]
    with pytest.raises(RuntimeError, match="k_undeclared"):
        kr.remarks("__global__ void k() { k_undeclared(); }\n")


# (chain_train_narrow's two files are compiled by no test: `python tools/kernel_resources.py chain_train_narrow --check` covers that record)
@needs_hipcc
@pytest.mark.parametrize("family", [f for f in kr.FAMILIES if f != "chain_train_narrow"])
def test_the_committed_record_reproduces(family):
    with open(kr.record_path(family)) as f:
        assert kr.record_text(family) == f.read()


@needs_hipcc
def test_check_on_the_command_line(tmp_path):
    tool = [sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "core_bw_narrow", "--check"]
    r = subprocess.run(tool, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and "up to date" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    records = tmp_path / "profiles"
    records.mkdir()
    for f in glob.glob(os.path.join(ROOT, "profiles", "*_resources.json")):
        shutil.copy(f, records)
    path = records / "core_bw_narrow_resources.json"
    good = path.read_text()
    vgpr = json.loads(good)["widths"]["10"]["vgpr"]
    edited = good.replace(f'"vgpr": {vgpr}', f'"vgpr": {vgpr + 1}', 1)
    assert edited != good
    path.write_text(edited)
    r = subprocess.run(tool + ["--records", str(records)], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]
    assert f'-   "vgpr": {vgpr + 1},' in r.stdout and f'+   "vgpr": {vgpr},' in r.stdout and "@@" in r.stdout, r.stdout[-2000:]
    assert path.read_text() == edited  # --check writes nothing
