"""Child processes of tests/test_gpu_core_bw_narrow.py.  `generic`: GNX_BW_GENERIC is read once per process, so the comparison of
gnx_core_backward_narrow with the generic kernels at widths the matrix cores would take needs a process of its own.  `width_one`: a core at
(1,1,1) specialises the block's forward kernel at run time once per process, which another module of the suite counts in its own process.
`python -m tests.core_bw_narrow_child MODE` prints one JSON line; the first mismatch ends it with a non-zero status and the name of the
tensor."""
import json
import sys


def width_one():
    import torch
    import graphnets_jl_amd as gn
    from tests import test_gpu_core_bw_narrow as T
    torch.cuda.set_device(0)
    applies, fused = [], True
    for act in ("relu", "identity"):
        c = T.case("tiny", 1, (1, 1, 1), act)
        applies.append(c.applies())
        seen = {}
        ref, got = c.run(T.CORE), c.run(T.NARROW, profile=seen)
        try:
            assert T.compare(got, ref, c.what) == set(T.DX) | set(T.GRADS)
        except AssertionError as e:
            print(f"MISMATCH {e}")
            return 1
        fused = fused and "bw_delta" in seen and "bw_fw_dense_generic" not in seen
    print(json.dumps(dict(cases=2, applies=applies, fused=fused)))
    return 0


def main():
    import torch
    import graphnets_jl_amd as gn
    from tests import test_gpu_core_bw_narrow as T
    torch.cuda.set_device(0)
    L = gn._lib
    cases, generic = 0, True
    for dims in T.CHILD_DIMS:
        for batch, R in T.CHILD_CASES:
            for bf16 in (False, True):
                c = T.case(batch, R, dims, "relu", bf16=bf16)
                elem = L.ELEM_BF16 if bf16 else L.ELEM_F32
                assert c.applies(elem) == 1, c.what
                seen = {}
                ref = c.run(T.TYPED, elem, profile=seen) if bf16 else c.run(T.CORE, profile=seen)
                generic = generic and "bw_fw_dense_generic" in seen and not {"bw_ff1_recompute", "bw_dx_ff2", "bw_dx_ff1", "k_dw_gemm"} & set(seen)
                try:
                    assert T.compare(c.run(T.NARROW, elem), ref, f"{c.what} bf16={bf16}") == set(T.DX) | set(T.GRADS)
                except AssertionError as e:
                    print(f"MISMATCH {e}")
                    return 1
                cases += 1
    print(json.dumps(dict(cases=cases, generic=generic)))
    return 0


if __name__ == "__main__":
    sys.exit({"generic": main, "width_one": width_one}[sys.argv[1]]())
