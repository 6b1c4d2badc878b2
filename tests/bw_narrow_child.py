"""Child processes of tests/test_gpu_bw_narrow.py: what the library reads from the environment once per process (GNX_JIT_ALL, GNX_JIT,
GNX_JIT_CACHE) needs a process of its own.  `python -m tests.bw_narrow_child MODE` prints one JSON line; any failed call raises."""
import json
import sys


def main(mode):
    import torch
    import graphnets_jl_amd as gn
    from tests import test_gpu_bw_narrow as T
    torch.cuda.set_device(0)
    out = {}
    if mode == "jit_all":  # the five listed sets through the new entry run the run-time kernel: the bits of the ahead-of-time build
        differing, cases = [], 0
        for prm in T.AOT_SETS:
            dims = prm.values[0]
            c = T.CaseN(gn, T.graph(gn, "degrees"), 1, *dims, (1, 2, 3), T._seed("jit_all", dims))
            for bf16 in (False, True):
                before = T.stats(gn)["compiled"]
                assert c.applies_n(bf16) == 1 and c.size(T.NARROW, bf16) == c.size(T.FUSED, bf16), (dims, bf16)
                if T.stats(gn)["compiled"] != before + 1:
                    differing.append([list(dims[0]), bf16, "no run-time kernel was compiled"])
                nine = c.tensors(bf16)
                new, aot = c.go(T.NARROW, bf16, nine), c.go(T.FUSED, bf16, nine, ws_fill=0x3C)
                for name, a, b in zip(T.NAMES, new, aot):
                    assert (a is None) == (b is None), name
                    if a is not None and not torch.equal(T.digest_view(a), T.digest_view(b)):
                        differing.append([list(dims[0]), bf16, name])
                cases += 1
        out = dict(T.stats(gn), cases=cases, differing=differing)
    elif mode == "nojit":  # GNX_JIT=0: the typed call at a run-time set, the fused-typed call at a listed one
        c = T.CaseN(gn, T.graph(gn, "degrees"), 1, *T.S231, (1, 2, 3), 5)
        differing = []
        for bf16 in (False, True):
            nine = c.tensors(bf16)
            for name, a, b in zip(T.NAMES, c.go(T.NARROW, bf16, nine), c.go(T.TYPED, bf16, nine, ws_fill=0x3C)):
                assert (a is None) == (b is None), name
                if a is not None and not torch.equal(T.digest_view(a), T.digest_view(b)):
                    differing.append([bf16, name])
        listed = T.CaseN(gn, T.graph(gn, "degrees"), 1, (10, 5, 0), (3, 4, 5), (1, 2, 3), 5)
        out = dict(applies=[c.applies_n(b) for b in (False, True)], sizes_equal=[c.size(T.NARROW, b) == c.size(T.TYPED, b) for b in (False, True)],
                   listed_applies=[listed.applies_n(b) for b in (False, True)], differing=differing, stats=T.stats(gn))
    elif mode == "cache":  # GNX_JIT_CACHE holds the kernels of this case: loaded, not compiled
        c = T.CaseN(gn, T.graph(gn, "degrees"), 1, (1, 2, 3), (4, 4, 5), (2, 3, 2), 15)
        before = T.stats(gn)["disk_hits"]
        applies = [c.applies_n(b) for b in (False, True)]
        hits = T.stats(gn)["disk_hits"] - before
        out = dict(applies=applies, bw_disk_hits=hits, digests=[T.digest(c.go(T.NARROW, b, c.tensors(b))) for b in (False, True)], stats=T.stats(gn))
    else:
        raise SystemExit(f"unknown mode {mode}")
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1])
