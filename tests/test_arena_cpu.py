"""The arena checker of tests/arena.py on CPU tensors: the proof that tests/test_gpu_memory_contract.py can fail.  Every situation the checker
exists for is produced by writing the byte directly — no GPU and no broken kernel — and must be reported, with the carve, the side and the
offsets named; a call that stays inside its output and workspace carves must not be."""
import os
import re

import numpy as np
import pytest
import torch

from tests import arena as AR


def _arena(ws_fill=0x00):
    a = AR.Arena("cpu")
    a.input("x", np.arange(35, dtype=np.float32).reshape(1, 7, 5))  # 140 bytes: not a multiple of 16
    a.output("y", (1, 7, 3), torch.float32)                         # 84 bytes
    a.workspace("ws", 1000)
    a.input("empty", np.zeros((1, 0, 4), dtype=np.float32))         # (de, 0) edge features: an address, no bytes
    a.output("z", (3, 5), torch.bfloat16)                           # 30 bytes
    return a.build(ws_fill=ws_fill)


def _write_all_outputs(a):
    a.view("y")[:] = 1.0
    a.view("z")[:] = 2.0


def test_layout_is_exact_aligned_and_guarded():
    a = _arena()
    sizes = {"x": 140, "y": 84, "ws": 1000, "empty": 0, "z": 30}
    prev_end = 0
    for c in a.carves:
        assert c.nbytes == sizes[c.name]
        assert c.off % AR.ALIGN == 0 and a.ptr(c.name) % AR.ALIGN == 0
        assert c.off - prev_end >= AR.GUARD == 64 * 1024
        prev_end = c.off + c.nbytes
    assert a.buf.numel() - prev_end == AR.GUARD
    assert a.ptr(None) is None
    assert np.array_equal(a.numpy("x"), np.arange(35, dtype=np.float32).reshape(1, 7, 5))
    assert bool((a.raw("ws") == 0).all()) and bool(torch.isnan(a.view("y")).all()) and bool(torch.isnan(a.view("z").float()).all())
    b = _arena(ws_fill=0xFF)
    assert bool((b.raw("ws") == 0xFF).all())
    # everything that is not a carve is sentinel
    mask = torch.ones_like(a.buf, dtype=torch.bool)
    for c in a.carves:
        mask[c.off:c.off + c.nbytes] = False
    assert bool((a.buf[mask] == AR.SENTINEL).all())


def test_a_call_inside_its_carves_passes():
    a = _arena()
    _write_all_outputs(a)
    a.raw("ws")[:] = 7           # a workspace may hold anything afterwards, every byte of it
    assert a.violations() == []
    a.check("in bounds")
    # refill(): the state before the next call; the inputs are untouched by it
    a.refill(0xFF)
    assert bool((a.raw("ws") == 0xFF).all()) and bool(torch.isnan(a.view("y")).all())
    assert np.array_equal(a.numpy("x"), np.arange(35, dtype=np.float32).reshape(1, 7, 5))


@pytest.mark.parametrize("carve", ["y", "ws", "x", "z"])
def test_a_byte_just_before_a_carve_is_reported(carve):
    a = _arena()
    _write_all_outputs(a)
    a.buf[a.by_name[carve].off - 1] = 0
    found = a.violations()
    assert len(found) == 1 and "BEFORE" in found[0] and f"'{carve}'" in found[0] and "first at -1 and last at -1" in found[0], found
    with pytest.raises(AssertionError, match="BEFORE"):
        a.check()


@pytest.mark.parametrize("carve", ["y", "ws", "x", "z", "empty"])
def test_a_byte_just_after_a_carve_is_reported(carve):
    a = _arena()
    _write_all_outputs(a)
    c = a.by_name[carve]
    a.buf[c.off + c.nbytes] = 0           # e.g. the 4th lane of a float4 store behind a 3-wide last row
    a.buf[c.off + c.nbytes + 11] = 0
    found = a.violations()
    assert len(found) == 1 and "AFTER" in found[0] and f"'{carve}'" in found[0] and "2 bytes, first at +0 and last at +11" in found[0], found
    with pytest.raises(AssertionError, match=f"AFTER .*'{carve}'"):
        a.check()


def test_a_byte_in_the_middle_of_a_gap_is_reported():
    a = _arena()
    _write_all_outputs(a)
    y, ws = a.by_name["y"], a.by_name["ws"]
    mid = (y.off + y.nbytes + ws.off) // 2
    a.buf[mid] = 1
    found = a.violations()
    assert len(found) == 1 and ("'y'" in found[0] or "'ws'" in found[0]) and f"arena offsets {mid}..{mid}" in found[0], found
    # the very first and the very last byte of the arena are looked at too
    b = _arena()
    _write_all_outputs(b)
    b.buf[0] = 0
    b.buf[-1] = 0
    found = b.violations()
    assert len(found) == 2 and "BEFORE input 'x'" in found[0] and "AFTER output 'z'" in found[1], found


def test_a_whole_stray_row_is_attributed_to_its_carve():
    a = _arena()
    _write_all_outputs(a)
    y = a.by_name["y"]
    a.buf[y.off + y.nbytes:y.off + y.nbytes + 12] = 0   # an eighth row of three floats
    found = a.violations()
    assert len(found) == 1 and "AFTER output 'y' (84 bytes): 12 bytes, first at +0 and last at +11" in found[0], found


def test_a_changed_input_is_reported():
    a = _arena()
    _write_all_outputs(a)
    a.view("x")[0, 6, 4] = -1.0
    found = a.violations()
    assert len(found) == 1 and "input 'x' was modified" in found[0] and "2 bytes, first at +138 and last at +139" in found[0], found
    with pytest.raises(AssertionError, match="input 'x' was modified"):
        a.check()


def test_an_input_rewritten_with_the_same_bytes_is_not_reported():
    a = _arena()
    _write_all_outputs(a)
    a.view("x")[:] = torch.arange(35, dtype=torch.float32).view(1, 7, 5)
    assert a.violations() == []


def test_an_output_left_unwritten_is_reported():
    a = _arena()
    a.view("z")[:] = 2.0
    y = a.view("y")
    y[:] = 1.0
    y[0, 6, 2] = float("nan")                             # a NaN the call wrote has other bits than the 0xFF fill ...
    assert a.violations() == []
    a.raw("y")[-4:] = AR.UNWRITTEN                        # ... an element it never wrote still holds them
    found = a.violations()
    assert len(found) == 1 and "output 'y'" in found[0] and "1 of 21 elements never written, first element 20, last 20" in found[0], found
    with pytest.raises(AssertionError, match="never written"):
        a.check()
    assert a.violations(unwritten=False) == []
    # bf16 elements are two bytes wide
    b = _arena()
    b.view("y")[:] = 1.0
    b.view("z")[:2] = 2.0
    found = b.violations()
    assert len(found) == 1 and "output 'z'" in found[0] and "5 of 15 elements never written, first element 10, last 14" in found[0], found


def test_several_findings_are_all_listed():
    a = _arena()
    _write_all_outputs(a)
    a.buf[a.by_name["ws"].off - 3] = 0
    a.view("x")[0, 0, 0] = 9.0
    a.raw("z")[:2] = AR.UNWRITTEN
    found = a.violations()
    assert len(found) == 3, found
    with pytest.raises(AssertionError) as e:
        a.check("case")
    assert str(e.value).startswith("case: ") and "BEFORE workspace 'ws'" in str(e.value) and "'x' was modified" in str(e.value)


def test_output_bits_compare_two_runs():
    a, b = _arena(0x00), _arena(0xFF)
    for t in (a, b):
        _write_all_outputs(t)
    assert all(torch.equal(a.output_bits()[k], b.output_bits()[k]) for k in ("y", "z"))
    b.view("y")[0, 0, 0] = 1.0000001
    assert not torch.equal(a.output_bits()["y"], b.output_bits()["y"])


def test_a_workspace_sized_by_a_query_that_needs_addresses():
    a = AR.Arena("cpu")
    w = np.arange(12, dtype=np.float32)
    a.input("w", w)
    seen = []

    def query():  # stands for gnx_*_workspace_bytes(h, &params, R) with params pointing into the arena
        seen.append(a.ptr("w"))
        assert np.array_equal(a.numpy("w"), w)
        return 777
    a.workspace("ws", query)
    a.output("y", (5,), torch.float32)
    a.build(ws_fill=0xFF)
    assert len(seen) == 1 and a.nbytes("ws") == 777 and bool((a.raw("ws") == 0xFF).all())
    assert np.array_equal(a.numpy("w"), w) and a.by_name["y"].off - (a.by_name["ws"].off + 777) >= AR.GUARD
    a.view("y")[:] = 0.0
    assert a.violations() == []
    a.buf[a.by_name["ws"].off + 777] = 0
    assert "AFTER workspace 'ws' (777 bytes)" in a.violations()[0]


# ---------------------------------------------------------------------------------------------------------------------------------------
# skewed carves: the same buffers at 256 k + 4 / + 8 / + 12 (+ 2 for a bf16 carve), tests/test_gpu_alignment.py
# ---------------------------------------------------------------------------------------------------------------------------------------
SKEWS = {"x": 4, "y": 8, "ws": 0, "empty": 12, "z": 2}


def _skewed(ws_fill=0x00):
    a = AR.Arena("cpu", skew=lambda c: SKEWS[c.name])
    a.input("x", np.arange(35, dtype=np.float32).reshape(1, 7, 5))
    a.output("y", (1, 7, 3), torch.float32)
    a.workspace("ws", 1000)
    a.input("empty", np.zeros((1, 0, 4), dtype=np.float32))
    a.output("z", (3, 5), torch.bfloat16)
    return a.build(ws_fill=ws_fill)


def test_a_skewed_layout_is_exact_skewed_and_guarded():
    a = _skewed()
    sizes = {"x": 140, "y": 84, "ws": 1000, "empty": 0, "z": 30}
    prev_end = 0
    for c in a.carves:
        assert c.nbytes == sizes[c.name] and a.raw(c.name).numel() == sizes[c.name]
        assert c.off % AR.ALIGN == SKEWS[c.name] and a.ptr(c.name) % AR.ALIGN == SKEWS[c.name]
        assert c.off - prev_end >= AR.GUARD
        prev_end = c.off + c.nbytes
    assert a.buf.numel() - prev_end == AR.GUARD
    assert np.array_equal(a.numpy("x"), np.arange(35, dtype=np.float32).reshape(1, 7, 5))
    assert bool((a.raw("ws") == 0).all()) and bool(torch.isnan(a.view("y")).all()) and bool(torch.isnan(a.view("z").float()).all())
    mask = torch.ones_like(a.buf, dtype=torch.bool)
    for c in a.carves:
        mask[c.off:c.off + c.nbytes] = False
    assert bool((a.buf[mask] == AR.SENTINEL).all())
    _write_all_outputs(a)
    assert a.violations() == []
    # skew=None and a skew of 0 everywhere are the unskewed layout, byte for byte
    b, z = _arena(), AR.Arena("cpu", skew=lambda c: 0)
    z.input("x", np.arange(35, dtype=np.float32).reshape(1, 7, 5)); z.output("y", (1, 7, 3), torch.float32); z.workspace("ws", 1000)
    z.input("empty", np.zeros((1, 0, 4), dtype=np.float32)); z.output("z", (3, 5), torch.bfloat16)
    z.build()
    assert [c.off for c in b.carves] == [c.off for c in z.carves] and torch.equal(b.buf, z.buf)


@pytest.mark.parametrize("bad", [3, 256, -4, 6])
def test_a_skew_outside_the_rule_is_refused(bad):
    """odd, >= ALIGN, negative, or (6 on an fp32 carve) no multiple of the element size"""
    a = AR.Arena("cpu", skew=lambda c: bad)
    a.output("y", (4,), torch.float32)
    with pytest.raises(AssertionError):
        a.build()


@pytest.mark.parametrize("carve", ["x", "y", "z"])
def test_a_byte_just_before_a_skewed_carve_is_reported(carve):
    a = _skewed()
    _write_all_outputs(a)
    a.buf[a.by_name[carve].off - 1] = 0   # (inside the ALIGN-aligned start .. start + skew: still a guard byte)
    found = a.violations()
    assert len(found) == 1 and "BEFORE" in found[0] and f"'{carve}'" in found[0] and "first at -1 and last at -1" in found[0], found
    b = _skewed()
    _write_all_outputs(b)
    c = b.by_name[carve]
    b.buf[c.off - SKEWS[carve]] = 0       # the aligned address a vector store rounded down to would hit
    found = b.violations()
    assert len(found) == 1 and f"BEFORE {c.kind} '{carve}'" in found[0] and f"first at {-SKEWS[carve]:+d}" in found[0], found


@pytest.mark.parametrize("carve", ["x", "y", "z", "empty"])
def test_a_byte_just_after_a_skewed_carve_is_reported(carve):
    a = _skewed()
    _write_all_outputs(a)
    c = a.by_name[carve]
    a.buf[c.off + c.nbytes] = 0
    a.buf[c.off + c.nbytes + 11] = 0
    found = a.violations()
    assert len(found) == 1 and "AFTER" in found[0] and f"'{carve}'" in found[0] and "2 bytes, first at +0 and last at +11" in found[0], found


def test_a_late_workspace_in_a_skewed_arena_is_laid_out_twice():
    sk = {"w": 12, "ws": 0, "y": 4, "h": 2}
    a = AR.Arena("cpu", skew=lambda c: sk[c.name])
    w = np.arange(12, dtype=np.float32)
    a.input("w", w)
    seen = []

    def query():
        seen.append(a.ptr("w"))
        assert a.ptr("w") % AR.ALIGN == 12 and np.array_equal(a.numpy("w"), w)
        return 777
    a.workspace("ws", query)
    a.output("y", (5,), torch.float32)
    a.input("h", torch.arange(7, dtype=torch.float32).to(torch.bfloat16))
    a.build(ws_fill=0xFF)
    assert len(seen) == 1 and a.nbytes("ws") == 777 and bool((a.raw("ws") == 0xFF).all())
    for n, k in sk.items():
        assert a.ptr(n) % AR.ALIGN == k, n
    assert np.array_equal(a.numpy("w"), w) and np.array_equal(a.numpy("h"), np.arange(7, dtype=np.float32))
    assert a.by_name["y"].off - (a.by_name["ws"].off + 777) >= AR.GUARD
    a.view("y")[:] = 0.0
    assert a.violations() == []
    a.buf[a.by_name["y"].off - 1] = 0
    assert "BEFORE output 'y'" in a.violations()[0]


# ---------------------------------------------------------------------------------------------------------------------------------------
# completeness of tests/test_gpu_alignment.py: every host-side pointer-alignment test of csrc/
# ---------------------------------------------------------------------------------------------------------------------------------------
ALIGNMENT_TEST = re.compile(r"\bal16\(|(?:\(uintptr_t\)|\(al\b)[^;{}]*?&\s*(?:15|7|3)\b")  # (`al`: the OR of a predicate's pointers, *_applies)

# file -> number of source lines holding a pointer-alignment test.  Each of them picks a kernel form (or refuses a call) by the address of a
# caller's buffer; tests/test_gpu_alignment.py runs both sides of them.
ALIGNMENT_SITES = {
    "gnx_backward.hip": 2,       # launch_delta's `al`; the core backward's al16 (its entry points' checks: gnx_staging.h)
    "gnx_backward_wide.hip": 2,  # k_dw_gemm's and the segmented sums' v4
    "gnx_chain.cpp": 1,          # workspace
    "gnx_dropout.hip": 2,        # the quad / scalar mask kernel; workspace
    "gnx_edge_n.hip": 1,
    "gnx_edge_x6.hip": 10,       # proj_x6_applies, node_x6_applies and the launchers' refusals
    "gnx_ffn_fused.hip": 2,      # ffn_fused_applies; the LayerNorm-on-load refusal
    "gnx_ffn_x6.hip": 5,         # ffn_x6_applies and the launchers' refusals
    "gnx_forward.hip": 2,        # the typed loop's bf16 check of every step; the core's wide_ln decision (the other entry checks: gnx_staging.h)
    "gnx_staging.h": 2,          # check_ws and check_bf16_aligned: the workspace / bf16 checks of every entry point of gnx_forward.hip and gnx_backward.hip
    "gnx_generic.hip": 3,        # ln_stats_applies, launch_ln_stats, launch_layernorm2's al16
    "gnx_wide.hip": 17,          # al16 itself, out_vec, launch_gemm's g.vec and refusals, wide_plan
}


def alignment_sites():
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphnets.jl_amd", "csrc")
    out = {}
    for f in sorted(os.listdir(src)):
        if f.endswith((".hip", ".cpp", ".h")):
            n = sum(1 for line in open(os.path.join(src, f), encoding="utf-8") if ALIGNMENT_TEST.search(line))
            if n:
                out[f] = n
    return out


def test_every_pointer_alignment_branch_is_counted():
    found = alignment_sites()
    assert found == ALIGNMENT_SITES, (
        "the pointer-alignment tests of csrc/ changed: " +
        ", ".join(f"{f}: {ALIGNMENT_SITES.get(f, 0)} -> {found.get(f, 0)}" for f in sorted(set(found) | set(ALIGNMENT_SITES)) if found.get(f) != ALIGNMENT_SITES.get(f)) +
        ".  A new alignment branch needs a one(...) group or an anchor case in tests/test_gpu_alignment.py that takes both of its sides BEFORE "
        "the count here is updated.")


def test_relayout_moves_the_carves_and_keeps_their_bytes():
    a = AR.Arena("cpu")
    w = np.arange(12, dtype=np.float32)
    a.input("w", w)
    calls = []
    a.workspace("ws", lambda: calls.append(a.ptr("w") % AR.ALIGN) or 777)
    a.output("y", (5,), torch.float32)
    a.build(ws_fill=0xFF)
    a.view("y")[:] = 3.0
    a.relayout(lambda c: {"w": 8, "ws": 0, "y": 12}[c.name], ws_fill=0x11)
    assert calls == [0, 8] and a.nbytes("ws") == 777 and bool((a.raw("ws") == 0x11).all())
    assert a.ptr("w") % AR.ALIGN == 8 and a.ptr("y") % AR.ALIGN == 12 and a.ptr("ws") % AR.ALIGN == 0
    assert np.array_equal(a.numpy("w"), w) and bool(torch.isnan(a.view("y")).all())
    found = a.violations()
    assert len(found) == 1 and "5 of 5 elements never written" in found[0], found
    a.relayout(None)
    b = AR.Arena("cpu")
    b.input("w", w); b.workspace("ws", 777); b.output("y", (5,), torch.float32)
    b.build()
    assert [c.off for c in a.carves] == [c.off for c in b.carves] and torch.equal(a.buf, b.buf)


def test_relayout_fills_the_inputs_from_their_declared_bytes():
    """an input a call corrupted under one layout is reported there; the next layout of the same arena starts from the declared bytes again"""
    a = AR.Arena("cpu")
    w = np.arange(12, dtype=np.float32)
    a.input("w", w)
    a.workspace("ws", lambda: 64)
    a.output("y", (5,), torch.float32)
    a.build()
    a.view("w")[3] = -1.0
    a.view("y")[:] = 0.0
    assert any("input 'w' was modified" in f for f in a.violations())
    a.relayout(lambda c: 0 if c.kind == AR.WORKSPACE else 4)
    assert np.array_equal(a.numpy("w"), w) and a.ptr("w") % AR.ALIGN == 4
    a.view("y")[:] = 0.0
    assert a.violations() == []
