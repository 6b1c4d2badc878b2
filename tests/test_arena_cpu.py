"""The arena checker of tests/arena.py on CPU tensors: the proof that tests/test_gpu_memory_contract.py can fail.  Every situation the checker
exists for is produced by writing the byte directly — no GPU and no broken kernel — and must be reported, with the carve, the side and the
offsets named; a call that stays inside its output and workspace carves must not be."""
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
