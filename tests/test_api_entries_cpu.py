"""The entry table of the Python binding (graphnets.jl_amd/api.py, `_entry`): which C symbols a call of a GNBlock or GNCore reaches and the
arguments around the family's pointers, for the full product of family x direction x element type x switches x Dropout record, against a table
written out here.  Needs no GPU and no library: the table is plain data, and nothing here may load libgnx.so."""
import itertools
import os
import re

import pytest

import graphnets_jl_amd as gn
from graphnets_jl_amd.api import _entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = gn._lib.ELEM_F32, gn._lib.ELEM_BF16
NIE = "NotImplementedError"
FL, DR = "flags", "drop"

BLOCK_SW = ("bf16_backward", "fused_backward", "narrow_backward")
CHAIN_SW = ("narrow_chain", "narrow_chain_backward", "bf16_chain", "bf16_backward", "native_chain_backward")
CORE_SW = ("bf16_backward", "narrow_backward", "typed_dropout")


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def load():
        raise AssertionError("the entry table loaded the library")
    monkeypatch.setattr(gn._lib, "load", load)


def want_block(direction, elem, sw, record):
    """(query, query_tail, call, head, tail, key) or NIE; the Dense block has no Dropout record: `record` changes nothing"""
    bf = elem == BF16
    if direction == "forward":
        if bf:
            return ("gnx_block_typed_workspace_bytes", (BF16, FL), "gnx_block_forward_typed", (BF16,), (FL,), ("block_bf16", "in_dims", "out_dims", "R", FL))
        return ("gnx_block_workspace_bytes", (), "gnx_block_forward", (), (FL,), ("block", "in_dims", "out_dims", "R"))
    if bf and "bf16_backward" not in sw:
        return NIE
    call, e = {(False, "plain"): ("gnx_block_backward", ()), (False, "fused"): ("gnx_block_backward_fused", ()), (False, "narrow"): ("gnx_block_backward_narrow", (F32,)),
               (True, "plain"): ("gnx_block_backward_typed", (BF16,)), (True, "fused"): ("gnx_block_backward_fused_typed", (BF16,)),
               (True, "narrow"): ("gnx_block_backward_narrow", (BF16,))}[
        (bf, "narrow" if "narrow_backward" in sw else "fused" if "fused_backward" in sw else "plain")]  # narrow_backward wins over fused_backward
    return (call + "_workspace_bytes", e, call, e, (), None)


def want_chain(direction, elem, sw, record):
    bf = elem == BF16
    if bf and ("bf16_chain" not in sw or record):
        return NIE
    if direction == "forward":
        n = int("narrow_chain" in sw)
        if record:
            return ("gnx_chain_block_forward_train_workspace_bytes", (n,), "gnx_chain_block_forward_train", (DR,), (n, FL), ("chain_train", n, "in_dims", "widths", "R"))
        if bf:
            return ("gnx_chain_block_forward_typed_workspace_bytes", (BF16, n), "gnx_chain_block_forward_typed", (BF16,), (n, FL),
                    ("chain_bf16", bool(n), "in_dims", "widths", "R"))
        if n:
            return ("gnx_chain_block_forward_narrow_workspace_bytes", (), "gnx_chain_block_forward_narrow", (), (FL,), ("chain_narrow", "in_dims", "widths", "R"))
        return ("gnx_chain_block_workspace_bytes", (), "gnx_chain_block_forward", (), (FL,), ("chain", "in_dims", "widths", "R"))
    if bf and "bf16_backward" not in sw:
        return NIE
    n = int("narrow_chain_backward" in sw)
    if record:
        return ("gnx_chain_block_backward_train_workspace_bytes", (n,), "gnx_chain_block_backward_train", (DR,), (n,), None)
    if bf and "native_chain_backward" in sw:
        return ("gnx_chain_block_backward_narrow_typed_workspace_bytes", (BF16,), "gnx_chain_block_backward_narrow_typed", (BF16,), (), None)
    if bf:
        return ("gnx_chain_block_backward_typed_workspace_bytes", (BF16, n), "gnx_chain_block_backward_typed", (BF16,), (n,), None)
    if n:
        return ("gnx_chain_block_backward_narrow_workspace_bytes", (), "gnx_chain_block_backward_narrow", (), (), None)
    return ("gnx_chain_block_backward_workspace_bytes", (), "gnx_chain_block_backward", (), (), None)


def want_core(direction, elem, sw, record):
    bf, typed, n = elem == BF16, "typed_dropout" in sw, int("narrow_backward" in sw)
    if direction == "forward":
        if record and typed:
            return ("gnx_core_train_typed_workspace_bytes", (elem, FL), "gnx_core_forward_train_typed", (elem, DR), (FL,), ("core_train_typed", "dims", "R", elem, FL))
        if record:
            return NIE if bf else ("gnx_core_train_workspace_bytes", (), "gnx_core_forward_train", (DR,), (FL,), ("core_train", "dims", "R"))
        if bf:
            return ("gnx_core_typed_workspace_bytes", (BF16, FL), "gnx_core_forward_typed", (BF16,), (FL,), ("core_bf16", "dims", "R", FL))
        return ("gnx_core_workspace_bytes", (), "gnx_core_forward", (), (FL,), ("core", "dims", "R"))
    if bf and "bf16_backward" not in sw:
        return NIE
    if record and typed:  # typed_dropout wins over narrow_backward
        return ("gnx_core_backward_train_typed_workspace_bytes", (elem, n), "gnx_core_backward_train_typed", (elem, DR, n), (), None)
    if n:
        return ("gnx_core_backward_narrow_workspace_bytes", (elem,), "gnx_core_backward_narrow", (elem, DR), (), None)
    if bf:
        return ("gnx_core_backward_typed_workspace_bytes", (BF16,), "gnx_core_backward_typed", (BF16,), (), None)
    if record:
        return ("gnx_core_backward_workspace_bytes", (), "gnx_core_backward_train", (DR,), (), None)
    return ("gnx_core_backward_workspace_bytes", (), "gnx_core_backward", (), (), None)


FAMILIES = {"block": (BLOCK_SW, want_block), "chain": (CHAIN_SW, want_chain), "core": (CORE_SW, want_core)}


def product():
    for family, (names, want) in FAMILIES.items():
        for direction, elem, record in itertools.product(("forward", "backward"), (F32, BF16), (False, True)):
            for bits in itertools.product((False, True), repeat=len(names)):
                sw = frozenset(s for s, b in zip(names, bits) if b)
                yield family, direction, elem, sw, record, want(direction, elem, sw, record)


def got(family, direction, elem, sw, record):
    try:
        return tuple(_entry(family, direction, elem, sw, record))
    except NotImplementedError:
        return NIE


def test_the_table_is_the_one_written_here():
    n = 0
    for family, direction, elem, sw, record, want in product():
        assert got(family, direction, elem, sw, record) == want, (family, direction, elem, sorted(sw), record)
        n += 1
    assert n == 2 * 2 * 2 * (2 ** 3 + 2 ** 5 + 2 ** 3)


@pytest.mark.parametrize("family,direction,elem,sw,record,call", [
    ("block", "backward", F32, {"fused_backward", "narrow_backward"}, False, "gnx_block_backward_narrow"),  # narrow_backward wins over fused_backward
    ("block", "backward", BF16, {"bf16_backward", "fused_backward", "narrow_backward"}, False, "gnx_block_backward_narrow"),
    ("core", "backward", F32, {"typed_dropout", "narrow_backward"}, True, "gnx_core_backward_train_typed"),  # typed_dropout wins over narrow_backward
    ("core", "backward", BF16, {"bf16_backward", "typed_dropout", "narrow_backward"}, True, "gnx_core_backward_train_typed"),
    ("core", "backward", F32, {"typed_dropout", "narrow_backward"}, False, "gnx_core_backward_narrow"),  # ... under an active record only
    ("chain", "backward", BF16, {"bf16_chain", "bf16_backward", "native_chain_backward"}, False, "gnx_chain_block_backward_narrow_typed"),
    ("chain", "backward", F32, {"native_chain_backward"}, False, "gnx_chain_block_backward"),  # native_chain_backward: bfloat16 features only
])
def test_the_orders_between_switches(family, direction, elem, sw, record, call):
    assert _entry(family, direction, elem, sw, record).call == call


def test_switches_the_family_does_not_have_change_nothing():
    every = set(BLOCK_SW) | set(CHAIN_SW) | set(CORE_SW) | {"bf16", "chain_dropout"}
    for family, direction, elem, sw, record, want in product():
        foreign = every - set(FAMILIES[family][0])
        assert got(family, direction, elem, sw | foreign, record) == want, (family, direction, elem, sorted(sw), record)


def test_a_query_belongs_to_its_call():
    """the query is `<call>_workspace_bytes`; a forward's may leave the `_forward` out (gnx_block_forward_typed: gnx_block_typed_workspace_bytes);
    the one exception is gnx_core_backward_train, sized by gnx_core_backward's query"""
    seen = set()
    for family, direction, elem, sw, record, want in product():
        if want == NIE:
            continue
        query, call = want[0], want[2]
        seen.add((query, call))
        assert direction in call
        if call == "gnx_core_backward_train":
            assert query == "gnx_core_backward_workspace_bytes"
        else:
            assert query in (call + "_workspace_bytes", call.replace("_forward", "", 1) + "_workspace_bytes"), (query, call)
    assert len({c for _, c in seen}) == len(seen) == 25  # a call has one query; 2 + 5 block, 4 + 5 chain, 4 + 5 core entries
    assert len({q for q, _ in seen}) == 24  # (gnx_core_backward_workspace_bytes sizes two calls)


def test_every_name_is_declared_in_the_header():
    with open(os.path.join(ROOT, "include", "gnx.h")) as f:
        declared = set(re.findall(r"\b(gnx_\w+)\s*\(", f.read()))
    for family, direction, elem, sw, record, want in product():
        if want != NIE:
            assert want[0] in declared and want[2] in declared, (want[0], want[2])


def test_the_switches_are_read_off_objects_that_predate_them():
    class Old:
        narrow_backward = True
        fused_backward = 0
    assert gn.api._switches(Old()) == {"narrow_backward"}
