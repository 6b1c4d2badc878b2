"""CPU-side checks of the Chain block's training entries (include/gnx.h: GNX_LAYER_DROPOUT, gnx_chain_dropout, gnx_chain_dropout_mask,
gnx_chain_block_train_applies, gnx_chain_block_forward_train / _backward_train and their queries): the six exports are declared, exported and
bound with equal parameter counts; gnx_chain_dropout has 32 bytes; every refusal of the record and of the Dropout entries is returned before any
GPU work, in the documented order, with gnx_last_error naming the cause; the existing entries still refuse layer kind 2; `_train_applies` on a
fake handle gives the masks of the Python restatement (tests/test_chain_train_plan_cpu.py); the resource record lists the 18 instantiations
without scratch; the Python layers record where a Dropout stood, and the switch is off by default."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_chain_narrow_abi import _fake_handle, _params
from tests.test_chain_train_plan_cpu import DENSE, DROP, train_masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnx_chain_dropout_mask", "gnx_chain_block_train_applies", "gnx_chain_block_forward_train_workspace_bytes", "gnx_chain_block_forward_train",
       "gnx_chain_block_backward_train_workspace_bytes", "gnx_chain_block_backward_train")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import graphnets_jl_amd as gn
    return gn._lib.load()


def test_entries_declared_exported_and_bound(lib, tmp_path):
    import graphnets_jl_amd as gn
    with open(os.path.join(ROOT, "include", "gnx.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        m = re.search(r"GNX_API [\w\s\*]+?\b" + name + r"\(([^;]*?)\);", text, flags=re.S)
        assert m, f"{name} is not declared in include/gnx.h"
        assert hasattr(lib, name), f"{name} is not exported by libgnx.so"
        assert name in gn._lib.SIGNATURES
        assert m.group(1).count(",") + 1 == len(gn._lib.SIGNATURES[name][1]), name
    assert lib.gnx_version() == 130
    assert re.search(r"#define GNX_LAYER_DROPOUT 2\b", text) and gn._lib.LAYER_DROPOUT == 2
    assert C.sizeof(gn._lib.ChainDropout) == 32 and C.sizeof(gn._lib.Dense) == 24
    src = tmp_path / "abi.c"
    src.write_text('#include "gnx.h"\n_Static_assert(sizeof(gnx_chain_dropout) == 32, "gnx_chain_dropout");\n_Static_assert(sizeof(gnx_dense) == 24, "gnx_dense");\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def _with_dropouts(gn, where, in_dims=(10, 5, 0), widths=((16, 3), (8, 4), (6, 5))):
    """_params with Dropout entries: where = {function index: [entry index of the resulting chain, ...]}; returns (params, keep, entry kinds)"""
    L = gn._lib
    p, keep = _params(gn, in_dims, widths)
    kinds = []
    for t, name in enumerate(("edgefn", "nodefn", "graphfn")):
        ch = getattr(p, name)
        src_layers = [ch.layers[i] for i in range(ch.n_layers)]
        src_widths = [ch.widths[i] for i in range(ch.n_layers)]
        n = ch.n_layers + len(where.get(t, ()))
        arr, wid, ks, j = (L.Dense * max(n, 1))(), (C.c_int32 * max(n, 1))(), [], 0
        for e in range(n):
            if e in where.get(t, ()):
                arr[e], wid[e] = L.Dense(None, None, 0, L.LAYER_DROPOUT), (wid[e - 1] if e else in_dims[0])
                ks.append(DROP)
            else:
                arr[e], wid[e] = src_layers[j], src_widths[j]
                ks.append(DENSE)
                j += 1
        keep += [arr, wid]
        ch.layers, ch.widths, ch.n_layers = arr, wid, n
        kinds.append([(wid[e], ks[e]) for e in range(n)])
    return p, keep, kinds


def _record(gn, p, value=0.25, seed=1):
    L = gn._lib
    d = L.ChainDropout()
    d.seed = seed
    keep = []
    for t, name in enumerate(("edgefn", "nodefn", "graphfn")):
        arr = (C.c_float * 16)(*([value] * 16))
        keep.append(arr)
        d.p[t] = C.cast(arr, C.POINTER(C.c_float))
    return d, keep


def _calls(lib, gn, fake, p, drop, narrow=0, R=1):
    """the two training calls on host buffers; every case below ends before any GPU work"""
    buf = np.full(4096, 7.0, dtype=np.float32)
    ws = np.full(1024, 0x5A, dtype=np.uint8)
    b = buf.ctypes.data
    d = None if drop is None else C.byref(drop)
    pp = None if p is None else C.byref(p)
    fw = lib.gnx_chain_block_forward_train(fake, pp, d, b, b, None, R, b, b, b, ws.ctypes.data, ws.nbytes, narrow, 0, None)
    e1 = lib.gnx_last_error()
    bw = lib.gnx_chain_block_backward_train(fake, pp, d, b, b, None, b, b, b, R, b, b, None, None, ws.ctypes.data, ws.nbytes, narrow, None)
    e2 = lib.gnx_last_error()
    assert np.all(buf == 7.0) and np.all(ws == 0x5A)
    return (fw, e1), (bw, e2)


def test_refusals_in_their_order_before_any_gpu_work(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    hbuf = _fake_handle(G=3)
    fake = C.c_void_p(hbuf.ctypes.data)
    good, _k, _ = _with_dropouts(gn, {0: [1], 1: [1], 2: [2]})
    rec, _kr = _record(gn, good)

    def refused(p, drop, cause, narrow=0, R=1, code=L.ERR_INVALID_ARG, handle=fake, bw_code=None):
        for (rc, err), want in zip(_calls(lib, gn, handle, p, drop, narrow, R), (code, code if bw_code is None else bw_code)):
            assert rc == want and cause in err, (rc, err, cause)
        if p is not None and handle is not None:
            for q in (lib.gnx_chain_block_forward_train_workspace_bytes, lib.gnx_chain_block_backward_train_workspace_bytes):
                if drop is None or narrow not in (0, 1) or R != 1:  # (the queries see no record)
                    assert q(handle, C.byref(p), R, narrow) == 0

    refused(good, rec, b"NULL handle or params", handle=None)
    refused(None, rec, b"NULL handle or params")
    # a p outside [0, 1] — before everything else about the entries, whatever narrow is
    for bad in (1.5, -0.25, float("nan")):
        r, _ = _record(gn, good, bad)
        refused(good, r, b"p must lie in [0, 1]", narrow=7)
    r, _ = _record(gn, good, 1.5)
    misplaced, _k2, _ = _with_dropouts(gn, {0: [0]})
    refused(misplaced, r, b"p must lie in [0, 1]")  # (the order: p first, then the entry's place)
    # a NULL p[t] for a function with a Dropout entry
    r, _ = _record(gn, good)
    r.p[1] = None
    refused(good, r, b"gnx_chain_dropout.p of the function is NULL", narrow=7)
    plain, _k3 = _params(gn)
    # misplaced or malformed entries (with and without a record)
    for where, cause in (({0: [0]}, b"follows a Dense or LayerNorm"), ({1: [1, 2]}, b"follows a Dense or LayerNorm")):
        bad, _kb, _ = _with_dropouts(gn, where)
        for drop in (rec, None):
            refused(bad, drop, cause, narrow=7)
    bad, _kb, _ = _with_dropouts(gn, {0: [1]})
    bad.edgefn.widths[1] = 15
    refused(bad, rec, b"keeps the width")
    bad, _kb, _ = _with_dropouts(gn, {0: [1]})
    bad.edgefn.layers[1].act = 1
    refused(bad, rec, b"no weight, no bias and no activation")
    bad, _kb, _ = _with_dropouts(gn, {0: [1]})
    bad.edgefn.layers[1].weight = bad.edgefn.layers[0].weight
    refused(bad, rec, b"no weight, no bias and no activation")
    # narrow other than 0 / 1, then the mirrored entry's refusals (the pullback's: one code for every refused parameter set)
    refused(good, rec, b"narrow must be 0 or 1", narrow=2)
    refused(good, rec, b"narrow must be 0 or 1", narrow=-1)
    refused(good, rec, b"bad n_replicas", R=0, bw_code=L.ERR_DIMS)
    refused(good, rec, b"bad n_replicas", R=2, bw_code=L.ERR_DIMS)  # R > 1 on a batch of three graphs
    neg, _kn, _ = _with_dropouts(gn, {0: [1]}, in_dims=(-1, 5, 0))
    refused(neg, rec, b"negative feature width", code=L.ERR_DIMS)
    # _train_applies: 0 on bad arguments
    for h, pp, R, b in ((None, C.byref(good), 1, 0), (fake, None, 1, 0), (fake, C.byref(good), 1, 2), (fake, C.byref(good), 0, 0), (fake, C.byref(misplaced), 1, 0)):
        assert lib.gnx_chain_block_train_applies(h, pp, R, b) == 0


def test_the_existing_entries_still_refuse_kind_two(lib):
    import graphnets_jl_amd as gn
    L = gn._lib
    hbuf = _fake_handle()
    fake = C.c_void_p(hbuf.ctypes.data)
    p, _k, _ = _with_dropouts(gn, {0: [1]})
    buf = np.full(4096, 7.0, dtype=np.float32)
    ws = np.full(1024, 0x5A, dtype=np.uint8)
    b, w = buf.ctypes.data, ws.ctypes.data
    for q in (lib.gnx_chain_block_workspace_bytes, lib.gnx_chain_block_forward_narrow_workspace_bytes, lib.gnx_chain_block_forward_narrow_applies,
              lib.gnx_chain_block_backward_workspace_bytes, lib.gnx_chain_block_backward_narrow_workspace_bytes, lib.gnx_chain_block_backward_narrow_applies):
        assert q(fake, C.byref(p), 1) == 0
    for entry in (lib.gnx_chain_block_forward, lib.gnx_chain_block_forward_narrow):
        assert entry(fake, C.byref(p), b, b, None, 1, b, b, b, w, ws.nbytes, 0, None) == L.ERR_INVALID_ARG and b"unknown layer kind" in lib.gnx_last_error()
    assert lib.gnx_chain_block_forward_typed(fake, C.byref(p), L.ELEM_F32, b, b, None, 1, b, b, b, w, ws.nbytes, 1, 0, None) == L.ERR_INVALID_ARG
    assert b"unknown layer kind" in lib.gnx_last_error()
    for entry in (lib.gnx_chain_block_backward, lib.gnx_chain_block_backward_narrow):
        assert entry(fake, C.byref(p), b, b, None, b, b, b, 1, b, b, None, None, w, ws.nbytes, None) != 0 and b"unknown layer kind" in lib.gnx_last_error()
    assert lib.gnx_chain_block_backward_typed(fake, C.byref(p), L.ELEM_F32, b, b, None, b, b, b, 1, b, b, None, None, w, ws.nbytes, 1, None) != 0
    assert b"unknown layer kind" in lib.gnx_last_error()
    assert lib.gnx_chain_block_backward_narrow_typed(fake, C.byref(p), L.ELEM_F32, b, b, None, b, b, b, 1, b, b, None, None, w, ws.nbytes, None) != 0
    assert b"unknown layer kind" in lib.gnx_last_error()
    assert np.all(buf == 7.0) and np.all(ws == 0x5A)


def test_train_applies_is_the_restatement(lib):
    import graphnets_jl_amd as gn
    hbuf = _fake_handle(G=1, N=4, E=6)
    fake = C.c_void_p(hbuf.ctypes.data)
    for where, in_dims, widths in (
            ({0: [1], 1: [1], 2: [1]}, (10, 5, 0), ((16, 3), (8, 4), (6, 5))),
            ({0: [1, 3]}, (10, 5, 3), ((32, 32, 3), (8, 4), (6, 5))),            # [32,do,32,do,3]: the forward's rule alone
            ({0: [2], 2: [2]}, (10, 5, 0), ((16, 3), (8, 4), (6, 5))),           # a Dropout as last entry
            ({0: list(range(1, 16, 2))}, (3, 2, 1), ((8,) * 8, (8, 4), (6, 5))),  # eight 8-wide layers, a Dropout after each
            ({1: [1]}, (10, 5, 0), ((33, 3), (8, 4), (6, 5))),
            ({}, (10, 5, 0), ((16, 3), (8, 4), (6, 5)))):
        p, _k, kinds = _with_dropouts(gn, where, in_dims, widths)
        fw, bw = train_masks(in_dims, kinds, (6, 4, 1))
        assert lib.gnx_chain_block_train_applies(fake, C.byref(p), 1, 0) == fw, (where, fw)
        assert lib.gnx_chain_block_train_applies(fake, C.byref(p), 1, 1) == bw, (where, bw)
        if not where:  # without Dropout entries: the test-mode rules
            assert fw == lib.gnx_chain_block_forward_narrow_applies(fake, C.byref(p), 1) and bw == lib.gnx_chain_block_backward_narrow_applies(fake, C.byref(p), 1)


def test_resource_record_lists_the_eighteen_instantiations_without_scratch():
    with open(os.path.join(ROOT, "profiles", "chain_train_narrow_resources.json")) as f:
        rec = json.load(f)
    n = 0
    for direction in ("forward", "backward"):
        for src in ("edge", "node", "rows"):
            for w in ("8", "16", "32"):
                r = rec["kernels"][direction]["srcs"][src][w]
                assert r["scratch"] == 0 and r["lds_static"] == 0 and 0 < r["vgpr"] <= 256, (direction, src, w, r)
                n += 1
    assert n == 18 and rec["instantiations_with_scratch_or_static_lds"] == []


def test_python_layers_record_the_dropouts_and_the_switch_is_off(lib):
    import torch
    import graphnets_jl_amd as gn
    d = lambda i, o, act="identity": gn.Dense.from_numpy(np.zeros((o, i), dtype=np.float32), np.zeros(o, dtype=np.float32), act, device="cpu")
    l0, l1 = d(20, 16, "relu"), d(16, 3)
    ch = gn.Chain(l0, gn.Dropout(0.1), l1, gn.Dropout(0.0), gn.Dropout(0.4))
    assert ch.layers == [l0, l1] and ch.dropout_p == 0.4 and len(ch) == 2       # as before
    assert ch.dropouts == [(1, 0.1), (2, 0.0), (2, 0.4)]
    assert [k for k, _ in ch._entries()] == ["layer", "dropout", "layer", "dropout", "dropout"]
    assert gn.Chain(l0, l1).dropouts == []
    blk = gn.GNBlock((10, 5, 0), (3, 4, 5), device="cpu")
    assert blk.chain_dropout is False and gn.GNBlock((10, 5, 0), (3, 4, 5), device="cpu", chain_dropout=True).chain_dropout is True
    assert gn.testmode(blk)._dropout_mode is False and gn.trainmode(blk)._dropout_mode is True and gn.testmode(blk, None)._dropout_mode is None
    rec = gn.ChainDropout(7, [[0.0, 0.1, 0.0], [], []])
    keep = []
    c = rec._c(keep)
    assert c.seed == 7 and abs(c.p[0][1] - 0.1) < 1e-7
