"""Training mode of a GNBlock with Chain update functions: Dropout entries inside the chains (include/gnx.h, gnx_chain_block_forward_train /
_backward_train, gnx_chain_dropout_mask, gnx_chain_block_train_applies) — the mask's bits, the identity cases, p = 1, both directions against
float64 with the library's masks as constants, the launch structure, the memory contract, stream capture and the Python switch."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

from oracle import gn_oracle as O
from tests import arena as AR
from tests import chain_dropout_ref as DR
from tests import util as U
from tests import test_gpu_chain_narrow as CN
from tests.test_chain_train_plan_cpu import DENSE, DROP, LN, train_masks
from tests.test_gpu_memory_contract import _chain_out_widths, _chain_params, _decl, _decl_chains, _decl_dense_grad, _decl_outputs, _dense_grad

pytestmark = pytest.mark.gpu
EXTRA = int(os.environ.get("GNX_FUZZ_EXTRA", "0"))
NAMES = CN.NAMES


@pytest.fixture(scope="module")
def gn():
    import torch
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


def _batch(kind, rng):
    """(adjacency matrices, R): the five graphs of 3..40 nodes; E > 256 with E % 64 != 0; one 300-node graph (node rows cross a workgroup); a
    single 31-node graph with 2 and 3 replicas"""
    if kind == "five":
        return CN._adjs(rng), 1
    if kind == "partial-workgroup":
        adjs = CN._adjs(rng, [37, 5, 29, 33, 11])
        E = int(sum(a.sum() for a in adjs))
        assert E > 256 and E % 64 != 0, E
        return adjs, 1
    if kind == "300-nodes":
        return [(rng.random((300, 300)) < 0.02).astype(np.int64)], 1
    return CN._adjs(rng, [31]), int(kind[-1])  # "replicas-2", "replicas-3"


def _want_masks(c):
    """the Python restatement of both training rules (tests/test_chain_train_plan_cpu.py) on the call's chains"""
    chains = []
    for name in DR.FN:
        ws, es = DR.widths(c.p, name), []
        for kind, v in c.ent[name]:
            es.append((es[-1][0], DROP) if kind == "dropout" else (ws[v], LN if isinstance(c.p[name][v][0], str) else DENSE))
        chains.append(es)
    return train_masks(c.p["in_dims"], chains, c.rows)


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


# ---- 1. the mask's bits ----
LAST_DROP_CASES = {8: ((2, 1, 0), [8, 3], [8, 5], [8, 7]), 16: ((3, 2, 1), [16, 3], [16, 5], [12, 7]), 32: ((8, 8, 8), [32, 3], [32, 5], [32, 7])}


@pytest.mark.parametrize("batch", ("five", "replicas-2"))
@pytest.mark.parametrize("wmax", (8, 16, 32))
def test_a_last_dropout_is_the_test_mode_output_times_the_exported_mask(gn, wmax, batch):
    """last widths 3, 5, 7 (rows start at every i % 4), the three source forms, both `narrow` values: exactly, element by element"""
    import torch
    rng = np.random.default_rng(40 + wmax)
    adjs, R = _batch(batch, rng)
    in_dims, ew, nw, gw = LAST_DROP_CASES[wmax]
    p = O.make_chain_block_params(rng, in_dims, ew, nw, gw)
    c = DR.TrainCall(gn, adjs, p, {name: {1: 0.3} for name in DR.FN}, R, seed=wmax)
    rec = c.record(seed=0x1234567 + wmax)
    m = c.masks(rec)
    assert c.applies(0) == 7
    for narrow in (0, 1):
        got = c.fw(narrow, rec)
        base, _ = c.fw_stripped(narrow)
        # (ef' and nf' of the training call are dropped before the next function reads them: compare function by function on the same inputs)
        torch.cuda.synchronize()
        mk = torch.from_numpy(m["edge"][2]).to(c.g.device)
        assert torch.equal(_bits(got[0]), _bits(base[0] * mk)), f"edge narrow={narrow}"
    # node / graph function: a block whose edge (and node) function has no Dropout, so that the inputs of the function agree with the stripped call's
    for t, name in ((1, "node"), (2, "graph")):
        c2 = DR.TrainCall(gn, adjs, p, {name: {1: 0.3}}, R, seed=wmax)
        rec2 = c2.record(seed=77 + t)
        mk = torch.from_numpy(c2.masks(rec2)[name][2]).to(c2.g.device)
        for narrow in (0, 1):
            got = c2.fw(narrow, rec2)
            base, _ = c2.fw_stripped(narrow)
            torch.cuda.synchronize()
            assert torch.equal(_bits(got[t]), _bits(base[t] * mk)), f"{name} narrow={narrow}"
            if t == 1:  # (the graph function then reads the dropped nf')
                assert torch.equal(_bits(got[0]), _bits(base[0]))


def test_masks_are_the_definition_and_differ_between_streams(gn):
    import torch
    lib, L = gn._lib.load(), gn._lib
    n, seed = 100003, 0xC0FFEE12345
    rec = gn.ChainDropout(seed, [[0.3] * 16] * 3)
    keep = []
    crec = rec._c(keep)

    def mask(t, l, p=0.3, count=n):
        out = torch.full((count,), float("nan"), dtype=torch.float32, device="cuda")
        assert lib.gnx_chain_dropout_mask(C.byref(crec), t, l, p, count, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0, lib.gnx_last_error()
        return out.cpu().numpy()

    seen = {}
    for t, l in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 15), (0, 15)):
        seen[(t, l)] = mask(t, l)
        assert np.array_equal(seen[(t, l)], DR.mask_numpy(seed, t, l, 0.3, n)), (t, l)  # include/gnx.h's definition restated on the host
        assert set(np.unique(seen[(t, l)])) == {np.float32(0), np.float32(1) / (np.float32(1) - np.float32(0.3))}
    keys = list(seen)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert not np.array_equal(seen[a], seen[b]), (a, b)
    core = L.Dropout(0.3, 0, seed)
    for entity in range(3):  # GNCore's entities 0..2 under the same seed
        out = torch.empty((n,), dtype=torch.float32, device="cuda")
        assert lib.gnx_dropout_mask(C.byref(core), entity, n, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        for k in keys:
            assert not np.array_equal(out.cpu().numpy(), seen[k]), (entity, k)
    # the kept share of 10^5 elements at p = 0.3: within 5 sigma of 0.7
    m = mask(1, 3, count=100000)
    share = float((m != 0).mean())
    print(f"kept share at p = 0.3 over 1e5 elements: {share:.5f}")
    assert abs(share - 0.7) <= 5 * np.sqrt(0.3 * 0.7 / 100000), share
    # p = 0 keeps everything at scale 1, p = 1 drops everything; refusals
    assert np.all(mask(0, 0, p=0.0, count=1000) == 1) and np.all(mask(0, 0, p=1.0, count=1000) == 0)
    out = torch.empty((8,), dtype=torch.float32, device="cuda")
    for t, l, p in ((3, 0, 0.3), (-1, 0, 0.3), (0, 16, 0.3), (0, -1, 0.3), (0, 0, 1.5), (0, 0, -0.1)):
        assert lib.gnx_chain_dropout_mask(C.byref(crec), t, l, p, 8, out.data_ptr(), None) == L.ERR_INVALID_ARG, (t, l, p)


# ---- 2. the identity cases ----
@pytest.mark.parametrize("narrow", (0, 1))
def test_identity_cases_are_the_mirrored_entry_on_the_stripped_chain(gn, narrow):
    import torch
    rng = np.random.default_rng(50)
    adjs, R = _batch("five", rng)
    p = O.make_chain_block_params(rng, (10, 5, 3), [16, "ln", 3], [8, 4], [6, 5], acts=(1, 2, 3))
    c = DR.TrainCall(gn, adjs, p, {"edge": {0: 0.25, 1: 0.5, 2: 0.1}, "node": {0: 0.25}, "graph": {1: 0.4}}, R)
    cot = c.cotangents(1)
    base, fw_bytes = c.fw_stripped(narrow)
    gbase, bw_bytes = c.bw_stripped(narrow, cot)
    # the training queries on the stripped chains are the mirrored queries; an identity call takes a workspace of that size
    assert c.query(narrow, stripped=True) == fw_bytes and c.query(narrow, backward=True, stripped=True) == bw_bytes
    assert c.query(narrow) >= fw_bytes and c.query(narrow, backward=True) >= bw_bytes
    for rec in (None, c.record(5, scale_p=0.0)):
        got = c.fw(narrow, rec, nbytes=fw_bytes)
        grads = c.bw(narrow, rec, cot, nbytes=bw_bytes)
        torch.cuda.synchronize()
        for u, v in zip(got, base):
            assert torch.equal(_bits(u), _bits(v))
        assert set(grads) == set(gbase)
        for n in gbase:
            assert torch.equal(_bits(grads[n]), _bits(gbase[n])), n


# ---- 3. p = 1 ----
@pytest.mark.parametrize("narrow", (0, 1))
def test_p_one_drops_everything(gn, narrow):
    import torch
    rng = np.random.default_rng(60)
    adjs, R = _batch("five", rng)
    p = O.make_chain_block_params(rng, (10, 5, 3), [16, 12, 3], [8, 4], [6, 5], acts=(1, 1, 1))
    c = DR.TrainCall(gn, adjs, p, {"edge": {1: 1.0}, "node": {0: 1.0}, "graph": {0: 1.0}}, R)
    rec = c.record(9)
    got = c.fw(narrow, rec)
    grads = c.bw(narrow, rec, c.cotangents(2))
    torch.cuda.synchronize()
    for t, name in enumerate(DR.FN):  # the Dense behind the entry is the last, linear layer: act(bias) in every row
        b = torch.from_numpy(p[name][-1][1]).to(c.g.device)
        assert torch.equal(_bits(got[t]), _bits(b.expand_as(got[t]))), name
    zero = lambda n: bool((grads[n] == 0).all())
    assert zero("d_ef") and zero("d_nf") and zero("d_gf")
    for name, upstream, behind in (("edge", (0, 1), 2), ("node", (0,), 1), ("graph", (0,), 1)):
        for i in upstream:
            assert zero(f"{name}{i}.dW") and zero(f"{name}{i}.db"), (name, i)
        assert zero(f"{name}{behind}.dW"), name
        assert not zero(f"{name}{behind}.db"), name  # (the bias gradient is the column sum of the upstream gradient)


# ---- 4. the forward against float64 ----
FW_CASES = [(i, "hidden") for i in range(len(CN.WIDTH_CASES))] + [(2, "behind-ln"), (0, "last")]
FW_BATCH = {0: "five", 1: "replicas-2", 2: "partial-workgroup", 3: "300-nodes", 4: "five", 5: "replicas-3", 6: "five", 7: "five"}


def _drops(p, how):
    if how == "hidden":
        return DR.drop_after_hidden(p)
    if how == "behind-ln":
        return {name: {i: 0.25 for i, l in enumerate(p[name]) if isinstance(l[0], str) and i > 0} for name in DR.FN}
    return {name: {len(p[name]) - 1: 0.25} for name in DR.FN if p[name]}


@pytest.mark.parametrize("i,how", FW_CASES, ids=[f"{CN.WIDTH_CASES[i][:4]}-{how}" for i, how in FW_CASES])
def test_forward_against_float64(gn, i, how):
    import torch
    rng = np.random.default_rng(100 + i)
    adjs, R = _batch(FW_BATCH[i] if how == "hidden" else "five", rng)
    p = CN._params(rng, CN.WIDTH_CASES[i])
    c = DR.TrainCall(gn, adjs, p, _drops(p, how), R, seed=i)
    assert any(c.drops.get(n) for n in DR.FN)
    fw, bw = _want_masks(c)
    assert (c.applies(0), c.applies(1)) == (fw, bw), (c.applies(0), c.applies(1), fw, bw)
    rec = c.record(1000 + i)
    ref, scale, _, _ = c.reference(c.masks(rec))
    for narrow in (0, 1):
        got = c.fw(narrow, rec)
        torch.cuda.synchronize()
        worst = 0.0
        for name, o, r, s in zip(("ef", "nf", "gf"), got, ref, scale):
            if r is not None and r.size:
                worst = max(worst, float(np.max(np.abs(o.cpu().numpy().astype(np.float64) - r) / (U.RTOL * s + 1e-30))))
            U.assert_close(None if o is None else o.cpu().numpy(), r, s, f"narrow={narrow} {name}")
        print(f"chain train forward {CN.WIDTH_CASES[i][:4]} {how} narrow={narrow}: worst |diff| / (1e-5 scale) = {worst:.3e}")


# ---- 5. the pullback against float64 torch autograd ----
BW_CASES = [
    ((10, 5, 0), [16, 3], [8, 4], [6, 5], (1, 2, 0), "hidden", "five"),
    ((2, 2, 1), [8, 8, 1], [8, 3], [4, 2], (1, 1, 1), "hidden", "replicas-2"),
    ((3, 2, 1), [9, 17, 4], [16, "ln", 5], ["ln", 9, 4], (4, 3, 1), "hidden", "partial-workgroup"),  # (no LayerNorm right behind a dropped relu row:
                                                                                                     #  an all-zero row is its singular point)
    ((8, 8, 8), [32, 7], [32, 9], [32, "ln", 4], (1, 2, 0), "hidden", "300-nodes"),
    ((10, 5, 3), ["ln", 12, 7], [6, "ln", 3], [4, 4], (1, 2, 0), "hidden", "five"),       # LayerNorm-first edge function: the indices are the caller's
    ((10, 5, 3), [16, "ln", 3], [8, 4], [6, 5], (1, 2, 3), "behind-ln", "five"),
    ((10, 5, 3), [16, 3], [8, 4], [6, 5], (1, 2, 0), "last", "replicas-3"),
]


def _make_bw(gn, k):
    """a kink-free draw: no relu pre-activation of the float64 restatement (under the call's masks) within fp32 rounding of 0"""
    in_dims, ew, nw, gw, acts, how, batch = BW_CASES[k]
    for attempt in range(20):
        rng = np.random.default_rng(800 + k + 1000 * attempt)
        adjs, R = _batch(batch, rng)
        p = O.make_chain_block_params(rng, in_dims, ew, nw, gw, acts=acts)
        c = DR.TrainCall(gn, adjs, p, _drops(p, how), R, seed=k + 1000 * attempt)
        rec = c.record(2000 + k)
        cot = c.cotangents(k)
        _, _, grads, ok = c.reference(c.masks(rec), cot)
        if ok:
            print(f"kink-free at attempt {attempt}")
            return c, rec, cot, grads
    pytest.fail("no kink-free draw in 20 attempts")


@pytest.mark.parametrize("k", range(len(BW_CASES)), ids=[f"{c[:4]}-{c[5]}" for c in BW_CASES])
def test_backward_against_float64_autograd(gn, k):
    import torch
    c, rec, cot, ref = _make_bw(gn, k)
    generic = c.bw(0, rec, cot)
    fused = c.bw(1, rec, cot)
    torch.cuda.synchronize()
    print(f"training pullback mask {c.applies(1)} of {BW_CASES[k][:4]}")
    for n, r in ref.items():
        if r.size == 0:
            continue
        eg = float(np.max(np.abs(generic[n].cpu().numpy().astype(np.float64) - r)))
        en = float(np.max(np.abs(fused[n].cpu().numpy().astype(np.float64) - r)))
        floor = 1e-5 * max(1.0, float(np.abs(r).max()))
        print(f"  {n}: generic err {eg:.3e}, fused err {en:.3e}, 1e-5 max(1, max|ref|) = {floor:.3e}")
        assert np.isfinite(eg) and eg <= floor, f"{n}: generic err {eg:.3e} > {floor:.3e}"
        assert np.isfinite(en) and en <= max(4.0 * eg, floor), f"{n}: fused err {en:.3e}, generic err {eg:.3e}, floor {floor:.3e}"


# ---- 6. the launch structure ----
def test_launch_structure(gn):
    import torch
    if U.default_flags(gn) != 0:
        return  # (forms switched on for the whole process change which kernels the generic entry runs)
    rng = np.random.default_rng(70)
    adjs, R = _batch("five", rng)
    p = O.make_chain_block_params(rng, (4, 3, 3), [16, 8, 3], [8, 4], [6, 5])  # (k_in 13: an edge function at register width 32 is cut from the pullback's rule)
    c = DR.TrainCall(gn, adjs, p, DR.drop_after_hidden(p), R)
    n_entries = sum(len(d) for d in c.drops.values())
    assert n_entries == 4 and c.applies(0) == 7 and c.applies(1) == 7
    rec, cot = c.record(3), c.cotangents(3)
    c.fw(1, rec); c.bw(1, rec, cot); c.fw(0, rec); c.bw(0, rec, cot)
    fw = CN._profiled(gn, lambda: c.fw(1, rec))
    assert sorted(fw) == sorted(NAMES), sorted(fw)  # one kernel per function under the test-mode names, no k_dropout
    assert all(fw[n]["launches"] == 1 and fw[n]["kernels"] == 1 for n in NAMES), fw
    bw = CN._profiled(gn, lambda: c.bw(1, rec, cot))
    ref = CN._profiled(gn, lambda: c.bw_stripped(True, cot))
    assert "k_dropout" not in bw and sorted(bw) == sorted(ref), (sorted(bw), sorted(ref))
    assert all((bw[n]["launches"], bw[n]["kernels"]) == (ref[n]["launches"], ref[n]["kernels"]) for n in ref), (bw, ref)
    # the generic path: one k_dropout per active entry and direction (the pullback call recomputes the forward, then pulls back)
    gfw = CN._profiled(gn, lambda: c.fw(0, rec))
    assert gfw["k_dropout"]["kernels"] == n_entries, gfw["k_dropout"]
    gbw = CN._profiled(gn, lambda: c.bw(0, rec, cot))
    assert gbw["k_dropout"]["kernels"] == 2 * n_entries, gbw["k_dropout"]
    half = c.record(3)
    half.p[0] = [0.0] * len(half.p[0])  # the edge function's entries off: removed from the call
    assert CN._profiled(gn, lambda: c.fw(0, half))["k_dropout"]["kernels"] == n_entries - len(c.drops["edge"])


# ---- 7. the memory contract ----
@pytest.mark.parametrize("narrow", (0, 1))
@pytest.mark.parametrize("direction", ("forward", "backward"))
def test_memory_contract(gn, direction, narrow):
    """every buffer carved at its exact size, 4-byte aligned only, the workspace exactly the query's; nothing but the outputs and the
    workspace is written; the bits depend neither on what the workspace held nor on the run; optional outputs NULL"""
    import torch
    L, lib = gn._lib, gn._lib.load()
    rng = np.random.default_rng(300 + narrow)
    adjs, R = _batch("five", rng)
    g = gn.GNGraphBatch(adjs)
    p = O.make_chain_block_params(rng, (3, 2, 1), [9, 17, 4], [16, "ln", 5], ["ln", 9, 4], acts=(4, 3, 1))
    drops = DR.drop_after_hidden(p)
    ent = DR.entries(p, drops)
    a = AR.Arena("cuda", skew=lambda c: 0 if c.kind == AR.WORKSPACE else 4)
    _decl_chains(a, p)
    x = U.packed_inputs(rng, R, g.n_edges, g.n_nodes, g.n_graphs, p["in_dims"])
    ins = [_decl(a, n, v) for n, v in zip(("ef", "nf", "gf"), x)]
    keep = []
    params = lambda: DR.insert_dropouts(L, _chain_params(gn, a, p, keep), ent, keep)
    rec = gn.ChainDropout(4242, [[v if k == "dropout" else 0.0 for k, v in ent[name]] for name in DR.FN])
    crec = rec._c(keep)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    if direction == "forward":
        outs = _decl_outputs(a, "", R, (g.n_edges, g.n_nodes, g.n_graphs), _chain_out_widths(p))
        ws = a.workspace("ws", lambda: lib.gnx_chain_block_forward_train_workspace_bytes(g._h, C.byref(params()), R, narrow))
        call = lambda nbytes: lib.gnx_chain_block_forward_train(g._h, C.byref(params()), C.byref(crec), *map(a.ptr, ins), R, *map(a.ptr, outs), a.ptr(ws), nbytes,
                                                                narrow, 0, stream())
        query = b"gnx_chain_block_forward_train_workspace_bytes()"
    else:
        gs = [_decl(a, n, rng.standard_normal((R, T, d)).astype(np.float32)) for n, T, d in
              zip(("g_ef_out", "g_nf_out", "g_gf_out"), (g.n_edges, g.n_nodes, g.n_graphs), _chain_out_widths(p))]
        dx = [a.output("d_ef", x[0].shape), None, a.output("d_gf", x[2].shape)]  # d_nf not wanted
        for name in DR.FN:
            for i, (w, b, c) in enumerate(p[name]):
                if (name, i) == ("node", 0):
                    continue  # a parameter gradient that is not wanted
                if isinstance(w, str):
                    a.output(f"grad.{name}{i}.dW", b.shape); a.output(f"grad.{name}{i}.db", c.shape)
                else:
                    _decl_dense_grad(a, f"grad.{name}{i}", w, b)
        ws = a.workspace("ws", lambda: lib.gnx_chain_block_backward_train_workspace_bytes(g._h, C.byref(params()), R, narrow))

        def call(nbytes):
            arrays = []
            for name in DR.FN:
                arr = (L.DenseGrad * max(len(ent[name]), 1))()
                for e, (kind, v) in enumerate(ent[name]):
                    arr[e] = L.DenseGrad(None, None) if kind == "dropout" or (name, v) == ("node", 0) else _dense_grad(gn, a, f"grad.{name}{v}")
                arrays.append(arr)
            gr = L.ChainBlockGrads(*[C.cast(q, C.POINTER(L.DenseGrad)) for q in arrays])
            return lib.gnx_chain_block_backward_train(g._h, C.byref(params()), C.byref(crec), *map(a.ptr, ins), *map(a.ptr, gs), R, *map(a.ptr, dx), C.byref(gr),
                                                      a.ptr(ws), nbytes, narrow, stream())
        query = b"gnx_chain_block_backward_train_workspace_bytes()"
    a.build(ws_fill=0x00)
    assert a.nbytes(ws) > 0, lib.gnx_last_error()
    assert all(a.ptr(n) % 8 == 4 for n in ins if n is not None)
    bits = []
    for fill in (0x00, 0xFF, 0xFF):
        a.refill(fill)
        torch.cuda.synchronize()
        rc = call(a.nbytes(ws))
        torch.cuda.synchronize()
        assert rc == 0, lib.gnx_last_error()
        a.check(f"workspace {fill:#04x}")
        bits.append(a.output_bits())
    for k in bits[0]:
        assert torch.equal(bits[0][k], bits[1][k]), f"'{k}' depends on what the workspace held"
        assert torch.equal(bits[1][k], bits[2][k]), f"'{k}' differs between two calls"
    a.refill(0x00)
    rc = call(a.nbytes(ws) - 1)
    torch.cuda.synchronize()
    assert rc == L.ERR_WORKSPACE and query in lib.gnx_last_error(), lib.gnx_last_error()
    a.check("refused", unwritten=False)


# ---- 8. capture ----
@pytest.mark.parametrize("narrow", (0, 1))
def test_a_captured_call_replays_the_eager_bits(gn, narrow):
    """the seed travels by value: the record is gone when the graph replays"""
    import torch
    rng = np.random.default_rng(80)
    adjs, R = _batch("five", rng)
    p = O.make_chain_block_params(rng, (10, 5, 3), [16, 3], [8, 4], [6, 5])
    c = DR.TrainCall(gn, adjs, p, DR.drop_after_hidden(p), R)
    cot = c.cotangents(4)
    nf, nb = c.query(narrow), c.query(narrow, backward=True)  # (the queries build the tables the calls read, outside the capture)
    wf, wb = (torch.zeros((n,), dtype=torch.uint8, device=c.g.device) for n in (nf, nb))
    rec = c.record(0xABCDEF)
    eager, egrads = c.fw(narrow, rec, ws=wf, nbytes=nf), c.bw(narrow, rec, cot, ws=wb, nbytes=nb)
    torch.cuda.synchronize()
    outs, grads = c.outputs(), c.grads()
    side = torch.cuda.Stream()
    cg = torch.cuda.CUDAGraph()
    # No graph handle may be destroyed while a stream of the process is being captured (gnx_graphs_destroy frees device memory, which
    # invalidates the capture), and torch.cuda.graph does not collect garbage on entry: a dead reference cycle of an EARLIER test that
    # holds a handle would otherwise be collected at some allocation between the two calls below.  Collect now, and keep the collector off meanwhile.
    gc.collect()
    gc.disable()
    try:
        with torch.cuda.stream(side):
            with torch.cuda.graph(cg, stream=side):
                c.fw(narrow, c.record(0xABCDEF), outs=outs, ws=wf, stream=side.cuda_stream, nbytes=nf)
                c.bw(narrow, c.record(0xABCDEF), cot, outs=grads, ws=wb, stream=side.cuda_stream, nbytes=nb)
    finally:
        gc.enable()
    for t in list(outs) + list(grads.values()):
        t.zero_()
    cg.replay()
    torch.cuda.synchronize()
    for u, v in zip(eager, outs):
        assert torch.equal(_bits(u), _bits(v))
    for n in egrads:
        assert torch.equal(_bits(egrads[n]), _bits(grads[n])), n


# ---- 9. Python ----
def _py_case(gn, rng, narrow, case=((10, 5, 3), [16, 8, 3], [8, 4], [6, 5])):
    import torch
    adjs, R = _batch("five", rng)
    p = O.make_chain_block_params(rng, *case)
    c = DR.TrainCall(gn, adjs, p, DR.drop_after_hidden(p), R)
    c.blk.chain_dropout = True
    c.blk.narrow_chain = c.blk.narrow_chain_backward = bool(narrow)
    x = [None if t is None else t.permute(2, 1, 0).clone().requires_grad_(True) for t in c.xt]  # (d, T, R): the layout of the features
    return c, gn.NT(c.g, *x), x


@pytest.mark.parametrize("narrow", (0, 1))
def test_python_switch_gives_the_entries_bits(gn, narrow):
    import torch
    c, nt, x = _py_case(gn, np.random.default_rng(90), narrow)
    torch.manual_seed(5)
    y = c.blk(nt)
    rec = c.blk.last_chain_dropout
    assert rec.p == c.record(0).p
    want = c.fw(narrow, rec)
    cot = c.cotangents(5)
    wgrads = c.bw(narrow, rec, cot)
    loss = sum((o * g.permute(2, 1, 0)).sum() for o, g in zip((y.ef, y.nf, y.gf), cot))
    loss.backward()
    torch.cuda.synchronize()
    for got, w in zip((y.ef, y.nf, y.gf), want):
        assert torch.equal(_bits(got.detach().permute(2, 1, 0)), _bits(w))
    for t, n in zip(x, ("d_ef", "d_nf", "d_gf")):
        assert torch.equal(_bits(t.grad.permute(2, 1, 0)), _bits(wgrads[n])), n
    # the masks through the Python helper are the entry's: layer 1 of the edge function is its first Dropout
    m = gn.chain_dropout_mask(rec, 0, 1, (16, c.g.n_edges, c.R))
    assert np.array_equal(m.permute(2, 1, 0).cpu().numpy(), c.masks(rec)["edge"][1])
    # two calls draw different masks; torch.manual_seed reproduces a call's
    with torch.no_grad():
        gn.trainmode(c.blk)
        a = c.blk(nt); s1 = c.blk.last_chain_dropout.seed
        b = c.blk(nt); s2 = c.blk.last_chain_dropout.seed
        torch.manual_seed(5)
        again = c.blk(nt)
        gn.trainmode(c.blk, None)
    assert s1 != s2 and not torch.equal(a.ef, b.ef)
    assert c.blk.last_chain_dropout.seed == rec.seed and torch.equal(_bits(again.ef), _bits(y.ef.detach()))
    # testmode: the test-mode bits inside a gradient call, no NotImplementedError
    gn.testmode(c.blk)
    t = c.blk(nt)
    base, _ = c.fw_stripped(bool(narrow))
    torch.cuda.synchronize()
    assert t.ef.requires_grad
    for got, w in zip((t.ef, t.nf, t.gf), base):
        assert torch.equal(_bits(got.detach().permute(2, 1, 0)), _bits(w))
    gn.testmode(c.blk, None)
    # the switch off: today's refusal
    c.blk.chain_dropout = False
    with pytest.raises(NotImplementedError):
        c.blk(nt)


def _random_drop_block(rng):
    """tests/test_gpu_chain_narrow's random narrow blocks, some with a 40-wide function (a mixed mask), a Dropout behind random layers"""
    case = CN._random_block(rng)
    in_dims, ew, nw, gw, acts = case
    if rng.random() < 0.3 and gw and not isinstance(gw[0], str):
        gw = [40] + list(gw[1:]) if len(gw) > 1 else gw
    p = O.make_chain_block_params(rng, in_dims, ew, nw, gw, acts=acts)
    drops = {name: {} for name in DR.FN}
    for name in DR.FN:
        for i in range(len(p[name])):
            if rng.random() < 0.5 and len(p[name]) + len(drops[name]) < 16:
                drops[name][i] = float(rng.choice([0.1, 0.25, 0.5]))
    return p, drops


@pytest.mark.parametrize("seed", range(10 + EXTRA))
def test_seeded_sweep(gn, seed):
    """random narrow and mixed blocks, random Dropouts: both forward paths against float64 under the call's masks"""
    import torch
    rng = np.random.default_rng(7100 + seed)
    p, drops = _random_drop_block(rng)
    adjs, R = _batch("five" if seed % 4 else "replicas-2", rng)
    c = DR.TrainCall(gn, adjs, p, drops, R, seed=seed)
    fw, bw = _want_masks(c)
    assert (c.applies(0), c.applies(1)) == (fw, bw)
    rec = c.record(31 * seed + 1)
    ref, scale, _, _ = c.reference(c.masks(rec))
    for narrow in (0, 1):
        got = c.fw(narrow, rec)
        torch.cuda.synchronize()
        for name, o, r, s in zip(("ef", "nf", "gf"), got, ref, scale):
            U.assert_close(None if o is None else o.cpu().numpy(), r, s, f"sweep {seed} narrow={narrow} {name}")
