"""4-byte aligned buffers on every dispatch form of the C ABI (include/gnx.h: "Alignment"), on the GPU.

tests/test_gpu_memory_contract.py hands the library 256-byte aligned buffers only, and so does every other module (torch's allocator).  Below
that the library takes other kernel forms: the host-side predicates of csrc/ (counted by tests/test_arena_cpu.py::
test_every_pointer_alignment_branch_is_counted) test the caller's pointers for 16 bytes and choose a loader, an epilogue or a whole launch
sequence by the answer.  This module runs the contract module's case table again with the arena's carves at 256 k + 4 / + 8 / + 12 bytes
(tests/arena.py: `skew`), under four kinds of policy:

    mix            every buffer that is not a workspace at 4 (1 + crc32(name) % 3) bytes: operands misaligned differently from one another
    features+4     feature inputs and outputs, upstream and input gradients at + 4; parameters aligned
    params+4       weights, biases, LayerNorm gamma / beta and parameter-gradient outputs at + 4; features aligned
    one(<group>)   one operand group at + 4 and everything else aligned: the forms in between (everything skewed drops every plan straight to
                   its most generic form)

A (case, policy) run lays the case's arena out under the policy, calls the case once with a 0xFF workspace and asserts (1) status 0 — a public
entry point never refuses a 4-byte aligned fp32 / bf16 buffer —, (2) the arena check: nothing outside outputs and workspaces changed, every
output element written, (3) the case's own float64-oracle check at the bars it already uses, and (4), for the cases of BITWISE (no summation
order depends on an address), that the output bytes equal those of the same case laid out aligned.  Workspaces stay 16-byte aligned (the ABI
asks that) except in test_a_misaligned_workspace_is_refused.  The last part calls the Python mirror on views into the middle of a tensor."""
import ctypes as C
import fnmatch
import re
import zlib

import numpy as np
import pytest
import torch

from oracle import gn_oracle as O
from tests import arena as AR
from tests import test_gpu_memory_contract as MC
from tests import util as U
from tests.test_gpu_memory_contract import CASES, EXPECT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gn():
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return gn


# ---------------------------------------------------------------------------------------------------------------------------------------
# carve names -> operand classes (the systematic names of the contract module's cases)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _is_param(c):
    return c.name.startswith(("blk.", "core.", "chain."))


def _is_param_grad(c):
    return c.name.startswith("grad.")


def _is_feature(c):
    """feature inputs and outputs, forward outputs handed to a backward, upstream gradients, input gradients, and the operands of the small entry
    points (logits, masks, padded grids, ...): every carve that is neither a workspace nor a parameter nor a parameter gradient"""
    return c.kind != AR.WORKSPACE and not _is_param(c) and not _is_param_grad(c)


def _leaf(c):
    return c.name.rsplit(".", 1)[-1]


_named = lambda rx: (lambda c, rx=re.compile(rx): c.kind != AR.WORKSPACE and bool(rx.search(c.name)))
GROUPS = {
    "in:ef": lambda c: c.kind == AR.INPUT and _is_feature(c) and _leaf(c) == "ef",
    "in:nf": lambda c: c.kind == AR.INPUT and _is_feature(c) and _leaf(c) == "nf",
    "in:gf": lambda c: c.kind == AR.INPUT and _is_feature(c) and _leaf(c) == "gf",
    "out:ef": lambda c: _is_feature(c) and _leaf(c) == "ef_out",   # (an output of a forward, the stored forward output of a backward)
    "out:nf": lambda c: _is_feature(c) and _leaf(c) == "nf_out",
    "out:gf": lambda c: _is_feature(c) and _leaf(c) == "gf_out",
    "block.W": _named(r"^(core\.)?blk\.\w+\.W$"),
    "block.b": _named(r"^(core\.)?blk\.\w+\.b$"),
    "ln1": _named(r"^core\.ln1_"),
    "ln2": _named(r"^core\.ln2_"),
    "ff.W": _named(r"^core\.ff_\w\.fc\d\.W$"),
    "ff.b": _named(r"^core\.ff_\w\.fc\d\.b$"),
    "upstream": _named(r"^g_(ef|nf|gf)_out$"),
    "input-grads": _named(r"^d_(ef|nf|gf)$"),
    "param-grads": _named(r"^grad\."),
}


class Policy:
    def __init__(self, name, skew, must_move=None):
        self.name, self.skew, self.must_move = name, skew, must_move

    def __repr__(self):
        return self.name


def _mix(c):
    return 0 if c.kind == AR.WORKSPACE else 4 * (1 + zlib.crc32(c.name.encode()) % 3)


MIX = Policy("mix", _mix)
FEATURES4 = Policy("features+4", lambda c: 4 if _is_feature(c) else 0)
PARAMS4 = Policy("params+4", lambda c: 4 if c.kind != AR.WORKSPACE and (_is_param(c) or _is_param_grad(c)) else 0)
ONE = {k: Policy(f"one({k})", (lambda c, f=f: 4 if f(c) else 0), must_move=f) for k, f in GROUPS.items()}
ALIGNED = Policy("aligned", None)


# ---------------------------------------------------------------------------------------------------------------------------------------
# which case runs under which policy
# ---------------------------------------------------------------------------------------------------------------------------------------
# the alignment-sensitive subset: every id whose path holds one of the pointer-alignment predicates of csrc/
SENSITIVE = ["block/wide/*", "block/wide-odd*", "block/encoder*", "block/mid-widths*", "block/deferred/wide", "block/steps/mid-widths",
             "core/wide/*", "core/width-64*", "core/mid*", "core-train/*", "chain/forward/wide/*", "chain/backward/big",
             "block-backward/big/*", "core-backward/big*", "row-stats/*", "dropout-mask/*", "fn-input/wide*", "bf16/*"]

_FWD = ["in:ef", "in:nf", "in:gf", "out:ef", "out:nf", "out:gf"]
_CORE_P = ["block.W", "block.b", "ln1", "ln2", "ff.W", "ff.b"]
_BW = ["upstream", "input-grads", "param-grads"]
ANCHORS = {
    "block/wide/default": _FWD + ["block.W", "block.b"],
    "block/encoder(10,5,0)=>(128,64,32)": ["in:ef", "in:nf", "out:ef", "out:nf", "out:gf", "block.W", "block.b"],
    "core/wide/default": _FWD + _CORE_P,
    "core/wide/4099-nodes": _FWD + _CORE_P,
    "block-backward/big/wide": _FWD + ["block.W", "block.b"] + _BW,
    "core-backward/big(64,32,16)/gelu": ["in:ef", "in:nf", "in:gf"] + _CORE_P + _BW,
}

# The cases whose output BYTES do not depend on where their buffers lie: (pattern, policies it holds under; None = all of them).  These are the
# kernels without an alignment-dependent summation order: the fused narrow kernel in its pack / chained / steps / run forms, the generic
# kernels, the narrow core, the copy-like small entry points, and the bf16 forms (their contract is bitwise; the staging copies of the
# fallbacks lie in the aligned workspace, so moving the features cannot change a sum).
_ALL = None
_NATIVE_BF16 = ["bf16/readme/one-graph/R3", "bf16/readme/small-graphs", "bf16/jit-odd/medium", "bf16/steps/readme/one-graph",
                "bf16/steps/jit-odd/small-graphs"]  # the cases whose EXPECT row forbids the widen / round kernels, and their small-graph twins
BITWISE = [
    ("block/readme*", _ALL), ("block/jit*", _ALL), ("block/nothing/*", _ALL), ("block/chained/*", _ALL), ("block/steps/*", _ALL),
    ("*/FORCE_GENERIC*", _ALL), ("*/NO_JIT*", _ALL), ("*/NO_MFMA*", _ALL),
    ("core/narrow*", _ALL),
    ("row-stats/*", _ALL),  # include/gnx.h: gnx_row_stats gives the same bits at any alignment (k_ln_stats_v4<Q, false>: the same sums, dword loads)
    ("pad/*", _ALL), ("collapse/*", _ALL), ("xent/*", _ALL), ("dropout-mask/*", _ALL), ("fn-input/*", _ALL),
    ("bf16/*", {"features+4"}),
] + [(cid, _ALL) for cid in _NATIVE_BF16]
# ids taken out of BITWISE again: id -> the branch that changes the order of a sum with the address
NOT_BITWISE = {
    "block/steps/mid-widths": "widths from 32 run k_rows_gemm: launch_gemm's g.vec / out_vec choose the loader class and the epilogue by address",
}


def is_bitwise(cid, policy):
    if cid in NOT_BITWISE:
        return False
    return any(fnmatch.fnmatchcase(cid, pat) and (pols is None or policy.name in pols) for pat, pols in BITWISE)


def _sensitive(cid):
    return any(fnmatch.fnmatchcase(cid, pat) for pat in SENSITIVE)


def _pairs():
    out = []
    for cid in CASES:  # case-major: the policies of a case run back to back and share its setup and its oracle (_case)
        out.append((cid, MIX))
        if _sensitive(cid):
            out += [(cid, FEATURES4), (cid, PARAMS4)]
    return out


PAIRS = _pairs()
ONE_PAIRS = [(cid, ONE[k]) for cid, groups in ANCHORS.items() for k in groups]


def test_the_tables_name_cases_that_exist():
    assert set(ANCHORS) <= set(CASES) and set(_NATIVE_BF16) <= set(CASES) and set(NOT_BITWISE) <= set(CASES)
    for pat in SENSITIVE + [p for p, _ in BITWISE]:
        assert any(fnmatch.fnmatchcase(cid, pat) for cid in CASES), pat
    for cid in NOT_BITWISE:  # (an exception that excepts nothing is stale)
        assert any(fnmatch.fnmatchcase(cid, pat) for pat, _ in BITWISE), cid
    for cid in CASES:
        if cid.startswith("bf16/"):
            assert is_bitwise(cid, FEATURES4), cid
    for cid in _NATIVE_BF16:
        assert cid not in EXPECT or EXPECT[cid][1] >= {"k_bf16_widen", "k_bf16_round"}, cid
    assert not any(is_bitwise(cid, p) for cid, p in ONE_PAIRS)


# ---------------------------------------------------------------------------------------------------------------------------------------
# one (case, policy) run
# ---------------------------------------------------------------------------------------------------------------------------------------
_STATE = {}  # the case set up last: its arena, run, verify (the oracle is memoised inside) and the output bytes of its aligned run


def _case(gn, cid):
    if _STATE.get("cid") != cid:
        _STATE.clear()
        a = AR.Arena("cuda")
        run, verify = CASES[cid](gn, a)
        _STATE.update(cid=cid, a=a, run=run, verify=verify, aligned=None)
    return _STATE


def _layout(a, policy, ws_fill=0xFF):
    if a.buf is None:
        a.skew = policy.skew
        return a.build(ws_fill=ws_fill)
    return a.relayout(policy.skew, ws_fill=ws_fill)


def _call(gn, st, policy):
    """lay the arena out under `policy`, call the case once on a 0xFF workspace; -> status"""
    a = st["a"]
    _layout(a, policy)
    for c in a.carves:
        k = a.ptr(c.name) % AR.ALIGN
        assert k == (policy.skew(c) if policy.skew else 0) and (c.kind != AR.WORKSPACE or k == 0), (c.name, k)
    torch.cuda.synchronize()
    rc = st["run"](a)
    torch.cuda.synchronize()
    return rc


def run_pair(gn, cid, policy):
    lib = MC._L(gn).load()
    st = _case(gn, cid)
    a = st["a"]
    bitwise = is_bitwise(cid, policy)
    if bitwise and st["aligned"] is None:
        rc = _call(gn, st, ALIGNED)
        assert rc == 0, f"{cid} [aligned]: status {rc}: {lib.gnx_last_error()}"
        a.check(f"{cid} [aligned]")
        st["aligned"] = a.output_bits()
    what = f"{cid} [{policy.name}]"
    rc = _call(gn, st, policy)
    if policy.must_move is not None:  # a one(...) group that names no buffer of the case would test nothing
        moved = [c.name for c in a.carves if c.nbytes and a.ptr(c.name) % 16]
        assert moved and all(policy.must_move(a.by_name[n]) for n in moved), (what, moved)
    assert rc == 0, f"{what}: status {rc}: {lib.gnx_last_error()}"
    a.check(what)
    st["verify"](a, what)
    if bitwise:
        got = a.output_bits()
        for k, ref in st["aligned"].items():
            if not torch.equal(got[k], ref):
                d = (got[k] != ref).nonzero().view(-1)
                raise AssertionError(f"{what}: output '{k}' depends on the alignment of the buffers: {int(d.numel())} bytes differ from the aligned "
                                     f"run, first at byte {int(d[0])}, last at {int(d[-1])}")


@pytest.mark.parametrize("cid,policy", PAIRS, ids=[f"{c}-{p.name}" for c, p in PAIRS])
def test_alignment(gn, cid, policy):
    run_pair(gn, cid, policy)


@pytest.mark.parametrize("cid,policy", ONE_PAIRS, ids=[f"{c}-{p.name}" for c, p in ONE_PAIRS])
def test_one_operand_group_misaligned(gn, cid, policy):
    run_pair(gn, cid, policy)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the workspace is the one buffer that needs 16 bytes: + 4 and + 8 are refused before anything is written
# ---------------------------------------------------------------------------------------------------------------------------------------
WORKSPACE_FAMILIES = {
    "block forward": "block/readme/small-graphs(pack)",
    "typed forward": "bf16/readme/small-graphs",
    "steps": "block/steps/small-graphs",
    "core forward": "core/narrow(10,5,3)/medium",
    "core train": "core-train/narrow(10,5,3)",
    "chain forward": "chain/forward/layernorm",
    "block backward": "block-backward/small/readme",
    "core backward": "core-backward/small(10,5,3)",
    "core train backward": "core-train/backward/narrow",
    "chain backward": "chain/backward/small/layernorm",
}


@pytest.mark.parametrize("shift", [4, 8])
@pytest.mark.parametrize("family", list(WORKSPACE_FAMILIES))
def test_a_misaligned_workspace_is_refused(gn, family, shift):
    """Every workspace carve of the case starts `shift` bytes behind a 256-byte boundary and keeps the size its query gave, so the pointer and
    the whole workspace lie inside the carve and the alignment is the only thing to refuse (a size reduced by `shift` would be refused for its
    size).  GNX_ERR_WORKSPACE, and not a byte of the arena changes: guards, inputs, the 0xFF of the outputs, the 0xFF of the workspaces."""
    L, lib = MC._L(gn), MC._L(gn).load()
    cid = WORKSPACE_FAMILIES[family]
    st = _case(gn, cid)
    a = st["a"]
    _layout(a, Policy(f"workspace+{shift}", lambda c: shift if c.kind == AR.WORKSPACE else 0))
    wss = [c for c in a.carves if c.kind == AR.WORKSPACE]
    assert wss and all(c.nbytes > 0 and a.ptr(c.name) % 16 == shift for c in wss)
    torch.cuda.synchronize()
    rc = st["run"](a)
    torch.cuda.synchronize()
    assert rc == L.ERR_WORKSPACE, f"{cid} [workspace+{shift}]: status {rc}: {lib.gnx_last_error()}"
    assert b"16-byte aligned" in lib.gnx_last_error(), lib.gnx_last_error()
    assert a.violations(unwritten=False) == []
    for c in a.carves:
        if c.nbytes and c.kind != AR.INPUT:
            assert bool((a.raw(c.name) == AR.UNWRITTEN).all()), f"{cid}: {c.kind} '{c.name}' was written by a refused call"


# ---------------------------------------------------------------------------------------------------------------------------------------
# the Python mirror: views into the middle of a tensor go to the library as they are (api.py passes a contiguous view through)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _graph(gn, N, E, seed):
    return MC._from_csc(gn, [U.er_csc(np.random.default_rng(seed), N, E)])


def _replica_views(packed, r, dev, dtype=None):
    """(Julia-shaped views of replica r inside the packed [R][T][D] device tensors, the packed numpy replica)"""
    views, xs = [], []
    for x in packed:
        if x is None:
            views.append(None); xs.append(None)
            continue
        t = torch.from_numpy(x).to(dev)
        t = t if dtype is None else t.to(dtype)
        v = t[r:r + 1]
        assert v.is_contiguous() and v.data_ptr() % 4 == 0 and v.data_ptr() % 16 != 0, (x.shape, v.data_ptr() % 16)
        views.append(v.permute(2, 1, 0)); xs.append(v.float().cpu().numpy())
    return views, xs


def _offset_views(packed, dev):
    """the packed [1][T][D] tensors as views that start one float into a buffer one float longer.  (Dropping the first ROW of these tensors
    keeps 16 bytes: their rows are 128, 64 and 32 floats.)"""
    views = []
    for x in packed:
        buf = torch.empty(x.size + 1, dtype=torch.float32, device=dev)
        buf[1:] = torch.from_numpy(x.reshape(-1)).to(dev)
        v = buf[1:].view(x.shape)
        assert v.is_contiguous() and v.data_ptr() % 4 == 0 and v.data_ptr() % 16 != 0, (x.shape, v.data_ptr() % 16)
        views.append(v.permute(2, 1, 0))
    return views


def _same_bits(y, z, what):
    for n in ("ef", "nf", "gf"):
        a, b = getattr(y, n), getattr(z, n)
        assert (a is None) == (b is None), (what, n)
        if a is not None:
            bits = {torch.float32: torch.int32, torch.bfloat16: torch.int16}[a.dtype]  # (NaNs and signed zeros compare by their bytes)
            assert a.dtype == b.dtype and torch.equal(a.view(bits), b.view(bits)), f"{what}: {n} differs from the call on a copy"


def _clones(views):
    out = [None if v is None else v.permute(2, 1, 0).clone() for v in views]
    assert all(c is None or c.data_ptr() % 256 == 0 for c in out)
    return [None if c is None else c.permute(2, 1, 0) for c in out]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_mirror_block_on_a_replica_of_a_packed_batch(gn, bf16):
    """README widths, replica 1 of R = 3: E . 10 and N . 5 elements per replica put it at 4 (not 16) bytes — 7001 edges and 1001 nodes in fp32,
    1002 nodes in bf16 (1001 . 5 bf16 elements would be 2 bytes off, which the mirror copies)"""
    N = 1002 if bf16 else 1001
    g, csc = _graph(gn, N, 7001, 300)
    rng = np.random.default_rng(301)
    p = O.make_block_params(rng, (10, 5, 0), (3, 4, 5))
    blk = U.block_from_params(gn, p)
    packed = U.packed_inputs(rng, 3, g.n_edges, g.n_nodes, g.n_graphs, (10, 5, 0))
    views, xs = _replica_views(packed, 1, g.device, torch.bfloat16 if bf16 else None)
    y = blk(gn.NT(g, *views))
    z = blk(gn.NT(g, *_clones(views)))
    torch.cuda.synchronize()
    _same_bits(y, z, "GNBlock README widths" + (" bf16" if bf16 else ""))
    ref, scale = O.block_forward_sparse(p, csc, *xs, return_scale=True)
    if bf16:
        assert y.ef.dtype == torch.bfloat16
        for n, r, s in zip(("ef", "nf", "gf"), ref, scale):
            got = U.from_jl(getattr(y, n).float()).astype(np.float64)
            ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(r), 1e-30))) - 7)
            assert (np.abs(got - r) <= 0.5 * ulp + U.RTOL * s + 1e-30).all(), n  # MC._check_bf16_outputs's bound
    else:
        for n, r, s in zip(("ef", "nf", "gf"), ref, scale):
            U.assert_close(U.from_jl(getattr(y, n)), r, s, f"GNBlock on replica 1: {n}")


def test_mirror_wide_block_on_offset_views(gn):
    g, csc = _graph(gn, 601, 4099, 302)
    rng = np.random.default_rng(303)
    p = O.make_block_params(rng, (128, 64, 32), (128, 64, 32), act=(1, 1, 0))
    blk = U.block_from_params(gn, p)
    packed = U.packed_inputs(rng, 1, g.n_edges, g.n_nodes, g.n_graphs, (128, 64, 32))
    y = blk(gn.NT(g, *_offset_views(packed, g.device)))
    torch.cuda.synchronize()
    ref, scale = O.block_forward_sparse(p, csc, *packed, return_scale=True)
    for n, r, s in zip(("ef", "nf", "gf"), ref, scale):
        U.assert_close(U.from_jl(getattr(y, n)), r, s, f"wide GNBlock on offset views: {n}")


def test_mirror_core_on_offset_views(gn):
    g, csc = _graph(gn, 601, 4099, 304)
    rng = np.random.default_rng(305)
    p = O.make_core_params(rng, (128, 64, 32))
    core = U.core_from_params(gn, p)
    packed = U.packed_inputs(rng, 1, g.n_edges, g.n_nodes, g.n_graphs, (128, 64, 32))
    y = core(gn.NT(g, *_offset_views(packed, g.device)))
    torch.cuda.synchronize()
    ref, scale = O.core_forward_sparse(p, csc, *packed, return_scale=True)
    for n, r, s in zip(("ef", "nf", "gf"), ref, scale):
        U.assert_close(U.from_jl(getattr(y, n)), r, s, f"GNCore on offset views: {n}")
