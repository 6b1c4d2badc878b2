"""Which C entries a call of the Python binding reaches, and what they compute: for every combination of layer family (GNBlock with Dense update
functions, GNBlock with Chain update functions, GNCore), element type, switch and Dropout record that graphnets.jl_amd/api.py tells apart,

  1. the ordered list of `gnx_*` symbols the call looks up on the library — forward query, forward call, then backward query, backward call,
     nothing else (gnx_last_error aside) — is the list written in ROWS below, and
  2. every output and every gradient (inputs and parameters) is bit for bit what the binding computed before its launchers, autograd nodes and
     entry ladders were folded into one per family: tests/golden/api_entries/parent.npz, recorded by this test on an MI355X with that commit's
     api.py (`GNX_RECORD_GOLDEN=1 pytest tests/test_gpu_api_entries.py` writes the file instead of asserting the bits; the lists are asserted
     either way).  A directory of its own, because tests/test_golden.py takes every .npz directly under tests/golden for an oracle vector.

All rows run on one tiny batch: a graph of 3 nodes and 4 edges whose node 0 has no in-edge, and a graph of 2 nodes and 1 edge; the two R = 2
rows on the first graph alone."""
import gc
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "api_entries", "parent.npz")
RECORD = os.environ.get("GNX_RECORD_GOLDEN") == "1"
F32, BF16 = torch.float32, torch.bfloat16

pytestmark = pytest.mark.gpu

ADJ_A = np.array([[0, 1, 1], [0, 0, 1], [0, 1, 0]], dtype=np.int64)  # A[i, j] = 1 <=> edge i -> j: 0->1, 0->2, 1->2, 2->1; nothing enters node 0
ADJ_B = np.array([[0, 1], [0, 0]], dtype=np.int64)


def _pair(call):
    """(query, call) of an entry whose query is `<call>_workspace_bytes`"""
    return [call + "_workspace_bytes", call]


ERR = "NotImplementedError"


def _row(id, family, dtype=F32, grad=True, sw=None, mode=None, dropout=0.0, R=1, fw=None, bw=None):
    """sw: the owner's switches; mode: "train" / "test" (trainmode / testmode) or None; fw / bw: the expected names; fw = ERR: the call raises"""
    want = ERR if fw == ERR else list(fw) + (list(bw) if grad else [])
    return pytest.param(dict(id=id, family=family, dtype=dtype, grad=grad, sw=sw or {}, mode=mode, dropout=dropout, R=R, want=want), id=id)


def _rows():
    rows = []
    # ---- GNBlock with Dense update functions, (2,2,2) => (2,2,2) ----
    fw = {F32: ["gnx_block_workspace_bytes", "gnx_block_forward"], BF16: ["gnx_block_typed_workspace_bytes", "gnx_block_forward_typed"]}
    bw = {(F32, "plain"): "gnx_block_backward", (F32, "fused_backward"): "gnx_block_backward_fused", (F32, "narrow_backward"): "gnx_block_backward_narrow",
          (BF16, "plain"): "gnx_block_backward_typed", (BF16, "fused_backward"): "gnx_block_backward_fused_typed",
          (BF16, "narrow_backward"): "gnx_block_backward_narrow"}
    for dt, tag in ((F32, "f32"), (BF16, "bf16")):
        for switch in ("plain", "fused_backward", "narrow_backward"):
            sw = {} if switch == "plain" else {switch: True}
            rows.append(_row(f"block-{tag}-{switch}-nograd", "block", dt, False, sw, fw=fw[dt]))
            rows.append(_row(f"block-{tag}-{switch}-grad", "block", dt, True, dict(sw, bf16_backward=dt == BF16), fw=fw[dt], bw=_pair(bw[(dt, switch)])))
    rows.append(_row("block-bf16-grad-without-bf16_backward", "block", BF16, True, {"bf16_backward": False}, fw=ERR))
    rows.append(_row("block-f32-both-narrow-wins-grad", "block", F32, True, {"fused_backward": True, "narrow_backward": True}, fw=fw[F32],
                     bw=_pair("gnx_block_backward_narrow")))
    rows.append(_row("block-f32-plain-grad-R2", "block", F32, True, {}, R=2, fw=fw[F32], bw=_pair("gnx_block_backward")))
    # ---- GNBlock with Chain update functions, no Dropout ----
    for nc in (0, 1):
        for ncb in (0, 1):
            rows.append(_row(f"chain-f32-narrow{nc}-bw_narrow{ncb}-grad", "chain", F32, True, {"narrow_chain": bool(nc), "narrow_chain_backward": bool(ncb)},
                             fw=_pair("gnx_chain_block_forward_narrow") if nc else ["gnx_chain_block_workspace_bytes", "gnx_chain_block_forward"],
                             bw=_pair("gnx_chain_block_backward_narrow" if ncb else "gnx_chain_block_backward")))
    for ncb, native in ((0, 0), (1, 0), (1, 1)):
        rows.append(_row(f"chain-bf16-bw_narrow{ncb}-native{native}-grad", "chain", BF16, True,
                         {"bf16_chain": True, "bf16_backward": True, "narrow_chain": bool(ncb), "narrow_chain_backward": bool(ncb), "native_chain_backward": bool(native)},
                         fw=_pair("gnx_chain_block_forward_typed"),
                         bw=_pair("gnx_chain_block_backward_narrow_typed" if native else "gnx_chain_block_backward_typed")))
    rows.append(_row("chain-bf16-without-bf16_chain", "chain", BF16, True, {"bf16_chain": False, "bf16_backward": True}, fw=ERR))
    # ---- GNBlock with Chain update functions, Dropout(0.5) behind the first Dense of the edge and the node function ----
    for n in (0, 1):
        rows.append(_row(f"chaindrop-f32-narrow{n}-grad", "chain", F32, True, {"chain_dropout": True, "narrow_chain": bool(n), "narrow_chain_backward": bool(n)},
                         dropout=0.5, fw=_pair("gnx_chain_block_forward_train"), bw=_pair("gnx_chain_block_backward_train")))
    rows.append(_row("chaindrop-f32-trainmode-nograd", "chain", F32, False, {"chain_dropout": True}, mode="train", dropout=0.5,
                     fw=_pair("gnx_chain_block_forward_train")))
    rows.append(_row("chaindrop-f32-testmode-nograd", "chain", F32, False, {"chain_dropout": True}, mode="test", dropout=0.5,
                     fw=["gnx_chain_block_workspace_bytes", "gnx_chain_block_forward"]))
    rows.append(_row("chaindrop-bf16-trainmode", "chain", BF16, False, {"chain_dropout": True, "bf16_chain": True, "bf16_backward": True}, mode="train",
                     dropout=0.5, fw=ERR))
    rows.append(_row("chaindrop-f32-grad-without-chain_dropout", "chain", F32, True, {"chain_dropout": False}, dropout=0.5, fw=ERR))
    # ---- GNCore, (4,3,2) ----
    cfw = {F32: ["gnx_core_workspace_bytes", "gnx_core_forward"], BF16: ["gnx_core_typed_workspace_bytes", "gnx_core_forward_typed"]}
    for dt, tag in ((F32, "f32"), (BF16, "bf16")):
        sw = {"bf16": True, "bf16_backward": True} if dt == BF16 else {}
        rows.append(_row(f"core-{tag}-nograd", "core", dt, False, sw, fw=cfw[dt]))
        for nb in (0, 1):
            call = "gnx_core_backward_narrow" if nb else ("gnx_core_backward_typed" if dt == BF16 else "gnx_core_backward")
            rows.append(_row(f"core-{tag}-bw_narrow{nb}-grad", "core", dt, True, dict(sw, narrow_backward=bool(nb)), fw=cfw[dt], bw=_pair(call)))
    train = ["gnx_core_train_workspace_bytes", "gnx_core_forward_train"]
    rows.append(_row("coredrop-f32-plain-grad", "core", F32, True, {}, dropout=0.25, fw=train, bw=["gnx_core_backward_workspace_bytes", "gnx_core_backward_train"]))
    rows.append(_row("coredrop-f32-bw_narrow-grad", "core", F32, True, {"narrow_backward": True}, dropout=0.25, fw=train, bw=_pair("gnx_core_backward_narrow")))
    for dt, tag in ((F32, "f32"), (BF16, "bf16")):
        for nb in (0, 1):
            rows.append(_row(f"coredrop-{tag}-typed_dropout-bw_narrow{nb}-grad", "core", dt, True,
                             {"bf16": True, "bf16_backward": True, "typed_dropout": True, "narrow_backward": bool(nb)}, dropout=0.25,
                             fw=["gnx_core_train_typed_workspace_bytes", "gnx_core_forward_train_typed"], bw=_pair("gnx_core_backward_train_typed")))
    rows.append(_row("coredrop-bf16-without-typed_dropout", "core", BF16, True, {"bf16": True, "bf16_backward": True}, dropout=0.25, fw=ERR))
    rows.append(_row("core-f32-plain-grad-R2", "core", F32, True, {}, R=2, fw=cfw[F32], bw=_pair("gnx_core_backward")))
    return rows


class _Proxy:
    """the loaded library, with every looked-up `gnx_*` name appended to `log`"""

    def __init__(self, lib, log):
        self.__dict__["_lib"], self.__dict__["_log"] = lib, log

    def __getattr__(self, name):
        if name.startswith("gnx_"):
            self._log.append(name)
        return getattr(self._lib, name)


@pytest.fixture(scope="module")
def gn():
    import graphnets_jl_amd as gn
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    gn._lib.load()  # (once beforehand: the wrapper below only proxies)
    return gn


@pytest.fixture(scope="module")
def graphs(gn):
    """the two batches' graph handles, alive for the whole module: a handle's destructor is a library call.  Handles that other test modules left
    in reference cycles are destroyed here, before the first row looks at the calls."""
    gc.collect()
    return {1: gn.GNGraphBatch([ADJ_A, ADJ_B]), 2: gn.GNGraphBatch([ADJ_A])}


@pytest.fixture(scope="module")
def golden():
    """the recorded arrays; in a recording run: the dict the rows fill, written when the module is done"""
    if not RECORD:
        yield np.load(GOLDEN)
        return
    rec = {}
    yield rec
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **rec)


def _features(gn, g, dims, R, dtype, gen):
    """the batched tuple of the row: R = 1 on the two graphs, R = 2 replicas on the first graph alone (one adjacency shared by the data batch)"""
    if R == 1:
        E, N = (4, 1), (3, 2)
        t = gn.NT(g, [torch.rand((dims[0], e), generator=gen) - 0.5 for e in E], [torch.rand((dims[1], n), generator=gen) - 0.5 for n in N],
                  [torch.rand((dims[2],), generator=gen) - 0.5 for _ in E])
    else:
        t = gn.NT(g, torch.rand((dims[0], 4, R), generator=gen) - 0.5, torch.rand((dims[1], 3, R), generator=gen) - 0.5, torch.rand((dims[2], R), generator=gen) - 0.5)
    return gn.batch(t, dtype=dtype)


def _fill(gen, *layers):
    """non-zero biases / LayerNorm scales and shifts (the constructors make zeros and ones); returns the parameter tensors in the layers' order"""
    out = []
    for l in layers:
        if hasattr(l, "gamma"):
            l.gamma = (1 + 0.5 * (torch.rand(l.gamma.shape, generator=gen) - 0.5)).to(l.gamma.device)
            l.beta = (torch.rand(l.beta.shape, generator=gen) - 0.5).to(l.beta.device)
            out += [l.gamma, l.beta]
        else:
            l.bias = (torch.rand(l.bias.shape, generator=gen) - 0.5).to(l.bias.device)
            out += [l.weight, l.bias]
    return out


def _model(gn, row, gen):
    """(layer, its parameter tensors, its input widths)"""
    sw, p = row["sw"], row["dropout"]
    D = lambda i, o, act="identity": gn.Dense(i, o, act, None, gen)
    if row["family"] == "block":
        m = gn.GNBlock((2, 2, 2), (2, 2, 2), generator=gen, **sw)
        return m, _fill(gen, m.edgefn, m.nodefn, m.graphfn), (2, 2, 2)
    if row["family"] == "chain":
        m = gn.GNBlock((2, 2, 2), (3, 2, 2), generator=gen, **sw)
        drop = [gn.Dropout(p)] if p > 0 else []
        m.edgefn = gn.Chain(D(8, 4, "relu"), *drop, gn.LayerNorm(4), D(4, 3))
        m.nodefn = gn.Chain(D(7, 4, "relu"), *drop, D(4, 2))
        m.graphfn = gn.Chain(D(7, 2))
        return m, _fill(gen, *(l for ch in (m.edgefn, m.nodefn, m.graphfn) for l in ch.layers)), (2, 2, 2)
    m = gn.GNCore((4, 3, 2), dropout=p, generator=gen, **sw)
    lns = [ln for gnorm in (m.gn1, m.gn2) for ln in (gnorm.edgeln, gnorm.nodeln, gnorm.graphln)]
    _fill(gen, m.block.edgefn, m.block.nodefn, m.block.graphfn, *lns, *(d for ff in (m.ffwd.eff, m.ffwd.nff, m.ffwd.gff) for d in ff))
    return m, m._param_list(), (4, 3, 2)


def _cotangent(o):
    """a fixed, non-uniform cotangent of the shape of `o`: multiples of 1/4 (exact in bfloat16)"""
    w = ((torch.arange(o.numel(), device=o.device) % 7) - 2).to(torch.float32) / 4
    return w.reshape(o.shape).to(o.dtype)


def _bits(t):
    """the bits of a float32 / bfloat16 tensor as a uint32 / uint16 numpy array"""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int32).numpy().view(np.uint32) if t.dtype == F32 else t.view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("row", _rows())
def test_the_call_reaches_the_tables_entries_and_keeps_the_parents_bits(gn, graphs, golden, monkeypatch, request, row):
    gen = torch.Generator().manual_seed(20240 + row["R"])  # (seeded once per row: a row's weights and features do not depend on which rows ran before)
    m, params, dims = _model(gn, row, gen)
    x = _features(gn, graphs[row["R"]], dims, row["R"], row["dtype"], gen)
    feats = [a.detach().clone() for a in (x.ef, x.nf, x.gf)]
    if row["grad"]:
        for t in feats + params:
            t.requires_grad_(True)
    if row["mode"] is not None:
        (gn.trainmode if row["mode"] == "train" else gn.testmode)(m)
    xin = gn.NT(x.graphs, *feats)
    torch.cuda.synchronize()

    log = []
    lib = gn._lib.load()
    gc.disable()  # (no destructor of somebody else's handle inside the window: see `graphs`)
    request.addfinalizer(gc.enable)
    monkeypatch.setattr(gn._lib, "load", lambda: _Proxy(lib, log))
    torch.manual_seed(0)
    if row["want"] == ERR:
        with pytest.raises(NotImplementedError):
            with torch.enable_grad() if row["grad"] else torch.no_grad():
                m(xin)
        assert log == [], log
        return
    with torch.enable_grad() if row["grad"] else torch.no_grad():
        y = m(xin)
        outs = [y.ef, y.nf, y.gf]
        if row["grad"]:
            torch.autograd.backward(outs, [_cotangent(o) for o in outs])
    torch.cuda.synchronize()
    monkeypatch.undo()

    names = [n for n in log if n != "gnx_last_error"]
    assert names == row["want"], f"{row['id']}: looked up {names}, the table says {row['want']}"

    got = {f"out_{n}": _bits(o) for n, o in zip(("ef", "nf", "gf"), outs)}
    if row["grad"]:
        for n, t in zip(("ef", "nf", "gf"), feats):
            assert t.grad is not None and t.grad.dtype == row["dtype"] and t.grad.shape == t.shape, n
            got[f"d_{n}"] = _bits(t.grad)
        for i, t in enumerate(params):
            assert t.grad is not None and t.grad.dtype == F32 and t.grad.shape == t.shape, f"parameter {i}"
            got[f"g{i:02d}"] = _bits(t.grad)
    if RECORD:
        golden.update({f"{row['id']}/{k}": v for k, v in got.items()})
        return
    prefix = row["id"] + "/"
    assert sorted(k[len(prefix):] for k in golden.files if k.startswith(prefix)) == sorted(got), f"{row['id']}: the recorded arrays are another set"
    for k, v in got.items():
        w = golden[prefix + k]
        assert v.dtype == w.dtype and v.shape == w.shape, f"{row['id']}/{k}: {v.dtype} {v.shape} against the recorded {w.dtype} {w.shape}"
        d = int((v != w).sum())
        assert d == 0, f"{row['id']}/{k}: {d} of {w.size} values differ from the parent commit's bits"
