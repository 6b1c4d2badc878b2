"""The one place the tools build a checked C call from.  A case (block_case / core_case / chain_case) is an owner built from oracle.gn_oracle
parameters with its C parameter record and the seeded inputs and cotangents; build() turns (case, family, direction, element type, entry) into a
closure around ONE checked call of the library, with its workspace and the tensors it writes.  The argument list of the call is not spelled
here: it comes from the binding's own entry table (graphnets.jl_amd/api.py: _entry, _values) — head, tail, query and query_tail of the _Entry —
reached by a set of the owner's switches or by a C entry name of NAMED, the one table of which switches stand behind which name.

Seeds and draw order are the tools' (the diff and bit-identity fields of the committed records depend on them): default_rng(0); the owner's
parameters first, then the features — "pm2": random * 4 - 2 (the backward tools), "unit": plain random (the chain and forward tools) — then the
standard-normal cotangents.

Nothing of the package is imported at module level (tools/timing.py: child_root)."""
import collections
import ctypes as C
import types

import numpy as np

from tools.timing import ptr

FN = (("edge", "edgefn"), ("node", "nodefn"), ("graph", "graphfn"))
Call = collections.namedtuple("Call", "f nbytes outs grads ws entry keep")


def rows(g):
    return (g.n_edges, g.n_nodes, g.n_graphs)


def elem_dtype(gn, elem):
    import torch
    return torch.bfloat16 if elem == gn._lib.ELEM_BF16 else torch.float32


def draw(rng, kind, shape, dtype=None):
    """one seeded device tensor: kind "pm2", "unit" or "normal" """
    import torch
    a = rng.standard_normal(shape).astype(np.float32) if kind == "normal" else rng.random(shape, dtype=np.float32)
    t = torch.from_numpy(a * 4 - 2 if kind == "pm2" else a).cuda()
    return t if dtype is None else t.to(dtype)


def _case(g, owner, p, keep, widths, out_widths, rng, dtype, R, features, cot, **more):
    x = [draw(rng, features, (R, T, d), dtype) if d else None for T, d in zip(rows(g), widths)]
    c = [draw(rng, "normal", (R, T, d), dtype) if d else None for T, d in zip(rows(g), out_widths)] if cot else None
    return types.SimpleNamespace(g=g, owner=owner, p=p, keep=keep, widths=tuple(widths), out_widths=tuple(out_widths), x=x, cot=c, R=R, rng=rng, **more)


def block_case(gn, g, in_dims, out_dims, act=None, dtype=None, R=1, features="pm2", cot=True):
    """a GNBlock with Dense update functions of oracle parameters, its inputs and (cot) the cotangents of its three outputs"""
    from oracle import gn_oracle as O
    from tests import util as U
    rng = np.random.default_rng(0)
    blk = U.block_from_params(gn, O.make_block_params(rng, in_dims, out_dims, **({} if act is None else dict(act=act))))
    keep = []
    return _case(g, blk, blk._c(keep), keep, in_dims, out_dims, rng, dtype, R, features, cot)


def core_case(gn, g, dims, dtype=None, cot=True):
    from oracle import gn_oracle as O
    from tests import util as U
    rng = np.random.default_rng(0)
    core = U.core_from_params(gn, O.make_core_params(rng, dims))
    keep = []
    return _case(g, core, core._c(keep), keep, dims, dims, rng, dtype, 1, "pm2", cot)


def chain_case(gn, g, cfg, dtype=None, cot=True, make=None):
    """a GNBlock with Chain update functions of cfg = (in_dims, edge widths, node widths, graph widths); make(p, keep) -> (owner, C record, output
    widths) where the owner is not tests/test_gpu_chain.py's plain block"""
    from oracle import gn_oracle as O
    rng = np.random.default_rng(0)
    p = O.make_chain_block_params(rng, *cfg)
    keep = []
    if make is None:
        from tests.test_gpu_chain import _block
        owner = _block(gn, p)
        cp, _, outw = owner._chain_params(keep)
    else:
        owner, cp, outw = make(p, keep)
    return _case(g, owner, cp, keep, cfg[0], outw, rng, dtype, 1, "unit", cot, oracle=p)


def chain_params(gn, p, keep):
    """the gnx_chain_block_params of an oracle parameter dict, built without a GNBlock (LayerNorm's eps modes included); the weights go to the device"""
    import torch
    from oracle import gn_oracle as O
    L = gn._lib
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    q = L.ChainBlockParams()
    q.de, q.dn, q.dg = p["in_dims"]
    for name, field in FN:
        layers = p[name]
        arr, wid = (L.Dense * max(len(layers), 1))(), (C.c_int32 * max(len(layers), 1))()
        for i, (w, b, c) in enumerate(layers):
            ln = isinstance(w, str)
            W, B = (dev(b), dev(c)) if ln else (dev(np.asarray(w).T), dev(b))
            kind = 0 if not ln else (L.LAYER_LAYERNORM | L.LAYER_LN_SQRT_EPS if O.ln_eps_mode(w) == 1 else L.LAYER_LAYERNORM)
            arr[i] = L.Dense(ptr(W), ptr(B), 0 if ln else int(c), kind)
            wid[i] = len(b) if ln else w.shape[0]
            keep += [W, B]
        keep += [arr, wid]
        ch = getattr(q, field)
        ch.layers, ch.widths, ch.n_layers = arr, wid, len(layers)
    return q


def given_case(g, p, keep, x, cot, out_widths, R=1, owner=None, oracle=None):
    """a case around inputs that exist already (tests/chain_bw_cases.py's data)"""
    return types.SimpleNamespace(g=g, owner=owner, p=p, keep=keep, widths=None, out_widths=tuple(out_widths), x=list(x), cot=None if cot is None else list(cot),
                                 R=R, rng=None, oracle=oracle)


# C entry name -> the owner's switches under which the binding's table (api._entry) reaches it.  TYPED: entries that take either element code
# and that the binding reaches for bfloat16 alone — looked up under GNX_ELEM_BF16; the element code is the first value of their query_tail and head.
# A Dropout record (the *_train entries, gnx_core_backward_narrow under one) comes with the call: build(drop=...).
NAMED = {
    "gnx_block_forward": (), "gnx_block_forward_typed": (),
    "gnx_block_backward": (), "gnx_block_backward_fused": ("fused_backward",), "gnx_block_backward_typed": ("bf16_backward",),
    "gnx_block_backward_fused_typed": ("bf16_backward", "fused_backward"), "gnx_block_backward_narrow": ("bf16_backward", "narrow_backward"),
    "gnx_chain_block_forward": (), "gnx_chain_block_forward_narrow": ("narrow_chain",), "gnx_chain_block_forward_typed": ("bf16_chain",),
    "gnx_chain_block_forward_train": (),
    "gnx_chain_block_backward": (), "gnx_chain_block_backward_narrow": ("narrow_chain_backward",),
    "gnx_chain_block_backward_typed": ("bf16_chain", "bf16_backward"),
    "gnx_chain_block_backward_narrow_typed": ("bf16_chain", "bf16_backward", "native_chain_backward"), "gnx_chain_block_backward_train": (),
    "gnx_core_forward": (), "gnx_core_forward_typed": (), "gnx_core_forward_train": (), "gnx_core_forward_train_typed": ("typed_dropout",),
    "gnx_core_backward": (), "gnx_core_backward_train": (), "gnx_core_backward_typed": ("bf16_backward",),
    "gnx_core_backward_narrow": ("bf16_backward", "narrow_backward"),
}
TYPED = ("gnx_block_forward_typed", "gnx_block_backward_typed", "gnx_block_backward_fused_typed", "gnx_chain_block_forward_typed",
         "gnx_chain_block_backward_typed", "gnx_chain_block_backward_narrow_typed", "gnx_core_forward_typed", "gnx_core_backward_typed")
# the switch behind the `narrow` value that the typed and training Chain entries pass
NARROW = {("chain", "forward"): "narrow_chain", ("chain", "backward"): "narrow_chain_backward"}


def resolve(gn, family, direction, elem, entry, record=False, narrow=0):
    """the binding's _Entry of `entry`: a set of switch names (api._entry's `switches`) or a C entry name of NAMED; narrow = 1: with the
    direction's narrow switch of a Chain block on, so that the entry passes narrow = 1"""
    api, L = gn.api, gn._lib
    if not isinstance(entry, str):
        return api._entry(family, direction, elem, frozenset(entry) | ({NARROW[family, direction]} if narrow else set()), record)
    switches = frozenset(NAMED[entry]) | ({NARROW[family, direction]} if narrow else set())
    e = api._entry(family, direction, L.ELEM_BF16 if entry in TYPED else elem, switches, record)
    assert e.call == entry, (entry, e.call)
    if entry in TYPED and elem != L.ELEM_BF16:
        assert e.query_tail[0] == L.ELEM_BF16 and e.head[0] == L.ELEM_BF16
        e = e._replace(query_tail=(elem,) + e.query_tail[1:], head=(elem,) + e.head[1:])
    return e


def _poisoned(torch, shape, dtype, poison):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda") if poison else torch.empty(shape, dtype=dtype, device="cuda")


def grad_slots(gn, case, family, poison=False, layout=None):
    """(the gradient tensors in the family's order, the C record of their pointers, what keeps it alive).  block: dW, db per function; core:
    one per core.parameters(); chain: flat dW, db per layer — layout {function: [layer index or None per entry]} where an entry list with
    Dropout slots (None) stands behind the record (the training entries)"""
    import torch
    L = gn._lib
    new = lambda shape: _poisoned(torch, shape, torch.float32, poison)
    if family == "block":
        gs = [t for l in (case.owner.edgefn, case.owner.nodefn, case.owner.graphfn) for t in (new((l.weight.shape[1], l.weight.shape[0])), new(tuple(l.bias.shape)))]
        return gs, L.BlockGrads(*[L.DenseGrad(ptr(gs[2 * i]), ptr(gs[2 * i + 1])) for i in range(3)]), []
    if family == "core":
        gs = [new((q.shape[1], q.shape[0])).t() if q.dim() == 2 else new(tuple(q.shape)) for q in case.owner.parameters()]
        return gs, gn.api._core_grads(case.owner, gs), []
    gs, arrays = [], []
    for name, _ in FN:
        layers = case.oracle[name]
        slots = list(range(len(layers))) if layout is None else layout[name]
        arr = (L.DenseGrad * max(len(slots), 1))()
        for e, v in enumerate(slots):
            if v is None:
                continue
            w, b, c = layers[v]
            gw, gb = new((len(b) if isinstance(w, str) else w.size,)), new((len(c) if isinstance(w, str) else len(b),))
            gs += [gw, gb]
            arr[e] = L.DenseGrad(ptr(gw), ptr(gb))
        arrays.append(arr)
    return gs, L.ChainBlockGrads(*[C.cast(q, C.POINTER(L.DenseGrad)) for q in arrays]), arrays


def build(gn, case, family, direction, elem, entry=(), *, x=None, cot=None, fwd=None, outs=None, ws=None, drop=None, narrow=0, flags=0, p=None,
          want=(True, True, True), grads=True, layout=None, poison=False, query=None):
    """One checked call.  entry: a C entry name or a set of switches, narrow: resolve's; drop: the Dropout / ChainDropout C record of a training
    call; query: (name, values after (handle, params, R)) of another workspace query than the entry's own.
    x / cot / fwd (a block pullback's forward outputs) / outs / ws default to the case's tensors and to fresh ones; p: another C parameter
    record than the case's.  want: which input gradients a pullback writes; grads=False: its parameter gradients are NULL.  poison: outputs start
    as NaN, the workspace as 0xA5 bytes (at least 256 of them).  Device memory is taken in the order the tools always took it: a forward's
    outputs, then its workspace; a pullback's workspace (workspace() takes those of several forms first), its input gradients, its gradient slots.
    Returns Call(f, nbytes, outs, grads, ws, entry, keep): f(x=None, cot=None, outs=None, ws=None, fwd=None) runs the call, on other tensors where given,
    and asserts that it returned 0; outs: the three outputs (forward) or input gradients (backward), None where there is none."""
    import torch
    api, lib = gn.api, gn._lib.load()
    g, R, back = case.g, case.R, direction == "backward"
    e = resolve(gn, family, direction, elem, entry, record=drop is not None, narrow=narrow)
    if query is not None:
        e = e._replace(query=query[0], query_tail=tuple(query[1]))
    env = dict(flags=flags, drop=None if drop is None else C.byref(drop))
    h, pp = g._h, C.byref(case.p if p is None else p)
    s = torch.cuda.current_stream().cuda_stream
    dt = elem_dtype(gn, elem)
    nbytes = int(getattr(lib, e.query)(h, pp, R, *api._values(e.query_tail, env)))
    assert poison or family != "chain" or nbytes > 0, lib.gnx_last_error()  # (a Chain query's 0 is a refusal)
    x = case.x if x is None else x
    if outs is None and not back:
        outs = [_poisoned(torch, (R, T, d), dt, poison) if d else None for T, d in zip(rows(g), case.out_widths)]
    if ws is None:
        ws = torch.full((max(nbytes, 256),), 0xA5, dtype=torch.uint8, device="cuda") if poison else torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    if outs is None:
        outs = [_poisoned(torch, tuple(t.shape), dt, poison) if t is not None and w else None for t, w in zip(x, want)]
    gs, rec, alive = grad_slots(gn, case, family, poison, layout) if back and grads else ([], None, [])
    fwd = list(fwd) if family == "block" and back else []  # (a block pullback reads the forward's outputs too)
    cot = list(case.cot if cot is None else cot) if back else []
    post = (None if rec is None else C.byref(rec),) if back else ()
    head, tail, call = api._values(e.head, env), api._values(e.tail, env), getattr(lib, e.call)
    ptrs = lambda given, default: default if given is None else [ptr(t) for t in given]
    X, F, G, O_, W = ptrs(x, None), ptrs(fwd, None), ptrs(cot, None), ptrs(outs, None), ws

    def f(x=None, cot=None, outs=None, ws=None, fwd=None):
        w = W if ws is None else ws
        rc = call(h, pp, *head, *ptrs(x, X), *ptrs(fwd, F), *ptrs(cot, G), R, *ptrs(outs, O_), *post, w.data_ptr(), nbytes, *tail, s)
        assert rc == 0, (e.call, lib.gnx_last_error())

    return Call(f, nbytes, outs, gs, ws, e, [case, x, fwd, cot, outs, gs, rec, alive, ws, drop])


def workspace(gn, case, family, direction, elem, entry, **kw):
    """the workspace of the call that build() makes from the same arguments, allocated now: a tool that times several pullbacks takes all
    their workspaces first and hands each to build(ws=...)"""
    import torch
    e = resolve(gn, family, direction, elem, entry, record=kw.get("drop") is not None, narrow=kw.get("narrow", 0))
    env = dict(flags=kw.get("flags", 0), drop=None)
    nbytes = int(getattr(gn._lib.load(), e.query)(case.g._h, C.byref(case.p), case.R, *gn.api._values(e.query_tail, env)))
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda")


def applies(gn, case, name, *more, p=None):
    """the int an `_applies` query of include/gnx.h returns for the case: name(handle, params, R, *more)"""
    return int(getattr(gn._lib.load(), name)(case.g._h, C.byref(case.p if p is None else p), case.R, *more))
