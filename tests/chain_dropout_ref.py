"""Shared by the tests of the Chain block's training mode (Dropout entries inside the update-function Chains: include/gnx.h,
gnx_chain_block_forward_train / _backward_train): how a test writes such a block down, the float64 restatement with the library's masks read as
constants, and one block on one batch through the ABI.

A case is the oracle's chain parameters `p` (oracle.gn_oracle.make_chain_block_params) and `drops`: {"edge" | "node" | "graph": {i: p_drop}} — a
Dropout(p_drop) stands right behind layer i of p[name].  The entries of the call's chain are then the layers with the Dropouts where they stand."""
import ctypes as C

import numpy as np

from oracle import gn_oracle as O
from tests import util as U

FN = ("edge", "node", "graph")


def mask_numpy(seed, function, layer, p, n):
    """include/gnx.h's definition of the mask restated on the host: element i of the flat tensor is mask_of(component i % 4 of
    philox4(i / 4, 16 + 16 function + layer, seed), p, scale) — Philox-4x32-10, counter (quad lo, quad hi, stream, 0x676e78), key = the seed;
    mask_of(bits) = (bits >> 8) / 2^24 > p ? 1 / (1 - p) : 0 in float32."""
    M = np.uint64(0xFFFFFFFF)
    quad = np.arange((n + 3) // 4, dtype=np.uint64)
    c = [quad & M, quad >> np.uint64(32), np.full_like(quad, 16 + 16 * function + layer), np.full_like(quad, 0x676E78)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    bits = np.stack(c, axis=1).reshape(-1)[:n]
    u = (bits >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    pf = np.float32(p)
    scale = np.float32(1) / (np.float32(1) - pf) if pf < 1 else np.float32(0)
    return np.where(u > pf, scale, np.float32(0)).astype(np.float32)


def entries(p, drops):
    """{name: [("layer", i) | ("dropout", p_drop), ...]} in the order of the call's chain"""
    out = {}
    for name in FN:
        es = []
        for i in range(len(p[name])):
            es.append(("layer", i))
            if i in drops.get(name, {}):
                es.append(("dropout", float(drops[name][i])))
        out[name] = es
    return out


def drop_after_hidden(p, pd=0.25):
    """a Dropout(pd) behind every hidden Dense of every function (not behind a LayerNorm, not behind the last layer)"""
    return {name: {i: pd for i, l in enumerate(p[name][:-1]) if not isinstance(l[0], str)} for name in FN}


def widths(p, name):
    """output width of every layer of p[name] (a LayerNorm keeps its input's: the length of gamma)"""
    return [len(l[1]) if isinstance(l[0], str) else l[0].shape[0] for l in p[name]]


def block(gn, p, drops, **switches):
    """the GNBlock of the case: Chains of Dense / LayerNorm layers with gn.Dropout where `drops` puts them"""
    de, dn, dg = p["in_dims"]
    blk = gn.GNBlock((de, dn, dg), (1, 0, 0), **switches)  # placeholder layers: the chains below define the widths

    def mk(name):
        ls = []
        for i, (W, b, a) in enumerate(p[name]):
            ls.append(gn.LayerNorm.from_numpy(b, a) if isinstance(W, str) else gn.Dense.from_numpy(W, b, U.ACT_NAMES[a]))
            if i in drops.get(name, {}):
                ls.append(gn.Dropout(drops[name][i]))
        return gn.Chain(ls)

    blk.edgefn, blk.nodefn, blk.graphfn = mk("edge"), mk("node"), mk("graph")
    return blk


def insert_dropouts(L, q, ent, keep):
    """gnx_chain_block_params `q` of the stripped chains (any pointers) -> the call's chains: the same entries with GNX_LAYER_DROPOUT entries
    (no weight, no bias, identity, the width of the entry in front) where `ent` has them"""
    out = L.ChainBlockParams()
    out.de, out.dn, out.dg = q.de, q.dn, q.dg
    for name, field in zip(FN, ("edgefn", "nodefn", "graphfn")):
        src, es = getattr(q, field), ent[name]
        arr = (L.Dense * max(len(es), 1))()
        wid = (C.c_int32 * max(len(es), 1))()
        for e, (kind, v) in enumerate(es):
            if kind == "dropout":
                arr[e], wid[e] = L.Dense(None, None, 0, L.LAYER_DROPOUT), wid[e - 1]
            else:
                arr[e], wid[e] = src.layers[v], src.widths[v]
        keep += [arr, wid]
        ch = getattr(out, field)
        ch.layers, ch.widths, ch.n_layers = arr, wid, len(es)
    return out


def torch_block(csc, ef, nf, gf, W, ent, masks, want_scale=False):
    """float64 torch restatement of the block with Dropout entries (one replica).  W[name]: the layers as tests.chain_torch takes them; ent:
    entries(); masks[name][entry index]: the [rows][w] mask of that entry as a constant.  Returns (outputs, scales or None, pre): scales as
    oracle.chain_block_forward_sparse propagates them (|W| S + |b| through a Dense, layernorm_scale), multiplied by the mask at a Dropout."""
    import torch
    ACT = {0: lambda x: x, 1: torch.relu, 2: torch.tanh, 3: torch.sigmoid, 4: lambda x: torch.nn.functional.gelu(x, approximate="tanh")}
    colptr, rowval, node_off, edge_off = (torch.from_numpy(np.asarray(a)) for a in csc)
    N, G = len(colptr) - 1, len(node_off) - 1
    dst = torch.repeat_interleave(torch.arange(N), colptr[1:] - colptr[:-1])
    ng = torch.repeat_interleave(torch.arange(G), node_off[1:] - node_off[:-1])
    eg = torch.repeat_interleave(torch.arange(G), edge_off[1:] - edge_off[:-1])
    cat = lambda parts: torch.cat([q for q in parts if q is not None], dim=1)
    seg = lambda v, idx, n: torch.zeros((n, v.shape[1]), dtype=v.dtype).index_add(0, idx, v)
    pre = []

    def chain(name, x, s):
        for e, (kind, v) in enumerate(ent[name]):
            if kind == "dropout":
                m = torch.from_numpy(np.asarray(masks[name][e], dtype=np.float64))
                x = x * m
                s = None if s is None else s * m
                continue
            w, b, a = W[name][v]
            if isinstance(w, str):
                if s is not None:
                    s = torch.from_numpy(np.asarray(O.layernorm_scale(x.detach().numpy(), s.numpy(), b.detach().numpy(), a.detach().numpy(), O.CHAIN_LN_EPS,
                                                                      O.ln_eps_mode(w)), dtype=np.float64))
                mu = x.mean(dim=1, keepdim=True)
                var = ((x - mu) ** 2).mean(dim=1, keepdim=True)
                den = (var + 1e-5).sqrt() if O.ln_eps_mode(w) == 1 else var.sqrt() + 1e-5
                x = b * ((x - mu) / den) + a
                continue
            if s is not None:
                s = s.abs() @ w.detach().abs().T + b.detach().abs()
            z = x @ w.T + b
            pre.append((z, a))
            x = ACT[a](z)
        return x, s

    ab = (lambda v: v.detach().abs()) if want_scale else (lambda v: None)
    xe = cat([ef, None if nf is None else nf[rowval], None if nf is None else nf[dst], None if gf is None else gf[eg]])
    he, se = chain("edge", xe, ab(xe))
    hn = sn = hg = sg = None
    if W["node"]:
        xn = cat([seg(he, dst, N), nf, None if gf is None else gf[ng]])
        hn, sn = chain("node", xn, cat([seg(se, dst, N), ab(nf) if nf is not None else None, None if gf is None else ab(gf)[ng]]) if want_scale else None)
    if W["graph"]:
        xg = cat([seg(he, eg, G), None if hn is None else seg(hn, ng, G), gf])
        hg, sg = chain("graph", xg, cat([seg(se, eg, G), None if sn is None else seg(sn, ng, G), ab(gf) if gf is not None else None]) if want_scale else None)
    return (he, hn, hg), (se, sn, sg), pre


class TrainCall:
    """one block with Dropout entries on one batch: the parameters, the inputs, the record, and the four training entries through the ABI on
    workspaces of exactly the queried sizes; next to it the stripped block (the chains without their Dropouts) for the mirrored entries"""

    def __init__(self, gn, adjs, p, drops, R=1, seed=0):
        import torch
        from tests import test_gpu_chain as TC
        self.gn, self.L, self.lib, self.p, self.drops, self.R = gn, gn._lib, gn._lib.load(), p, drops, R
        self.g = gn.GNGraphBatch(adjs)
        self.csc = O.csc_from_adj(adjs)
        self.x = U.packed_inputs(np.random.default_rng(9000 + seed), R, self.g.n_edges, self.g.n_nodes, self.g.n_graphs, p["in_dims"])
        self.xt = [None if a is None else torch.from_numpy(a).to(self.g.device) for a in self.x]
        self.ent = entries(p, drops)
        self.blk = block(gn, p, drops)
        self.keep = []
        self.cp, _, self.outw = self.blk._chain_train_params(self.keep)
        self.blk0 = TC._block(gn, p)
        self.cp0 = self.blk0._chain_params(self.keep)[0]
        self.rows = (self.g.n_edges, self.g.n_nodes, self.g.n_graphs)

    def record(self, seed, scale_p=1.0):
        """the record of a call: every Dropout entry's p (times scale_p: 0 gives the all-identity record)"""
        return self.gn.ChainDropout(seed, [[v * scale_p if k == "dropout" else 0.0 for k, v in self.ent[name]] for name in FN])

    def entry_width(self, name, e):
        ws = widths(self.p, name)
        return ws[max(v for k, v in self.ent[name][:e + 1] if k == "layer")]

    def masks(self, rec):
        """{name: {entry index: float32 [R][rows][w]}} through gnx_chain_dropout_mask"""
        import torch
        out = {}
        keep = []
        crec = rec._c(keep)
        for t, name in enumerate(FN):
            out[name] = {}
            for e, (kind, _) in enumerate(self.ent[name]):
                if kind != "dropout":
                    continue
                m = torch.full((self.R, self.rows[t], self.entry_width(name, e)), float("nan"), dtype=torch.float32, device=self.g.device)
                rc = self.lib.gnx_chain_dropout_mask(C.byref(crec), t, e, rec.p[t][e], m.numel(), m.data_ptr(), torch.cuda.current_stream().cuda_stream)
                assert rc == 0, self.lib.gnx_last_error()
                out[name][e] = m.cpu().numpy()
        return out

    def applies(self, backward):
        return self.lib.gnx_chain_block_train_applies(self.g._h, C.byref(self.cp), self.R, int(backward))

    def query(self, narrow, backward=False, stripped=False):
        q = self.lib.gnx_chain_block_backward_train_workspace_bytes if backward else self.lib.gnx_chain_block_forward_train_workspace_bytes
        return q(self.g._h, C.byref(self.cp0 if stripped else self.cp), self.R, int(narrow))

    def outputs(self):
        import torch
        return [torch.full((self.R, T, d), float("nan"), dtype=torch.float32, device=self.g.device) if d > 0 else None for T, d in zip(self.rows, self.outw)]

    def fw(self, narrow, rec, outs=None, ws=None, fill=0xA5, stream=None, nbytes=None):
        import torch
        nbytes = self.query(narrow) if nbytes is None else nbytes
        assert nbytes > 0, self.lib.gnx_last_error()
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=self.g.device) if ws is None else ws
        outs = self.outputs() if outs is None else outs
        ptr = lambda t: None if t is None else t.data_ptr()
        keep = []
        crec = None if rec is None else C.byref(rec._c(keep))
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        rc = self.lib.gnx_chain_block_forward_train(self.g._h, C.byref(self.cp), crec, *map(ptr, self.xt), self.R, *map(ptr, outs), ws.data_ptr(), nbytes, int(narrow), 0, s)
        assert rc == 0, self.lib.gnx_last_error()
        return outs

    def fw_stripped(self, narrow):
        """the mirrored test-mode entry on the chains without their Dropouts"""
        import torch
        q, entry = ((self.lib.gnx_chain_block_forward_narrow_workspace_bytes, self.lib.gnx_chain_block_forward_narrow) if narrow else
                    (self.lib.gnx_chain_block_workspace_bytes, self.lib.gnx_chain_block_forward))
        nbytes = q(self.g._h, C.byref(self.cp0), self.R)
        ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=self.g.device)
        outs = self.outputs()
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = entry(self.g._h, C.byref(self.cp0), *map(ptr, self.xt), self.R, *map(ptr, outs), ws.data_ptr(), nbytes, 0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, self.lib.gnx_last_error()
        return outs, nbytes

    # ---- the pullback ----
    def grad_names(self):
        """every gradient tensor of the call: d_ef / d_nf / d_gf of the present inputs, "<fn><layer>.dW" / ".db" per layer of p"""
        shapes = {n: tuple(t.shape) for n, t in zip(("d_ef", "d_nf", "d_gf"), self.xt) if t is not None}
        for name in FN:
            for i, (W, b, a) in enumerate(self.p[name]):
                shapes[f"{name}{i}.dW"] = (len(b),) if isinstance(W, str) else (W.shape[1], W.shape[0])
                shapes[f"{name}{i}.db"] = (len(a),) if isinstance(W, str) else (len(b),)
        return shapes

    def grads(self, skip=()):
        import torch
        return {n: torch.full(s, float("nan"), dtype=torch.float32, device=self.g.device) for n, s in self.grad_names().items() if n not in skip}

    def _grad_arrays(self, outs, ent):
        L = self.L
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        arrays = []
        for name in FN:
            arr = (L.DenseGrad * max(len(ent[name]), 1))()
            for e, (kind, v) in enumerate(ent[name]):
                arr[e] = L.DenseGrad(None, None) if kind == "dropout" else L.DenseGrad(ptr(outs.get(f"{name}{v}.dW")), ptr(outs.get(f"{name}{v}.db")))
            arrays.append(arr)
        return arrays, L.ChainBlockGrads(*[C.cast(a, C.POINTER(L.DenseGrad)) for a in arrays])

    def bw(self, narrow, rec, cot, outs=None, ws=None, fill=0xA5, stream=None, skip=(), nbytes=None):
        import torch
        nbytes = self.query(narrow, backward=True) if nbytes is None else nbytes
        assert nbytes > 0, self.lib.gnx_last_error()
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=self.g.device) if ws is None else ws
        outs = self.grads(skip) if outs is None else outs
        arrays, gr = self._grad_arrays(outs, self.ent)
        keep = []
        crec = None if rec is None else C.byref(rec._c(keep))
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = self.lib.gnx_chain_block_backward_train(self.g._h, C.byref(self.cp), crec, *map(ptr, self.xt), *map(ptr, cot), self.R,
                                                     *[ptr(outs.get(n)) for n in ("d_ef", "d_nf", "d_gf")], C.byref(gr), ws.data_ptr(), nbytes, int(narrow), s)
        assert rc == 0, self.lib.gnx_last_error()
        return outs

    def bw_stripped(self, narrow, cot):
        import torch
        q, entry = ((self.lib.gnx_chain_block_backward_narrow_workspace_bytes, self.lib.gnx_chain_block_backward_narrow) if narrow else
                    (self.lib.gnx_chain_block_backward_workspace_bytes, self.lib.gnx_chain_block_backward))
        nbytes = q(self.g._h, C.byref(self.cp0), self.R)
        ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=self.g.device)
        outs = self.grads()
        arrays, gr = self._grad_arrays(outs, entries(self.p, {}))
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = entry(self.g._h, C.byref(self.cp0), *map(ptr, self.xt), *map(ptr, cot), self.R, *[ptr(outs.get(n)) for n in ("d_ef", "d_nf", "d_gf")], C.byref(gr),
                   ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, self.lib.gnx_last_error()
        return outs, nbytes

    def cotangents(self, seed):
        import torch
        rng = np.random.default_rng(12000 + seed)
        return [torch.from_numpy(rng.standard_normal((self.R, T, d)).astype(np.float32)).to(self.g.device) if d > 0 else None for T, d in zip(self.rows, self.outw)]

    # ---- float64 ----
    def reference(self, masks, cot=None, kink=5e-6):
        """float64: (outputs [R][rows][w], scales, gradients by name or None, kink-free) with `masks` (self.masks(rec)) as constants; the
        parameter gradients summed over the replicas.  kink-free: no relu pre-activation within fp32 rounding of 0, every gradient finite."""
        import torch
        T = lambda v: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True)
        W = {name: [(w, T(b), T(c)) if isinstance(w, str) else (T(w), T(b), c) for w, b, c in self.p[name]] for name in FN}
        outs, scales, ok = [[], [], []], [[], [], []], True
        dx = [None if v is None else np.zeros(v.shape) for v in self.x]
        for r in range(self.R):
            xs = [None if v is None else T(v[r]) for v in self.x]
            mr = {name: {e: m[r] for e, m in masks[name].items()} for name in FN}
            o, s, pre = torch_block(self.csc, *xs, W, self.ent, mr, want_scale=True)
            ok = ok and not any(a == 1 and z.numel() and float(z.detach().abs().min()) < kink for z, a in pre)
            for t in range(3):
                if o[t] is not None:
                    outs[t].append(o[t].detach().numpy()); scales[t].append(s[t].numpy())
            if cot is not None:
                sum((o[t] * torch.from_numpy(cot[t][r].cpu().numpy().astype(np.float64))).sum() for t in range(3) if o[t] is not None).backward()
                for t in range(3):
                    if xs[t] is not None:
                        dx[t][r] = xs[t].grad.numpy() if xs[t].grad is not None else 0.0
        stack = lambda q: [np.stack(v) if v else None for v in q]
        grads = None
        if cot is not None:
            grads = {n: v for n, v in zip(("d_ef", "d_nf", "d_gf"), dx) if v is not None}
            zero = lambda q: np.zeros(tuple(q.shape)) if q.grad is None else q.grad.numpy()
            for name in FN:
                for i, (w, b, c) in enumerate(W[name]):
                    grads[f"{name}{i}.dW"], grads[f"{name}{i}.db"] = (zero(b), zero(c)) if isinstance(w, str) else (zero(w).T, zero(b))
            ok = ok and all(np.isfinite(v).all() for v in grads.values())  # (a LayerNorm of a constant row has no float64 derivative: re-draw)
        return stack(outs), stack(scales), grads, ok
