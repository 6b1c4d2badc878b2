"""
gn_oracle — CPU restatement of GraphNets.jl's GNBlock / GNCore forward pass.

*** TEST INFRASTRUCTURE ONLY. ***  Nothing under `oracle/` is part of the product.  Only `tests/`,
`__graft_entry__.smoke()` and the `cpu_baseline` leg of `bench.py` may import it, and only as the
checker.  The product path (`graphnets.jl_amd/`, `libgnx.so`) never calls into this directory.

*** PARITY UNPINNED (absolute numerics). ***  The reference is pure Julia (Flux 0.14 / NNlib); Julia is not
installed here or on the GPU box, so the reference can be neither compiled nor imported, and its test-suite
(`/root/reference/test/runtests.jl`) holds no numerical golden values for this path.  What IS pinned:
  * the index semantics (src = row, dst = column, column-major edge slots, aggregation at dst), against the
    known-answer matrices the reference's tests hold (`test/runtests.jl:487-508`, `:659-680`), transcribed
    as data in `tests/golden/reference_known_answers.json`;
  * the relational properties the reference tests assert (batch invariance `:62-116`, batch∘unbatch identity
    `:328-390`, output shapes / `nothing` handling `:118-326`).
The arithmetic of `Dense`, `LayerNorm`, `batched_mul` lives in un-vendored Flux/NNlib/BLAS (Project.toml:6-15,
no Manifest); their assumed semantics are restated below from the published definitions.

Two forms are provided, both float64:
  (i)  DENSE form  — a line-by-line restatement of the reference's padded N^2 edge grid + one-hot
       "broadcaster" batched matmuls.  Only usable for tiny graphs.  Arrays use the reference's Julia
       shapes `(D, T, B)`; "column-major flatten" is spelled `order='F'`.
  (ii) SPARSE form — the same mathematics on packed CSC data, arrays in the C-ABI layout `[R][T][D]`
       (byte-identical to Julia's column-major `(D, T, R)`).
`tests/test_oracle.py` proves (i) == (ii) and checks both against the reference's fixtures.

The SPARSE form also has the pullbacks of the block, the core and the block with Chain update functions (`block_backward_sparse`,
`core_backward_sparse`, `chain_block_backward_sparse`), each gradient with an error scale; `tests/test_bw_x6_stress_cpu.py` and
`tests/test_chain_bw_stress_cpu.py` prove them equal to torch float64 autograd of the forward's restatements.
"""
from __future__ import annotations

import numpy as np

F64 = np.float64

# ----------------------------------------------------------------------------------------------------------
# Activations (Flux/NNlib definitions)
# ----------------------------------------------------------------------------------------------------------
ACT_IDENTITY, ACT_RELU, ACT_TANH, ACT_SIGMOID, ACT_GELU = 0, 1, 2, 3, 4


def apply_act(x, act):
    if act == ACT_IDENTITY:
        return x
    if act == ACT_RELU:
        return np.maximum(x, 0.0)
    if act == ACT_TANH:
        return np.tanh(x)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-x))
    if act == ACT_GELU:  # NNlib.gelu = tanh approximation
        return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))
    raise ValueError(f"unknown activation {act}")


# ----------------------------------------------------------------------------------------------------------
# Parameters
# ----------------------------------------------------------------------------------------------------------
def glorot_uniform(rng, out_dim, in_dim):
    """Flux.glorot_uniform: U(-s, s), s = sqrt(6 / (fan_in + fan_out)); weight is (out, in)."""
    if out_dim == 0 or in_dim == 0:
        return np.zeros((out_dim, in_dim), dtype=np.float32)
    s = np.sqrt(6.0 / (in_dim + out_dim))
    return rng.uniform(-s, s, size=(out_dim, in_dim)).astype(np.float32)


def block_input_widths(in_dims, out_dims):
    """gnblock.jl:52-54."""
    de, dn, dg = in_dims
    oe, on, og = out_dims
    return de + 2 * dn + dg, dn + oe + dg, on + oe + dg


def make_block_params(rng, in_dims, out_dims, random_bias=True, act=(0, 0, 0)):
    """GNBlock(in => out) (gnblock.jl:47-61): three single-Dense chains.  Flux's default bias is zero; tests
    draw U(-0.1, 0.1) biases so the bias path is exercised."""
    assert any(d > 0 for d in in_dims) and any(d > 0 for d in out_dims)  # gnblock.jl:48-49
    ke, kn, kg = block_input_widths(in_dims, out_dims)
    oe, on, og = out_dims

    def bias(n):
        return (rng.uniform(-0.1, 0.1, size=n) if random_bias else np.zeros(n)).astype(np.float32)

    return dict(
        in_dims=tuple(in_dims), out_dims=tuple(out_dims),
        We=glorot_uniform(rng, oe, ke), be=bias(oe), act_e=act[0],
        Wn=glorot_uniform(rng, on, kn), bn=bias(on), act_n=act[1],
        Wg=glorot_uniform(rng, og, kg), bg=bias(og), act_g=act[2],
    )


def make_core_params(rng, dims, random_bias=True, eps=1e-5, eps_mode=0):
    """GNCore(dims) (gncore.jl:46-54): block dims=>dims, GNFeedForward (gnfeedforward.jl:17-31),
    two GNGraphNorm (gngraphnorm.jl:9-17).  LayerNorm affine params are drawn randomly (Flux init is 1/0)."""
    assert all(d > 0 for d in dims)  # gnfeedforward.jl:18, gngraphnorm.jl:10
    p = dict(dims=tuple(dims), block=make_block_params(rng, dims, dims, random_bias), eps=eps, eps_mode=eps_mode)
    for tag, d in zip("eng", dims):
        for ln in ("ln1", "ln2"):
            p[f"{ln}_{tag}_gamma"] = rng.uniform(0.5, 1.5, size=d).astype(np.float32)
            p[f"{ln}_{tag}_beta"] = rng.uniform(-0.1, 0.1, size=d).astype(np.float32)
        p[f"ff_{tag}_W1"] = glorot_uniform(rng, 4 * d, d)
        p[f"ff_{tag}_b1"] = (rng.uniform(-0.1, 0.1, size=4 * d) if random_bias else np.zeros(4 * d)).astype(np.float32)
        p[f"ff_{tag}_W2"] = glorot_uniform(rng, d, 4 * d)
        p[f"ff_{tag}_b2"] = (rng.uniform(-0.1, 0.1, size=d) if random_bias else np.zeros(d)).astype(np.float32)
    return p


# ----------------------------------------------------------------------------------------------------------
# (i) DENSE form — literal restatement of the reference
# ----------------------------------------------------------------------------------------------------------
def padadjmats(adj_mats):
    """pad.jl:1-10 → (PN, PN, B)."""
    B = len(adj_mats)
    PN = max(a.shape[0] for a in adj_mats)
    out = np.zeros((PN, PN, B), dtype=F64)
    for b, a in enumerate(adj_mats):
        n = a.shape[0]
        out[:n, :n, b] = a
    return out


def getnode2edgebroadcaster(padded, transpose=False):
    """gngraphbatch.jl:197-211.  idx[i, j] = i (src) or j (dst, `transpose`), 1-based; one-hot of the masked
    index scattered into column `slot` of a (PN, PN^2) matrix."""
    PN, _, B = padded.shape
    idx = np.repeat(np.arange(1, PN + 1)[:, None], PN, axis=1).astype(F64)  # repeat(1:PN, 1, PN)
    if transpose:
        idx = idx.T
    dst = np.zeros((PN, PN * PN, B), dtype=F64)
    for b in range(B):
        flat = (padded[:, :, b] * idx).flatten(order="F")
        active_idx = np.nonzero(flat)[0]
        active = flat[active_idx].astype(np.int64)
        for slot, node in zip(active_idx, active):  # onehotbatch + scatter!(+)
            dst[node - 1, slot, b] += 1.0
    return dst


def getgraph2edgebroadcaster(padded):
    """gngraphbatch.jl:183-192 → (1, PN^2, B)."""
    PN, _, B = padded.shape
    m = np.zeros((1, PN * PN, B), dtype=F64)
    for b in range(B):
        m[0, :, b] = (padded[:, :, b].flatten(order="F") == 1.0)
    return m


def getedge2nodebroadcaster(padded):
    """gngraphbatch.jl:158-170 → (PN^2, PN, B)."""
    PN, _, B = padded.shape
    m = np.zeros((PN * PN, PN, B), dtype=F64)
    for b in range(B):
        for col in range(PN):
            m[PN * col: PN * col + PN, col, b] = padded[:, col, b]
    return m


def getgraph2nodebroadcaster(adj_mats, PN):
    """gngraphbatch.jl:172-181 → (1, PN, B)."""
    m = np.zeros((1, PN, len(adj_mats)), dtype=F64)
    for b, a in enumerate(adj_mats):
        m[0, : a.shape[0], b] = 1.0
    return m


def getedge2graphbroadcaster(padded):
    """gngraphbatch.jl:136-146 → (PN^2, 1, B)."""
    PN, _, B = padded.shape
    m = np.zeros((PN * PN, 1, B), dtype=F64)
    for b in range(B):
        m[:, 0, b] = padded[:, :, b].flatten(order="F")
    return m


def getnode2graphbroadcaster(adj_mats, PN):
    """gngraphbatch.jl:148-156 → (PN, 1, B)."""
    m = np.zeros((PN, 1, len(adj_mats)), dtype=F64)
    for b, a in enumerate(adj_mats):
        m[: a.shape[0], 0, b] = 1.0
    return m


class DenseGraphBatch:
    """GNGraphBatch (gngraphbatch.jl:1-54) without the edge-collapse members."""

    def __init__(self, adj_mats):
        self.adj_mats = [np.asarray(a, dtype=F64) for a in adj_mats]
        self.padded_adj_mats = padadjmats(self.adj_mats)
        PN = self.padded_adj_mats.shape[0]
        self.node_block_size = PN
        self.edge_block_size = PN * PN
        self.srcnode2edge = getnode2edgebroadcaster(self.padded_adj_mats)
        self.dstnode2edge = getnode2edgebroadcaster(self.padded_adj_mats, transpose=True)
        self.graph2edge = getgraph2edgebroadcaster(self.padded_adj_mats)
        self.edge2node = getedge2nodebroadcaster(self.padded_adj_mats)
        self.graph2node = getgraph2nodebroadcaster(self.adj_mats, PN)
        self.edge2graph = getedge2graphbroadcaster(self.padded_adj_mats)
        self.node2graph = getnode2graphbroadcaster(self.adj_mats, PN)
        # gngraphbatch.jl:113-134
        B = len(self.adj_mats)
        self.flat_node_unpadder = np.zeros(B * PN, dtype=bool)
        self.flat_edge_unpadder = np.zeros(B * PN * PN, dtype=bool)
        for b, a in enumerate(self.adj_mats):
            self.flat_node_unpadder[b * PN: b * PN + a.shape[0]] = True
            self.flat_edge_unpadder[b * PN * PN: (b + 1) * PN * PN] = self.padded_adj_mats[:, :, b].flatten(order="F") == 1.0


def getlowertriangularcoords(n):
    """gngraphbatch.jl:56-58: CartesianIndices of an n x n matrix with i >= j, in column-major order (0-based pairs)."""
    return [(i, j) for j in range(n) for i in range(n) if i >= j]


def getedgecollapser(n):
    """gngraphbatch.jl:67-82: (n^2, n(n+1)/2) matrix; column of coordinate (i, j) has a one at slots (i,j) and (j,i) of the
    column-major n x n grid — a two on the diagonal, since the reference adds both."""
    coords = getlowertriangularcoords(n)
    m = np.zeros((n * n, len(coords)), dtype=F64)
    for c, (i, j) in enumerate(coords):
        m[i + n * j, c] += 1
        m[j + n * i, c] += 1
    return m


def getcollapsededgeidxs(padded):
    """gngraphbatch.jl:60-65: per graph, positions (0-based) within the lower-triangle coordinate list whose adjacency entry is one."""
    coords = getlowertriangularcoords(padded.shape[0])
    return [np.array([c for c, (i, j) in enumerate(coords) if padded[i, j, b] == 1.0], dtype=np.int64) for b in range(padded.shape[2])]


def collapsef_dense(x):
    """gngraphbatch.jl:83-85: batched_mul(graph.ef, graph.graphs.edge_collapser) / Float32(2) on the padded (DE, PN^2, B) array."""
    return batched_mul(x["ef"], getedgecollapser(x["graphs"].node_block_size)) / 2.0


def unpaddedcollapsedef_dense(x):
    """gngraphbatch.jl:87-107: per batch element, the collapsed columns of the real lower-triangle edges."""
    c = collapsef_dense(x)
    idxs = getcollapsededgeidxs(x["graphs"].padded_adj_mats)
    if len(idxs) == 1:  # shared adjacency: one index list for every batch element
        return [c[:, idxs[0], b] for b in range(c.shape[2])]
    return [c[:, idxs[b], b] for b in range(c.shape[2])]


def batched_mul(A, Bm):
    """NNlib.batched_mul: C[:,:,k] = A[:,:,k] * B[:,:,k]; a size-1 batch on either side broadcasts."""
    if A.ndim == 2:
        A = A[:, :, None]
    if Bm.ndim == 2:
        Bm = Bm[:, :, None]
    nb = max(A.shape[2], Bm.shape[2])
    assert A.shape[2] in (1, nb) and Bm.shape[2] in (1, nb)
    out = np.zeros((A.shape[0], Bm.shape[1], nb), dtype=F64)
    for k in range(nb):
        out[:, :, k] = A[:, :, k if A.shape[2] > 1 else 0] @ Bm[:, :, k if Bm.shape[2] > 1 else 0]
    return out


def padef_shared(adj, ef):
    """pad.jl:26-39: packed (DE, E, B) scattered into (DE, N^2, B) at the column-major positions of the ones."""
    n = adj.shape[0]
    edge_idx = np.nonzero(np.asarray(adj).flatten(order="F") == 1)[0]
    out = np.zeros((ef.shape[0], n * n, ef.shape[2]), dtype=F64)
    out[:, edge_idx, :] = ef
    return out


def padef_vector(adj_mats, efs):
    """pad.jl:48-64."""
    padded = padadjmats(adj_mats)
    PN = padded.shape[0]
    out = np.zeros((efs[0].shape[0], PN * PN, len(adj_mats)), dtype=F64)
    for b, ef in enumerate(efs):
        edge_idx = np.nonzero(padded[:, :, b].flatten(order="F") == 1)[0]
        out[:, edge_idx, b] = ef
    return out


def padnf_vector(adj_mats, nfs):
    """pad.jl:14-24."""
    PN = max(a.shape[0] for a in adj_mats)
    out = np.zeros((nfs[0].shape[0], PN, len(adj_mats)), dtype=F64)
    for b, nf in enumerate(nfs):
        out[:, : nf.shape[1], b] = nf
    return out


def batch_dense(graphs, ef, nf, gf):
    """batch (batch.jl:53-64).  `graphs` is one adjacency matrix (shared; ef (DE,E,B), nf (DN,N,B), gf (DG,B))
    or a list (vector mode; lists of (DE,E_g), (DN,N_g), (DG,))."""
    assert not (ef is None and nf is None and gf is None)  # batch.jl:56
    if isinstance(graphs, (list, tuple)):
        adj_mats = [np.asarray(a) for a in graphs]
        g = DenseGraphBatch(adj_mats)
        bef = None if ef is None else padef_vector(adj_mats, [np.asarray(x, dtype=F64) for x in ef])
        bnf = None if nf is None else padnf_vector(adj_mats, [np.asarray(x, dtype=F64) for x in nf])
        bgf = None if gf is None else np.stack([np.asarray(x, dtype=F64) for x in gf], axis=1)[:, None, :]  # pad.jl:67
    else:
        adj = np.asarray(graphs)
        g = DenseGraphBatch([adj])
        bef = None if ef is None else padef_shared(adj, np.asarray(ef, dtype=F64))
        bnf = None if nf is None else np.asarray(nf, dtype=F64)  # pad.jl:12
        bgf = None if gf is None else np.asarray(gf, dtype=F64)[:, None, :]  # pad.jl:66
    return dict(graphs=g, ef=bef, nf=bnf, gf=bgf)


def dense_layer(W, b, act, x):
    """Flux.Dense on an N-D array: reshape to (in, :), y = act.(W*x .+ b), reshape back."""
    W = np.asarray(W, dtype=F64)
    b = np.asarray(b, dtype=F64)
    sh = x.shape
    y = W @ x.reshape(sh[0], -1, order="F") + b[:, None]
    return apply_act(y, act).reshape((W.shape[0],) + sh[1:], order="F")


def _vcat(parts):
    return np.concatenate([p for p in parts if p is not None], axis=0)


def getedgefninput_dense(g, ef, nf, gf):
    """edgefninput.jl:1-47 — segment order ef, nf⊗src, nf⊗dst, gf⊗g2e; absent inputs drop their segments."""
    parts = [ef]
    if nf is not None:
        parts += [batched_mul(nf, g.srcnode2edge), batched_mul(nf, g.dstnode2edge)]
    if gf is not None:
        parts += [batched_mul(gf, g.graph2edge)]
    return _vcat(parts)


def getnodefninput_dense(g, ef, nf, gf):
    """nodefninput.jl:1-24 — order agg, nf, gf."""
    parts = [batched_mul(ef, g.edge2node), nf]
    if gf is not None:
        parts += [batched_mul(gf, g.graph2node)]
    return _vcat(parts)


def getgraphfninput_dense(g, ef, nf, gf):
    """graphfninput.jl:1-13 — order edges, nodes, gf."""
    return _vcat([batched_mul(ef, g.edge2graph), batched_mul(nf, g.node2graph), gf])


def block_forward_dense(p, x):
    """(m::GNBlock)(x) (gnblock.jl:63-69) on the padded batched tuple; zero-row outputs → None (:71-78)."""
    g, ef, nf, gf = x["graphs"], x["ef"], x["nf"], x["gf"]
    h_ef = dense_layer(p["We"], p["be"], p["act_e"], getedgefninput_dense(g, ef, nf, gf))
    h_nf = dense_layer(p["Wn"], p["bn"], p["act_n"], getnodefninput_dense(g, h_ef, nf, gf))
    h_gf = dense_layer(p["Wg"], p["bg"], p["act_g"], getgraphfninput_dense(g, h_ef, h_nf, gf))
    z = lambda a: None if a.shape[0] == 0 else a
    return dict(graphs=g, ef=z(h_ef), nf=z(h_nf), gf=z(h_gf))


def layernorm(x, gamma, beta, eps=1e-5, eps_mode=0, axis=0):
    """Flux.LayerNorm(d) over the feature dim.  eps_mode 0: Flux 0.14 `normalise` = (x-μ)/(σ+ε) with the
    uncorrected std; eps_mode 1: (x-μ)/sqrt(σ²+ε).  Then γ .* x̂ .+ β."""
    mu = x.mean(axis=axis, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=axis, keepdims=True)
    xhat = (x - mu) / (np.sqrt(var) + eps) if eps_mode == 0 else (x - mu) / np.sqrt(var + eps)
    shape = [1] * x.ndim
    shape[axis] = -1
    return xhat * np.asarray(gamma, dtype=F64).reshape(shape) + np.asarray(beta, dtype=F64).reshape(shape)


def core_forward_dense(p, x):
    """(m::GNCore)(x) = x + block(gn1(x)) + ffwd(gn2(x)) (gncore.jl:56-68)."""
    g = x["graphs"]
    ln = lambda which: dict(
        graphs=g,
        **{k: layernorm(x[k], p[f"{which}_{t}_gamma"], p[f"{which}_{t}_beta"], p["eps"], p["eps_mode"])
           for k, t in (("ef", "e"), ("nf", "n"), ("gf", "g"))})
    blk = block_forward_dense(p["block"], ln("ln1"))
    x2 = ln("ln2")
    out = dict(graphs=g)
    for k, t in (("ef", "e"), ("nf", "n"), ("gf", "g")):
        h = dense_layer(p[f"ff_{t}_W1"], p[f"ff_{t}_b1"], ACT_RELU, x2[k])
        ff = dense_layer(p[f"ff_{t}_W2"], p[f"ff_{t}_b2"], ACT_IDENTITY, h)  # Dropout: identity in test mode
        out[k] = x[k] + blk[k] + ff
    return out


def unbatch_dense(x):
    """unbatch (unbatch.jl:6-39, unpad.jl:1-25)."""
    g, ef, nf, gf = x["graphs"], x["ef"], x["nf"], x["gf"]
    if len(g.adj_mats) == 1:
        adj = g.adj_mats[0]
        idx = np.nonzero(adj.flatten(order="F") == 1)[0]
        return dict(graphs=adj, ef=None if ef is None else ef[:, idx, :], nf=nf,
                    gf=None if gf is None else gf.reshape(gf.shape[0], -1, order="F"))
    efs = nfs = gfs = None
    if ef is not None:
        efs = [ef[:, np.nonzero(g.padded_adj_mats[:, :, b].flatten(order="F") == 1)[0], b] for b in range(len(g.adj_mats))]
    if nf is not None:
        nfs = [nf[:, : a.shape[0], b] for b, a in enumerate(g.adj_mats)]
    if gf is not None:
        gfs = [gf[:, 0, b] for b in range(len(g.adj_mats))]
    return dict(graphs=g.adj_mats, ef=efs, nf=nfs, gf=gfs)


# ----------------------------------------------------------------------------------------------------------
# (ii) SPARSE form — packed CSC, C-ABI layout [R][T][D]
# ----------------------------------------------------------------------------------------------------------
def csc_from_adj(adj_mats):
    """Edge k of graph g ↔ k-th `1` of vec(A_g) column-major (pad.jl:30): sorted by dst (column) then src (row).
    Returns global colptr[N+1], rowval[E] (global src node id), node_off[G+1], edge_off[G+1] (int64)."""
    node_off, edge_off, colptr, rowval = [0], [0], [0], []
    for a in adj_mats:
        a = np.asarray(a)
        n = a.shape[0]
        assert a.shape == (n, n)
        base = node_off[-1]
        for j in range(n):
            rows = np.nonzero(a[:, j] == 1)[0]
            rowval.extend((rows + base).tolist())
            colptr.append(colptr[-1] + len(rows))
        node_off.append(base + n)
        edge_off.append(colptr[-1])
    return (np.asarray(colptr, dtype=np.int64), np.asarray(rowval, dtype=np.int64),
            np.asarray(node_off, dtype=np.int64), np.asarray(edge_off, dtype=np.int64))


def _dense_rows(W, b, act, X):
    """Dense applied to row-major rows: X (T, K) → (T, out)."""
    return apply_act(X @ np.asarray(W, dtype=F64).T + np.asarray(b, dtype=F64)[None, :], act)


_CHUNK = 1 << 17  # rows per chunk of the row-wise stages: bounds the temporaries at BASELINE's 1M-edge / 128-wide sizes


def _segsum(v, seg, n):
    """out[seg[k]] += v[k] with np.bincount per column (vectorised; np.add.at is an order of magnitude slower)."""
    out = np.empty((n, v.shape[1]), dtype=v.dtype)
    for c in range(v.shape[1]):
        out[:, c] = np.bincount(seg, weights=v[:, c], minlength=n)
    return out


def _scale_rows(S, W, b):
    """Error scale of a Dense: S·|W|ᵀ + |b| in float32 (a bound only needs a few digits; sgemm is what makes the
    full-size scales affordable)."""
    return S.astype(np.float32, copy=False) @ np.abs(np.asarray(W, dtype=np.float32)).T + np.abs(np.asarray(b, dtype=np.float32))[None, :]


def block_forward_sparse(p, csc, ef, nf, gf, return_scale=False, in_scale=None):
    """SURVEY Appendix A on packed data.  ef (R,E,DE) | None, nf (R,N,DN) | None, gf (R,G,DG) | None.
    Returns (ef', nf', gf') with zero-width outputs as None.  With `return_scale` also returns, per output, the
    magnitude bound |W|·S + |b| that the parity tests use as the tolerance scale: S = |x| for exact inputs, or the
    `in_scale` triple (each >= |input|, same shapes) when the inputs are themselves computed results — the bound then
    also covers the first-order propagation of their error (a perturbation δ <= c·eps·S of the inputs moves the outputs
    by at most c·eps·(|W|·S)).  This is a WORST-CASE bound (every rounding error aligned): right for one layer, vacuous for a
    deep chain through million-term sums and LayerNorm's 1/σ — chains are checked layer by layer from the float32-rounded
    oracle input of each layer instead (tests/test_gpu_fullsize.py).  (A quadrature / probabilistic scale was tried and is
    wrong here: gf and the gathered node rows are shared by many edges, their errors are fully correlated in the next sum.)
    The edge stage runs in row chunks (1M edges x 288 inputs would be 2.3 GB at once)."""
    colptr, rowval, node_off, edge_off = csc
    N, E, G = len(colptr) - 1, len(rowval), len(node_off) - 1
    R = next(a.shape[0] for a in (ef, nf, gf) if a is not None)
    dst = np.repeat(np.arange(N), np.diff(colptr))
    node_graph = np.repeat(np.arange(G), np.diff(node_off))
    edge_graph = np.repeat(np.arange(G), np.diff(edge_off))
    oe, on, og = p["out_dims"]
    We, Wn, Wg = (np.asarray(p[k], dtype=F64) for k in ("We", "Wn", "Wg"))
    want = return_scale
    sin = in_scale if in_scale is not None else (None, None, None)
    outs, scales = ([], [], []), ([], [], [])
    for r in range(R):
        efr = None if ef is None else ef[r]
        nfr = None if nf is None else np.asarray(nf[r], dtype=F64)
        gfr = None if gf is None else np.asarray(gf[r], dtype=F64)
        s_ef = None if (ef is None or not want) else (np.abs(efr) if sin[0] is None else sin[0][r])
        s_nf = None if (nf is None or not want) else (np.abs(nfr) if sin[1] is None else sin[1][r]).astype(np.float32)
        s_gf = None if (gf is None or not want) else (np.abs(gfr) if sin[2] is None else sin[2][r]).astype(np.float32)
        he = np.empty((E, oe), dtype=F64)
        se = np.empty((E, oe), dtype=np.float32) if want else None
        for c0 in range(0, max(E, 1), _CHUNK):
            c1 = min(E, c0 + _CHUNK)
            if c1 <= c0:
                break
            parts, sparts = [], []
            if ef is not None:
                parts.append(np.asarray(efr[c0:c1], dtype=F64))
                if want:
                    sparts.append(np.asarray(s_ef[c0:c1], dtype=np.float32))
            if nf is not None:
                parts += [nfr[rowval[c0:c1]], nfr[dst[c0:c1]]]
                if want:
                    sparts += [s_nf[rowval[c0:c1]], s_nf[dst[c0:c1]]]
            if gf is not None:
                parts.append(gfr[edge_graph[c0:c1]])
                if want:
                    sparts.append(s_gf[edge_graph[c0:c1]])
            Xe = np.concatenate(parts, axis=1) if parts else np.zeros((c1 - c0, 0))
            he[c0:c1] = _dense_rows(We, p["be"], p["act_e"], Xe)
            if want:
                se[c0:c1] = _scale_rows(np.concatenate(sparts, axis=1), We, p["be"])

        parts = [_segsum(he, dst, N)]
        sparts = [_segsum(se, dst, N).astype(np.float32)] if want else None
        if nf is not None:
            parts.append(nfr)
            if want:
                sparts.append(s_nf)
        if gf is not None:
            parts.append(gfr[node_graph])
            if want:
                sparts.append(s_gf[node_graph])
        hn = _dense_rows(Wn, p["bn"], p["act_n"], np.concatenate(parts, axis=1))
        sn = _scale_rows(np.concatenate(sparts, axis=1), Wn, p["bn"]) if want else None

        parts = [_segsum(he, edge_graph, G), _segsum(hn, node_graph, G)]
        sparts = [_segsum(se, edge_graph, G).astype(np.float32), _segsum(sn, node_graph, G).astype(np.float32)] if want else None
        if gf is not None:
            parts.append(gfr)
            if want:
                sparts.append(s_gf)
        hg = _dense_rows(Wg, p["bg"], p["act_g"], np.concatenate(parts, axis=1))
        sg = _scale_rows(np.concatenate(sparts, axis=1), Wg, p["bg"]) if want else None
        for lst, v in zip(outs, (he, hn, hg)):
            lst.append(v)
        for lst, v in zip(scales, (se, sn, sg)):
            lst.append(v)
    res = tuple(None if d == 0 else np.stack(lst) for d, lst in zip((oe, on, og), outs))
    if return_scale:
        return res, tuple(None if d == 0 else np.stack(lst) for d, lst in zip((oe, on, og), scales))
    return res


def layernorm_scale(x, s, gamma, beta, eps=1e-5, eps_mode=0):
    """Error scale of LayerNorm(x) over the last axis for an input that carries the error scale s >= |x| (first order,
    worst case): δμ <= mean(s), δ(x-μ) <= s + mean(s) =: sc, δσ <= sqrt(mean(sc²)) =: q (Cauchy-Schwarz on
    mean((x-μ)·δ(x-μ))/σ), hence δx̂ <= (sc + |x̂|·q) / (σ+ε); the affine part adds its own rounding |γ·x̂| + |β|.
    LayerNorm divides by σ: for U[0,1) inputs (σ ≈ 0.29) the scale grows about 3.5x — that is arithmetic, not slack."""
    x = np.asarray(x, dtype=F64)
    s = np.asarray(s, dtype=F64)
    mu = x.mean(axis=-1, keepdims=True)
    xc = x - mu
    var = (xc ** 2).mean(axis=-1, keepdims=True)
    den = (np.sqrt(var) + eps) if eps_mode == 0 else np.sqrt(var + eps)
    xhat = xc / den
    sc = s + s.mean(axis=-1, keepdims=True)
    q = np.sqrt((sc ** 2).mean(axis=-1, keepdims=True))
    g = np.abs(np.asarray(gamma, dtype=F64))
    return (g * ((sc + np.abs(xhat) * q) / den + np.abs(xhat)) + np.abs(np.asarray(beta, dtype=F64))).astype(np.float32)


def _ffn_rows(p, t, x2, s2):
    """FeedForward (gnfeedforward.jl:27-31) on rows, in chunks (the 4d-wide hidden layer of 1M x 128 rows is 4 GB in float64);
    returns (ff, scale | None)."""
    W1, b1, W2, b2 = p[f"ff_{t}_W1"], p[f"ff_{t}_b1"], p[f"ff_{t}_W2"], p[f"ff_{t}_b2"]
    rows = x2.reshape(-1, x2.shape[-1])
    ff = np.empty_like(rows)
    sc = None if s2 is None else np.empty(rows.shape, dtype=np.float32)
    srows = None if s2 is None else s2.reshape(-1, s2.shape[-1])
    for c0 in range(0, rows.shape[0], _CHUNK):
        c1 = min(rows.shape[0], c0 + _CHUNK)
        h = _dense_rows(W1, b1, ACT_RELU, rows[c0:c1])
        ff[c0:c1] = _dense_rows(W2, b2, ACT_IDENTITY, h)  # Dropout: identity in test mode
        if sc is not None:
            sc[c0:c1] = _scale_rows(_scale_rows(srows[c0:c1], W1, b1), W2, b2)
    return ff.reshape(x2.shape), (None if sc is None else sc.reshape(x2.shape))


def core_forward_sparse(p, csc, ef, nf, gf, return_scale=False, in_scale=None):
    """GNCore on packed data (all three inputs required, gncore.jl:61-68): y = x + block(gn1(x)) + ffwd(gn2(x)).
    `return_scale` / `in_scale` as in block_forward_sparse: the scale of every output is |x| (or its incoming scale) + the
    block's scale for inputs carrying gn1's scale + the FeedForward's scale for inputs carrying gn2's scale, so a chain of
    layers can hand each layer's scale to the next (tests: `<= 1e-5 * scale` at every depth)."""
    xs = dict(e=np.asarray(ef, dtype=F64), n=np.asarray(nf, dtype=F64), g=np.asarray(gf, dtype=F64))
    sx = None
    if return_scale:
        sin = in_scale if in_scale is not None else (None, None, None)
        sx = {t: (np.abs(xs[t]).astype(np.float32) if si is None else np.asarray(si, dtype=np.float32)) for t, si in zip("eng", sin)}
    ln = lambda which: {t: layernorm(xs[t], p[f"{which}_{t}_gamma"], p[f"{which}_{t}_beta"], p["eps"], p["eps_mode"], axis=-1)
                        for t in "eng"}
    lns = lambda which: {t: layernorm_scale(xs[t], sx[t], p[f"{which}_{t}_gamma"], p[f"{which}_{t}_beta"], p["eps"], p["eps_mode"])
                         for t in "eng"}
    x1 = ln("ln1")
    if return_scale:
        s1 = lns("ln1")
        blk, sblk = block_forward_sparse(p["block"], csc, x1["e"], x1["n"], x1["g"], return_scale=True, in_scale=(s1["e"], s1["n"], s1["g"]))
        del s1
    else:
        blk, sblk = block_forward_sparse(p["block"], csc, x1["e"], x1["n"], x1["g"]), (None, None, None)
    del x1
    out, scales = [], []
    for i, t in enumerate("eng"):
        x2 = layernorm(xs[t], p[f"ln2_{t}_gamma"], p[f"ln2_{t}_beta"], p["eps"], p["eps_mode"], axis=-1)
        s2 = layernorm_scale(xs[t], sx[t], p[f"ln2_{t}_gamma"], p[f"ln2_{t}_beta"], p["eps"], p["eps_mode"]) if return_scale else None
        ff, sff = _ffn_rows(p, t, x2, s2)
        out.append(xs[t] + blk[i] + ff)
        if return_scale:
            scales.append(sx[t] + sblk[i] + sff)
    if return_scale:
        return tuple(out), tuple(scales)
    return tuple(out)


# ----------------------------------------------------------------------------------------------------------
# Pullbacks (float64) with an error scale
# ----------------------------------------------------------------------------------------------------------
# The scale S of a gradient is THE SAME PULLBACK EVALUATED IN ABSOLUTE VALUES: a product contributes S_a · S_b, a sum the sum of its terms'
# scales; S_v = |v| for a tensor handed to the call; for a value the call recomputes (LayerNorm outputs, a core's block outputs, hidden units,
# a gelu pre-activation) S_v is the forward oracle's `return_scale`; act' taken from an output y contributes |act'| plus its first-order
# sensitivity to y times S_y.  The pullback is linear in the cotangents and made of products and sums only, so values and scales run through
# the same code (`_dense_pullback`, `_ln_pullback`), once on the signed operands and once on their scales.  Like the forward scale this is a
# worst-case bound: `|got - ref| <= 1e-5 · S` elementwise is what an fp32 evaluation in any order keeps with room to spare.
_GELU_C, _GELU_A = np.sqrt(2.0 / np.pi), 0.044715


def _gelu_d1_d2(x):
    """first and second derivative of NNlib.gelu (tanh form)"""
    u, u1, u2 = _GELU_C * (x + _GELU_A * x ** 3), _GELU_C * (1.0 + 3.0 * _GELU_A * x ** 2), 6.0 * _GELU_C * _GELU_A * x
    t = np.tanh(u)
    s = 1.0 - t * t
    return 0.5 * (1.0 + t) + 0.5 * x * s * u1, s * u1 + 0.5 * x * (s * u2 - 2.0 * t * s * u1 * u1)


def act_grad(act, y, sy, z=None, sz=None):
    """(act', its scale) as the backward takes it: from the activation's OUTPUT y (scale sy) for identity / relu / tanh / sigmoid, from the
    pre-activation z (scale sz) for gelu.  Scale = |act'| + |d act' / d(y or z)| · s; relu's mask y > 0 has no first-order term (the callers keep
    their inputs away from the kink)."""
    if act == ACT_IDENTITY:
        one = np.ones_like(y)
        return one, one
    if act == ACT_RELU:
        m = (y > 0).astype(F64)
        return m, m
    if act == ACT_TANH:
        d = 1.0 - y * y
        return d, np.abs(d) + 2.0 * np.abs(y) * sy
    if act == ACT_SIGMOID:
        d = y * (1.0 - y)
        return d, np.abs(d) + np.abs(1.0 - 2.0 * y) * sy
    if act == ACT_GELU:
        d1, d2 = _gelu_d1_d2(z)
        return d1, np.abs(d1) + np.abs(d2) * sz
    raise ValueError(f"unknown activation {act}")


def _dense_pullback(X, SX, W, b, act, y, sy, g, sg):
    """One Dense y = act(X Wᵀ + b) on rows: (δ, dW [in][out] — the ABI's layout —, db, dX) and the four scales.  X, y, g: (T, ·) float64."""
    W = np.asarray(W, dtype=F64)
    aW = np.abs(W)
    z = sz = None
    if act == ACT_GELU:
        z, sz = X @ W.T + np.asarray(b, dtype=F64)[None, :], SX @ aW.T + np.abs(np.asarray(b, dtype=F64))[None, :]
    a, sa = act_grad(act, y, sy, z, sz)
    d, sd = g * a, sg * sa
    return (d, X.T @ d, d.sum(axis=0), d @ W), (sd, SX.T @ sd, sd.sum(axis=0), sd @ aW)


def _w0(a, T):
    """`nothing` / a zero-width tensor as a (T, 0) array"""
    return np.zeros((T, 0), dtype=F64) if a is None else np.asarray(a, dtype=F64)


BLOCK_GRAD_NAMES = tuple(f"grad.{fn}.{k}" for fn in ("edgefn", "nodefn", "graphfn") for k in ("dW", "db"))


def _block_pullback(p, csc, x, sx, y, sy, cot, scot):
    """One replica.  x, y, cot and their scales: triples of (T, d) float64 arrays (zero width for `nothing`).  Returns
    ((d_ef, d_nf, d_gf), {parameter gradient}), and the same pair of scales.  The edge level runs in row chunks."""
    colptr, rowval, node_off, edge_off = csc
    N, E, G = len(colptr) - 1, len(rowval), len(node_off) - 1
    dst = np.repeat(np.arange(N), np.diff(colptr))
    ng = np.repeat(np.arange(G), np.diff(node_off))
    eg = np.repeat(np.arange(G), np.diff(edge_off))
    de, dn, dg = p["in_dims"]
    oe, on, og = p["out_dims"]
    (ef, nf, gf), (sef, snf, sgf) = x, sx
    (he, hn, hg), (she, shn, shg) = y, sy
    cat = lambda parts: np.concatenate(parts, axis=1)
    # graph level
    Xg, SXg = cat([_segsum(he, eg, G), _segsum(hn, ng, G), gf]), cat([_segsum(she, eg, G), _segsum(shn, ng, G), sgf])
    (_, dWg, dbg, dXg), (_, sWg, sbg, sXg) = _dense_pullback(Xg, SXg, p["Wg"], p["bg"], p["act_g"], hg, shg, cot[2], scot[2])
    # node level
    Xn, SXn = cat([_segsum(he, dst, N), nf, gf[ng]]), cat([_segsum(she, dst, N), snf, sgf[ng]])
    gn_, sgn = cot[1] + dXg[ng][:, oe:oe + on], scot[1] + sXg[ng][:, oe:oe + on]
    (_, dWn, dbn, dXn), (_, sWn, sbn, sXn) = _dense_pullback(Xn, SXn, p["Wn"], p["bn"], p["act_n"], hn, shn, gn_, sgn)
    # edge level
    Ke = de + 2 * dn + dg
    acc = lambda: [np.zeros((E, de)), np.zeros((N, dn)), np.zeros((G, dg)), np.zeros((Ke, oe)), np.zeros(oe)]
    v, s = acc(), acc()
    for c0 in range(0, E, _CHUNK):
        c1 = min(E, c0 + _CHUNK)
        src_c, dst_c, eg_c = rowval[c0:c1], dst[c0:c1], eg[c0:c1]
        Xe, SXe = cat([ef[c0:c1], nf[src_c], nf[dst_c], gf[eg_c]]), cat([sef[c0:c1], snf[src_c], snf[dst_c], sgf[eg_c]])
        ge = cot[0][c0:c1] + dXg[eg_c][:, :oe] + dXn[dst_c][:, :oe]
        sge = scot[0][c0:c1] + sXg[eg_c][:, :oe] + sXn[dst_c][:, :oe]
        res = _dense_pullback(Xe, SXe, p["We"], p["be"], p["act_e"], he[c0:c1], she[c0:c1], ge, sge)
        for o, (_, dW, db, dX) in zip((v, s), res):
            o[0][c0:c1] = dX[:, :de]
            o[1] += _segsum(dX[:, de:de + dn], src_c, N) + _segsum(dX[:, de + dn:de + 2 * dn], dst_c, N)
            o[2] += _segsum(dX[:, de + 2 * dn:], eg_c, G)
            o[3] += dW
            o[4] += db
    outs = []
    for o, dXn_, dXg_, pw in ((v, dXn, dXg, (dWn, dbn, dWg, dbg)), (s, sXn, sXg, (sWn, sbn, sWg, sbg))):
        d_nf = o[1] + dXn_[:, oe:oe + dn]
        d_gf = o[2] + _segsum(dXn_[:, oe + dn:], ng, G) + dXg_[:, oe + on:]
        outs.append(((o[0], d_nf, d_gf), dict(zip(BLOCK_GRAD_NAMES, (o[3], o[4], *pw)))))
    return outs[0], outs[1]


def _pack_dx(per_replica, widths):
    return tuple(None if d == 0 else np.stack([q[k] for q in per_replica]) for k, d in enumerate(widths))


def block_backward_sparse(p, csc, x, y, cot, return_scale=True):
    """Pullback of block_forward_sparse as gnx_block_backward defines it: x = (ef, nf, gf) the forward inputs, y = (ef', nf', gf') the forward
    OUTPUTS AS GIVEN (at the ABI they are inputs: Xn and Xg are built from them and act' of tanh / sigmoid / relu is taken from them; a gelu
    level recomputes its pre-activation), cot the three cotangents; all packed [R][T][d], `None` for `nothing` / a zero width.  Returns the nine
    gradients {d_ef, d_nf, d_gf: [R][T][d] | None; grad.<fn>.dW: [in][out]; grad.<fn>.db} — parameter gradients summed over the replicas — and,
    with `return_scale`, the dict of their scales (see above; every input is handed to the call, so S_v = |v| throughout)."""
    rows = (len(csc[1]), len(csc[0]) - 1, len(csc[2]) - 1)
    R = next(a.shape[0] for a in (*x, *y, *cot) if a is not None)
    dxs, sdxs, grads, sgrads = [], [], None, None
    for r in range(R):
        tr = lambda trip: tuple(_w0(None if a is None else a[r], T) for a, T in zip(trip, rows))
        xr, yr, cr = tr(x), tr(y), tr(cot)
        ab = lambda trip: tuple(np.abs(a) for a in trip)
        (dx, gr), (sdx, sgr) = _block_pullback(p, csc, xr, ab(xr), yr, ab(yr), cr, ab(cr))
        dxs.append(dx); sdxs.append(sdx)
        grads = gr if grads is None else {k: grads[k] + gr[k] for k in gr}
        sgrads = sgr if sgrads is None else {k: sgrads[k] + sgr[k] for k in sgr}
    val = dict(zip(("d_ef", "d_nf", "d_gf"), _pack_dx(dxs, p["in_dims"])), **grads)
    if not return_scale:
        return val
    return val, dict(zip(("d_ef", "d_nf", "d_gf"), _pack_dx(sdxs, p["in_dims"])), **sgrads)


def _ln_pullback(x, sx, gamma, eps, eps_mode, g, sg):
    """Pullback of layernorm(x) = γ x̂ + β over the last axis: (dx, dγ, dβ) and their scales.  With dx̂ = g γ and r = den / σ (eps_mode 0) or 1
    (eps_mode 1): dx = (dx̂ - mean(dx̂) - x̂ · mean(dx̂ x̂) · r) / den.  Scales: the same expression with every term's absolute value added,
    and layernorm_scale(γ = 1, β = 0) for the recomputed x̂."""
    gamma = np.asarray(gamma, dtype=F64)
    mu = x.mean(axis=-1, keepdims=True)
    xc = x - mu
    var = (xc ** 2).mean(axis=-1, keepdims=True)
    den = (np.sqrt(var) + eps) if eps_mode == 0 else np.sqrt(var + eps)
    r = den / np.sqrt(var) if eps_mode == 0 else 1.0
    xhat = xc / den
    sxhat = layernorm_scale(x, sx, np.ones_like(gamma), np.zeros_like(gamma), eps, eps_mode).astype(F64)
    dxh, sdxh = g * gamma, sg * np.abs(gamma)
    dx = (dxh - dxh.mean(axis=-1, keepdims=True) - xhat * (dxh * xhat).mean(axis=-1, keepdims=True) * r) / den
    sdx = (sdxh + sdxh.mean(axis=-1, keepdims=True) + sxhat * (sdxh * sxhat).mean(axis=-1, keepdims=True) * r) / den
    flat = lambda a: a.reshape(-1, a.shape[-1])
    return (dx, flat(g * xhat).sum(axis=0), flat(g).sum(axis=0)), (sdx, flat(sg * sxhat).sum(axis=0), flat(sg).sum(axis=0))


def core_backward_sparse(p, csc, x, cot, return_scale=True, hidden_act=None):
    """Pullback of core_forward_sparse, y = x + block(gn1(x)) + ffwd(gn2(x)), as gnx_core_backward defines it: x and cot are the three packed
    [R][T][d] inputs and cotangents; everything else is recomputed.  `hidden_act`: the FeedForwards' hidden activation (default p["hidden_act"],
    else relu as in the forward oracle); tanh takes act' from the recomputed hidden units, gelu from the recomputed pre-activation.  Returns the
    33 gradients {d_ef, d_nf, d_gf, grad.<fn>.dW/db (block), grad.ln1_<t>/ln2_<t>.gamma/beta, grad.ff_<t>.fc1/fc2.dW/db} and their scales."""
    act = p.get("hidden_act", ACT_RELU) if hidden_act is None else hidden_act
    xs = [np.asarray(v, dtype=F64) for v in x]
    gs = [np.asarray(v, dtype=F64) for v in cot]
    sxs, sgs = [np.abs(v) for v in xs], [np.abs(v) for v in gs]
    eps, em = p["eps"], p["eps_mode"]
    R = xs[0].shape[0]
    val, sc = {}, {}
    dx, sdx = [g.copy() for g in gs], [s.copy() for s in sgs]  # the residual
    # FeedForward and gn2
    for i, t in enumerate("eng"):
        g2, b2 = p[f"ln2_{t}_gamma"], p[f"ln2_{t}_beta"]
        d = xs[i].shape[-1]
        l2 = layernorm(xs[i], g2, b2, eps, em, axis=-1).reshape(-1, d)
        sl2 = layernorm_scale(xs[i], sxs[i], g2, b2, eps, em).astype(F64).reshape(-1, d)
        W1, b1, W2, b2_ = p[f"ff_{t}_W1"], p[f"ff_{t}_b1"], p[f"ff_{t}_W2"], p[f"ff_{t}_b2"]
        g, sg = gs[i].reshape(-1, d), sgs[i].reshape(-1, d)
        dl2, sdl2 = np.empty_like(l2), np.empty_like(l2)
        tot = None
        for c0 in range(0, l2.shape[0], _CHUNK):
            c1 = min(l2.shape[0], c0 + _CHUNK)
            h = _dense_rows(W1, b1, act, l2[c0:c1])
            sh = sl2[c0:c1] @ np.abs(np.asarray(W1, dtype=F64)).T + np.abs(np.asarray(b1, dtype=F64))[None, :]
            one = np.ones_like(g[c0:c1])
            (dh_, dW2, db2, dh), (sdh_, sW2, sb2, sdh) = _dense_pullback(h, sh, W2, b2_, ACT_IDENTITY, one, one, g[c0:c1], sg[c0:c1])
            (_, dW1, db1, dl2[c0:c1]), (_, sW1, sb1, sdl2[c0:c1]) = _dense_pullback(l2[c0:c1], sl2[c0:c1], W1, b1, act, h, sh, dh, sdh)
            part = [dW1, db1, dW2, db2, sW1, sb1, sW2, sb2]
            tot = part if tot is None else [a + b for a, b in zip(tot, part)]
        for k, n in enumerate(("fc1.dW", "fc1.db", "fc2.dW", "fc2.db")):
            val[f"grad.ff_{t}.{n}"], sc[f"grad.ff_{t}.{n}"] = tot[k], tot[4 + k]
        (d2, dgam, dbet), (sd2, sgam, sbet) = _ln_pullback(xs[i], sxs[i], g2, eps, em, dl2.reshape(xs[i].shape), sdl2.reshape(xs[i].shape))
        dx[i] += d2; sdx[i] += sd2
        val[f"grad.ln2_{t}.gamma"], val[f"grad.ln2_{t}.beta"], sc[f"grad.ln2_{t}.gamma"], sc[f"grad.ln2_{t}.beta"] = dgam, dbet, sgam, sbet
    # block and gn1
    l1 = [layernorm(xs[i], p[f"ln1_{t}_gamma"], p[f"ln1_{t}_beta"], eps, em, axis=-1) for i, t in enumerate("eng")]
    sl1 = [layernorm_scale(xs[i], sxs[i], p[f"ln1_{t}_gamma"], p[f"ln1_{t}_beta"], eps, em).astype(F64) for i, t in enumerate("eng")]
    yb, syb = block_forward_sparse(p["block"], csc, *l1, return_scale=True, in_scale=tuple(sl1))
    dl1, sdl1, grads, sgrads = [], [], None, None
    for r in range(R):
        pick = lambda trip: tuple(np.asarray(a[r], dtype=F64) for a in trip)
        (d1, gr), (sd1, sgr) = _block_pullback(p["block"], csc, pick(l1), pick(sl1), pick(yb), pick(syb), pick(gs), pick(sgs))
        dl1.append(d1); sdl1.append(sd1)
        grads = gr if grads is None else {k: grads[k] + gr[k] for k in gr}
        sgrads = sgr if sgrads is None else {k: sgrads[k] + sgr[k] for k in sgr}
    val.update(grads); sc.update(sgrads)
    for i, t in enumerate("eng"):
        g1 = np.stack([q[i] for q in dl1])
        sg1 = np.stack([q[i] for q in sdl1])
        (d1, dgam, dbet), (sd1, sgam, sbet) = _ln_pullback(xs[i], sxs[i], p[f"ln1_{t}_gamma"], eps, em, g1, sg1)
        dx[i] += d1; sdx[i] += sd1
        val[f"grad.ln1_{t}.gamma"], val[f"grad.ln1_{t}.beta"], sc[f"grad.ln1_{t}.gamma"], sc[f"grad.ln1_{t}.beta"] = dgam, dbet, sgam, sbet
    for n, d_, s_ in zip(("d_ef", "d_nf", "d_gf"), dx, sdx):
        val[n], sc[n] = d_, s_
    return (val, sc) if return_scale else val


LN_TOKENS = {"ln": "layernorm", "ln_sqrt": "layernorm_sqrt_eps"}  # width token -> marker string of the layer tuple
LN_SQRT_EPS = LN_TOKENS["ln_sqrt"]
CHAIN_LN_EPS = 1e-5  # Flux's default, the only value the ABI has for a Chain's LayerNorm


def ln_eps_mode(marker):
    """eps mode of a chain's LayerNorm layer tuple (marker, gamma, beta): 0 = (x - mean) / (sigma + eps), 1 = / sqrt(sigma^2 + eps)"""
    assert marker in LN_TOKENS.values(), marker
    return 1 if marker == LN_SQRT_EPS else 0


def make_chain_block_params(rng, in_dims, edge_widths, node_widths, graph_widths, acts=(ACT_RELU, ACT_TANH, ACT_IDENTITY), last_acts=None):
    """GNBlock whose update functions are Chains of Dense layers (gnblock.jl:1-6 allows any Chain; the default is one Dense):
    `*_widths` = output widths of the layers of each chain (empty = that output is `nothing`); hidden layers use `acts[i % 3]`,
    the last layer of a chain is linear (like the reference's default) unless `last_acts` = (edge, node, graph) names its activation.
    A width entry "ln" puts a Flux `LayerNorm(d)` layer value there (d = the width in front of it; random gamma / beta): the layer tuple is
    ("layernorm", gamma, beta); the entry "ln_sqrt" the same in the sqrt-eps mode, / sqrt(sigma^2 + eps): ("layernorm_sqrt_eps", gamma, beta).
    Neither `last_acts` nor the mode draws anything: every seed gives the numbers it gave without them."""
    de, dn, dg = in_dims
    # (a LayerNorm keeps the width in front of it; a chain of LayerNorms alone keeps its input's)
    last = lambda ws, k: next((w for w in reversed(ws) if not isinstance(w, str)), k if ws else 0)
    oe = last(edge_widths, de + 2 * dn + dg)
    on = last(node_widths, oe + dn + dg)
    kin = dict(edge=de + 2 * dn + dg, node=oe + dn + dg, graph=oe + on + dg)
    p = dict(in_dims=tuple(in_dims))
    for t, (name, widths) in enumerate((("edge", edge_widths), ("node", node_widths), ("graph", graph_widths))):
        layers, k = [], kin[name]
        for i, w in enumerate(widths):
            if isinstance(w, str):
                layers.append((LN_TOKENS[w], rng.uniform(0.5, 1.5, size=k).astype(np.float32), rng.uniform(-0.2, 0.2, size=k).astype(np.float32)))
                continue
            act = acts[i % len(acts)] if i + 1 < len(widths) else (ACT_IDENTITY if last_acts is None else last_acts[t])
            layers.append((glorot_uniform(rng, w, k), rng.uniform(-0.1, 0.1, size=w).astype(np.float32), act))
            k = w
        p[name] = layers
    return p


def chain_block_forward_sparse(p, csc, ef, nf, gf, return_scale=False):
    """(m::GNBlock)(x) (gnblock.jl:63-69) with Chain update functions, on packed data: every chain is applied to the same
    function inputs as in block_forward_sparse (edgefninput.jl / nodefninput.jl / graphfninput.jl), layer after layer.
    Scales (worst case, as block_forward_sparse): |W|·S + |b| through every layer."""
    colptr, rowval, node_off, edge_off = csc
    N, E, G = len(colptr) - 1, len(rowval), len(node_off) - 1
    R = next(a.shape[0] for a in (ef, nf, gf) if a is not None)
    dst = np.repeat(np.arange(N), np.diff(colptr))
    node_graph = np.repeat(np.arange(G), np.diff(node_off))
    edge_graph = np.repeat(np.arange(G), np.diff(edge_off))

    def run(layers, X, S):
        for W, b, act in layers:
            if isinstance(W, str):  # ("layernorm", gamma, beta): a Flux LayerNorm(d) layer value between the Dense layers (gnblock.jl:1-6 admits any Chain)
                S = layernorm_scale(X, S, b, act, CHAIN_LN_EPS, ln_eps_mode(W))
                X = layernorm(X, b, act, CHAIN_LN_EPS, ln_eps_mode(W), axis=-1)
                continue
            S = np.abs(S) @ np.abs(np.asarray(W, dtype=F64)).T + np.abs(np.asarray(b, dtype=F64))[None, :]
            X = _dense_rows(W, b, act, X)
        return X, S

    outs, scales = ([], [], []), ([], [], [])
    for r in range(R):
        parts = []
        if ef is not None:
            parts.append(np.asarray(ef[r], dtype=F64))
        if nf is not None:
            nfr = np.asarray(nf[r], dtype=F64)
            parts += [nfr[rowval], nfr[dst]]
        if gf is not None:
            gfr = np.asarray(gf[r], dtype=F64)
            parts.append(gfr[edge_graph])
        Xe = np.concatenate(parts, axis=1)
        he, se = run(p["edge"], Xe, np.abs(Xe)) if p["edge"] else (None, None)
        hn = sn = hg = sg = None
        if p["node"]:
            # (a chain without layers = a zero-width output: an empty segment of the next input, as the reference's 0-row arrays, gnblock.jl:63-69)
            parts, sparts = ([_segsum(he, dst, N)], [_segsum(se, dst, N)]) if he is not None else ([], [])
            if nf is not None:
                parts.append(nfr); sparts.append(np.abs(nfr))
            if gf is not None:
                parts.append(gfr[node_graph]); sparts.append(np.abs(gfr[node_graph]))
            hn, sn = run(p["node"], np.concatenate(parts, axis=1), np.concatenate(sparts, axis=1))
        if p["graph"]:
            parts, sparts = [], []
            if he is not None:
                parts.append(_segsum(he, edge_graph, G)); sparts.append(_segsum(se, edge_graph, G))
            if hn is not None:
                parts.append(_segsum(hn, node_graph, G)); sparts.append(_segsum(sn, node_graph, G))
            if gf is not None:
                parts.append(gfr); sparts.append(np.abs(gfr))
            hg, sg = run(p["graph"], np.concatenate(parts, axis=1), np.concatenate(sparts, axis=1))
        for lst, v in zip(outs, (he, hn, hg)):
            lst.append(v)
        for lst, v in zip(scales, (se, sn, sg)):
            lst.append(v)
    pack = lambda ls: tuple(None if (lst[0] is None or lst[0].shape[1] == 0) else np.stack(lst) for lst in ls)
    return (pack(outs), pack(scales)) if return_scale else pack(outs)


def _act_prime_z(act, z):
    """|d act / dz| at the pre-activation z"""
    if act == ACT_IDENTITY:
        return np.ones_like(z)
    if act == ACT_RELU:
        return (z > 0).astype(F64)
    if act == ACT_TANH:
        return 1.0 - np.tanh(z) ** 2
    if act == ACT_SIGMOID:
        y = apply_act(z, act)
        return y * (1.0 - y)
    return np.abs(_gelu_d1_d2(z)[0])


def _chain_tape(layers, X, S, first_order=False):
    """chain_block_forward_sparse's `run`, keeping every layer's input and output with their scales: [(X, SX, y, Sy, Sn)], and the chain's output.
    Sy is the forward's own scale (a Dense: SX |W|^T + |b|, the scale of its pre-activation z, for any activation).  `first_order`: the scale
    handed to the NEXT layer is |y| + |act'(z)| (Sz - |z|) instead — the output's own rounding plus the first-order share of its
    pre-activation's error —, which is what Sz is for the identity and never more than Sz + |y| - |act' z|."""
    tape = []
    for W, b, act in layers:
        if isinstance(W, str):
            Sy = layernorm_scale(X, S, b, act, CHAIN_LN_EPS, ln_eps_mode(W)).astype(F64)
            y = layernorm(X, b, act, CHAIN_LN_EPS, ln_eps_mode(W), axis=-1)
            Sn = Sy
        else:
            Sy = np.abs(S) @ np.abs(np.asarray(W, dtype=F64)).T + np.abs(np.asarray(b, dtype=F64))[None, :]
            y = _dense_rows(W, b, act, X)
            Sn = Sy
            if first_order and act != ACT_IDENTITY:
                z = X @ np.asarray(W, dtype=F64).T + np.asarray(b, dtype=F64)[None, :]
                Sn = np.abs(y) + _act_prime_z(act, z) * (Sy - np.abs(z))
        tape.append((X, S, y, Sy, Sn))
        X, S = y, Sn
    return tape, X, S


def _prod1(a, sa, b, sb):
    """first-order scale of a product: |a b| (its own rounding) + |a| (Sb - |b|) + (Sa - |a|) |b|"""
    return np.abs(a) * sb + (sa - np.abs(a)) * np.abs(b)


def _dense_pullback1(X, SX, W, b, act, y, sy, sz, g, sg):
    """`_dense_pullback` with FIRST-ORDER scales: every product a . b contributes |a| Sb + Sa |b| - |a b| instead of Sa . Sb (the term dropped,
    (Sa - |a|)(Sb - |b|), is second order: 1e-5 of it is below 1e-5 . 1e-5 . Sa . Sb).  In a pullback through L layers and three levels the
    product rule multiplies the factors S / |value| of every recomputed operand — each about the number of terms of the sum behind it — and on
    a batch with sums over thousands of edges reaches 1e27 times the value; the first-order rule adds them.  sy: the scale of the layer's
    OUTPUT (first-order: |y| + |act'| (Sz - |z|)), sz: of its pre-activation."""
    W = np.asarray(W, dtype=F64)
    aW = np.abs(W)
    z = X @ W.T + np.asarray(b, dtype=F64)[None, :] if act == ACT_GELU else None
    a, sa = act_grad(act, y, sy, z, sz)
    d, sd = g * a, _prod1(g, sg, a, sa)
    sdW = np.abs(X).T @ sd + (SX - np.abs(X)).T @ np.abs(d)
    return (d, X.T @ d, d.sum(axis=0), d @ W), (sd, sdW, sd.sum(axis=0), sd @ aW)


def _ln_pullback1(x, sx, gamma, eps, eps_mode, g, sg):
    """`_ln_pullback` with first-order scales (see `_dense_pullback1`): with u = dxh - mean(dxh) - xhat c r, c = mean(dxh xhat), dx = u / den;
    the deviation's error is layernorm_scale's q (relative q / den on 1 / den)."""
    gamma = np.asarray(gamma, dtype=F64)
    mu = x.mean(axis=-1, keepdims=True)
    xc = x - mu
    var = (xc ** 2).mean(axis=-1, keepdims=True)
    den = (np.sqrt(var) + eps) if eps_mode == 0 else np.sqrt(var + eps)
    r = den / np.sqrt(var) if eps_mode == 0 else 1.0
    xhat = xc / den
    sxhat = layernorm_scale(x, sx, np.ones_like(gamma), np.zeros_like(gamma), eps, eps_mode).astype(F64)
    sc = sx + sx.mean(axis=-1, keepdims=True)
    q = np.sqrt((sc ** 2).mean(axis=-1, keepdims=True))
    m = lambda v: v.mean(axis=-1, keepdims=True)
    dxh, sdxh = g * gamma, sg * np.abs(gamma)
    c, s_c = m(dxh * xhat), m(_prod1(dxh, sdxh, xhat, sxhat))
    u = dxh - m(dxh) - xhat * c * r
    su = sdxh + m(sdxh) + r * _prod1(xhat, sxhat, c, s_c)
    dx, sdx = u / den, (su + np.abs(u) * (q / den)) / den
    flat = lambda a: a.reshape(-1, a.shape[-1])
    return (dx, flat(g * xhat).sum(axis=0), flat(g).sum(axis=0)), (sdx, flat(_prod1(g, sg, xhat, sxhat)).sum(axis=0), flat(sg).sum(axis=0))


def _chain_pullback(layers, tape, g, sg, first_order=False):
    """The pullback of one Chain on rows from the cotangent g of its output: (dX of the chain's input, [(dW | dgamma, db | dbeta)] per layer), and
    the same pair of scales — `_dense_pullback` / `_ln_pullback` layer by layer (`first_order`: their first-order forms), every recomputed
    layer input and output at its forward scale."""
    grads, sgrads = [None] * len(layers), [None] * len(layers)
    for i in range(len(layers) - 1, -1, -1):
        W, b, act = layers[i]
        X, SX, y, Sy, Sn = tape[i]
        if isinstance(W, str):
            (g, dgam, dbet), (sg, sgam, sbet) = (_ln_pullback1 if first_order else _ln_pullback)(X, SX, b, CHAIN_LN_EPS, ln_eps_mode(W), g, sg)
            grads[i], sgrads[i] = (dgam, dbet), (sgam, sbet)
        else:
            if first_order:
                (_, dW, db, g), (_, sW, sb, sg) = _dense_pullback1(X, SX, W, b, act, y, Sn, Sy, g, sg)
            else:
                (_, dW, db, g), (_, sW, sb, sg) = _dense_pullback(X, SX, W, b, act, y, Sy, g, sg)
            grads[i], sgrads[i] = (dW, db), (sW, sb)
    return (g, grads), (sg, sgrads)


def chain_block_tapes(p, csc, ef, nf, gf, first_order=False):
    """One replica of chain_block_forward_sparse with every layer kept: ef, nf, gf (T, d) float64 arrays (zero width for `nothing`).  Returns
    ((edge, node, graph) tapes — per layer (X, SX, y, Sy, Sn), for a Dense Sy = SX |W|^T + |b| is the scale of its pre-activation, Sn the scale the next layer is handed
    (`_chain_tape`) —, (he, hn, hg))."""
    colptr, rowval, node_off, edge_off = csc
    N, E, G = len(colptr) - 1, len(rowval), len(node_off) - 1
    dst = np.repeat(np.arange(N), np.diff(colptr))
    ng = np.repeat(np.arange(G), np.diff(node_off))
    eg = np.repeat(np.arange(G), np.diff(edge_off))
    cat = lambda parts: np.concatenate(parts, axis=1)
    Xe = cat([ef, nf[rowval], nf[dst], gf[eg]])
    te, he, she = _chain_tape(p["edge"], Xe, np.abs(Xe), first_order)
    if not p["edge"]:  # (a chain without layers = a zero-width output)
        he, she = np.zeros((E, 0)), np.zeros((E, 0))
    Xn = cat([_segsum(he, dst, N), nf, gf[ng]])
    tn, hn, shn = _chain_tape(p["node"], Xn, cat([_segsum(she, dst, N), np.abs(nf), np.abs(gf[ng])]), first_order)
    if not p["node"]:
        hn, shn = np.zeros((N, 0)), np.zeros((N, 0))
    Xg = cat([_segsum(he, eg, G), _segsum(hn, ng, G), gf])
    tg, hg, _ = _chain_tape(p["graph"], Xg, cat([_segsum(she, eg, G), _segsum(shn, ng, G), np.abs(gf)]), first_order)
    return (te, tn, tg), (he, hn, hg)


def chain_block_backward_sparse(p, csc, x, cot, return_scale=True, first_order=True):
    """Pullback of chain_block_forward_sparse as gnx_chain_block_backward defines it: x = (ef, nf, gf) the forward inputs and cot the three
    cotangents, packed [R][T][d] with `None` for `nothing`; everything between the inputs and the outputs is recomputed.  Returns {d_ef, d_nf, d_gf:
    [R][T][d] | None; "<fn><i>.dW": [in][out] of a Dense, gamma's gradient of a LayerNorm; "<fn><i>.db": the bias's, beta's} for fn in edge, node,
    graph — parameter gradients summed over the replicas — and, with `return_scale`, the dict of their scales (see `Pullbacks` above: a tensor
    handed to the call has S = |v|, a recomputed one the forward's scale).  The routing between the levels is `_block_pullback`'s.
    `first_order` (the default): the scales of `_dense_pullback1` / `_ln_pullback1` — never above those of the product rule (`first_order=False`:
    `_dense_pullback` / `_ln_pullback` as the block and the core use them), which on a chain is vacuous; tests/test_chain_bw_stress_cpu.py
    asserts both S >= |value| and first-order S <= product S on every case."""
    colptr, rowval, node_off, edge_off = csc
    N, E, G = len(colptr) - 1, len(rowval), len(node_off) - 1
    dst = np.repeat(np.arange(N), np.diff(colptr))
    ng = np.repeat(np.arange(G), np.diff(node_off))
    eg = np.repeat(np.arange(G), np.diff(edge_off))
    de, dn, dg = p["in_dims"]
    rows = (E, N, G)
    R = next(a.shape[0] for a in (*x, *cot) if a is not None)
    dxs, sdxs, val, sc = [], [], {}, {}
    for r in range(R):
        ef, nf, gf = (_w0(None if a is None else a[r], T) for a, T in zip(x, rows))
        (te, tn, tg), (he, hn, hg) = chain_block_tapes(p, csc, ef, nf, gf, first_order)
        oe, on = he.shape[1], hn.shape[1]
        ce, cn, cg = (_w0(None if a is None else a[r], T) for a, T in zip(cot, rows))
        # graph level
        dXg, sXg = np.zeros((G, oe + on + dg)), np.zeros((G, oe + on + dg))
        gr = {}
        if p["graph"]:
            cg = cg if cg.shape[1] else np.zeros((G, hg.shape[1]))  # (no cotangent for an output: zeros)
            (dXg, gr["graph"]), (sXg, sgg) = _chain_pullback(p["graph"], tg, cg, np.abs(cg), first_order)
        # node level
        dXn, sXn = np.zeros((N, oe + dn + dg)), np.zeros((N, oe + dn + dg))
        if p["node"]:
            cn = cn if cn.shape[1] else np.zeros((N, on))
            (dXn, gr["node"]), (sXn, sgn) = _chain_pullback(p["node"], tn, cn + dXg[ng][:, oe:oe + on], np.abs(cn) + sXg[ng][:, oe:oe + on], first_order)
        # edge level
        dXe, sXe = np.zeros((E, de + 2 * dn + dg)), np.zeros((E, de + 2 * dn + dg))
        if p["edge"]:
            ce = ce if ce.shape[1] else np.zeros((E, oe))
            (dXe, gr["edge"]), (sXe, sge) = _chain_pullback(p["edge"], te, ce + dXg[eg][:, :oe] + dXn[dst][:, :oe], np.abs(ce) + sXg[eg][:, :oe] + sXn[dst][:, :oe], first_order)
        sgr = dict(graph=sgg if p["graph"] else None, node=sgn if p["node"] else None, edge=sge if p["edge"] else None)
        outs = []
        for dXe_, dXn_, dXg_ in ((dXe, dXn, dXg), (sXe, sXn, sXg)):
            d_nf = _segsum(dXe_[:, de:de + dn], rowval, N) + _segsum(dXe_[:, de + dn:de + 2 * dn], dst, N) + dXn_[:, oe:oe + dn]
            d_gf = _segsum(dXe_[:, de + 2 * dn:], eg, G) + _segsum(dXn_[:, oe + dn:], ng, G) + dXg_[:, oe + on:]
            outs.append((dXe_[:, :de], d_nf, d_gf))
        dxs.append(outs[0]); sdxs.append(outs[1])
        for name in ("edge", "node", "graph"):
            for i in range(len(p[name])):
                for k, which in enumerate(("dW", "db")):
                    n = f"{name}{i}.{which}"
                    val[n] = gr[name][i][k] + (val[n] if n in val else 0.0)
                    sc[n] = sgr[name][i][k] + (sc[n] if n in sc else 0.0)
    val.update(zip(("d_ef", "d_nf", "d_gf"), _pack_dx(dxs, p["in_dims"])))
    sc.update(zip(("d_ef", "d_nf", "d_gf"), _pack_dx(sdxs, p["in_dims"])))
    return (val, sc) if return_scale else val


# ----------------------------------------------------------------------------------------------------------
# Layout bridges between the two forms
# ----------------------------------------------------------------------------------------------------------
def packed_from_julia_shared(a):
    """Julia (D, T, B) → C-ABI (B, T, D).  Same bytes when `a` is column-major."""
    return None if a is None else np.ascontiguousarray(np.transpose(np.asarray(a), (2, 1, 0)))


def packed_from_julia_vector(items):
    """Vector of (D, T_g) → (1, ΣT, D); vector of (D,) → (1, G, D)."""
    if items is None:
        return None
    items = [np.asarray(x) for x in items]
    if items[0].ndim == 1:
        return np.stack(items)[None]
    return np.concatenate([x.T for x in items], axis=0)[None]


def flat_from_dense(x, key):
    """flatunpaddednf/ef (views.jl:80-98): (D, ΣT) in graph-major order from the padded arrays."""
    g = x["graphs"]
    a = x[key]
    flat = a.reshape(a.shape[0], -1, order="F")
    mask = g.flat_node_unpadder if key == "nf" else g.flat_edge_unpadder
    return flat[:, mask]
