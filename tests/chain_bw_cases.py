"""The cases, references and expected kernels of the Chain pullbacks' stress: shared by tests/test_chain_bw_stress_cpu.py (no GPU: the oracle's values,
the soundness of the bar on every case, the controls), tests/chain_bw_stress_child.py (runs the cases on the device) and
tests/test_gpu_chain_bw_stress.py (compares on the CPU).  Nothing here touches the device or the library.  The comparisons are those of
tests/bw_x6_cases.py (`ratios`, `check_elementwise`, `check_statistical`, `legacy_close`): |got - ref| <= 1e-5 . S for every element.

THE BATCH: G = 131 graphs, N = 1031 nodes, E = 4099 edges, none a multiple of 64.  131 = 2 . 64 + 3: the graph level of the fused pullback
(k_chain_mlp_bw<., SRC_ROWS>) has two full waves and a wave of 3 rows — in a 4-wave workgroup a fourth wave past the end (`c0 < f.rows` false), in
a 2-wave workgroup a second workgroup with such a wave.  Graph 0 is large and has a hub of more than 128 in-edges, graph 1 has no edges, graph 2
is one node with its self loop, graph 3 is ordinary but for a node without in-edges; `batch()` asserts all of it.
ONE EXCEPTION: the ABI takes replicas (R > 1) on a batch of ONE graph only (csrc/gnx_chain.cpp: check_params), so N-R2 runs on the one graph of
tests/bw_x6_cases.py — 1031 nodes and 4099 edges as well, the same row counts per replica at the edge and node levels.

A case is a dict (id, family, in_dims, the three chains' widths, hidden activations, last-layer activations, R, variant); `data(cid)` draws it —
seeded by the id's position, the same in every process — and `reference(cid)` evaluates, once per process, the float64 oracle with its scale S
(oracle/gn_oracle.py: chain_block_backward_sparse) and the YARDSTICK: the same pullback by plain torch float32 autograd of
tests/chain_torch.py's _torch_chain_block on the CPU.  `forward_reference(cid)` is chain_block_forward_sparse with its scale.

Relu appears in N-relu alone, and there no row is left out: the inputs are redrawn row by row until every relu pre-activation of the float64
forward is further than U.KINK_MARGIN . U.RTOL . S_z from the kink.  No case has a LayerNorm over fewer than 3 elements
(tests/test_gpu_chain_bw_narrow.py::test_tiny_layernorms pins those and says why they have no reference)."""
import functools

import numpy as np
import torch

from oracle import gn_oracle as O
from tests import bw_x6_cases as BC
from tests import util as U
from tests.test_chain_bw_narrow_abi import formula_takes
from tests.chain_torch import _torch_chain_block

N_GRAPHS, N_NODES, N_EDGES, BATCH_SEED = 131, 1031, 4099, 17
CHAIN_BAR = 1e-3  # the legacy normwise bar of tests/test_gpu_chain.py: bar . max(1, max|ref|)
DX = ("d_ef", "d_nf", "d_gf")
FN = ("edge", "node", "graph")
F64, F32 = torch.float64, torch.float32
LN, LNS = "ln", "ln_sqrt"
T_, S_, G_, I_, R_ = O.ACT_TANH, O.ACT_SIGMOID, O.ACT_GELU, O.ACT_IDENTITY, O.ACT_RELU
SMOOTH = (T_, S_, I_)


def _case(cid, family, in_dims, ew, nw, gw, acts=SMOOTH, last=None, R=1, variant="plain", mask=None):
    return dict(id=cid, family=family, in_dims=in_dims, widths=(ew, nw, gw), acts=acts, last=last, R=R, variant=variant,
                mask=(7 if family == "narrow" else 0) if mask is None else mask)


W1632 = ((10, 5, 3), [16, 3], [8, 4], [6, 5])
LNBOTH = ((3, 2, 1), [9, LNS, 17, LN, 4], [16, LN, 5, LNS], [LNS, 9, 4, LN])  # every function: both eps modes; LayerNorm as first and as last layer
WPLAIN = ((40, 24, 8), [128, 64], [64, LN, 32], [33, 12])
ANY_MASK_CASE = ((8, 8, 8), [32, LN, 32, 32, 7], [LN, 32, 32, 9], [32, LN, 17, 4])  # the widths of tests/test_gpu_chain_bw_narrow.py's ANY_MASK_CASE
CASES = [
    _case("N-w8", "narrow", (2, 2, 1), [8, 8, 1], [3], [2]),                                   # every function in WMAX = 8
    _case("N-w16-32", "narrow", *W1632),                                                       # K_e = 23: WMAX = 32 edge, 16 node and graph
    _case("N-ln-both-modes", "narrow", *LNBOTH, acts=(T_, S_, T_)),                            # op 5 and op 6
    _case("N-last-act", "narrow", *W1632, last=(T_, S_, G_)),                                  # the last layer's act_grad_bw; gelu last (graph)
    _case("N-last-act-gelu-edge", "narrow", *W1632, last=(G_, T_, S_)),                        # ... the second parameter set: gelu last on the edge chain
    _case("N-gelu-hidden", "narrow", (10, 5, 3), [16, LN, 8, 3], [8, LNS, 6, 4], [6, 5], acts=(G_, G_, G_)),  # gelu in front of and behind a LayerNorm
    _case("N-relu", "narrow", *W1632, acts=(R_, R_, I_), variant="kinkfree"),
    # gridDim.y = 2, k_bw_dw_final over R . nwg (one graph).  The graph function's input is a sum over all 4099 edges and 1031 nodes: its first
    # layer's weight columns for the two sums are divided by E and N (a mean folded into the weights), or tanh saturates and the level's gradients are 0
    _case("N-R2", "narrow", *W1632, R=2, variant="mean_graph_input"),
    _case("N-log_uniform_cotangents", "narrow", *W1632, variant="log_uniform_cotangents"),
    _case("N-log_uniform_inputs", "narrow", *LNBOTH, acts=(T_, S_, T_), variant="log_uniform_inputs"),
    _case("N-cancelling_dW", "narrow", *W1632, acts=(I_, I_, I_), variant="cancelling_dW"),
    # cotangents at the edge level alone, so that a row's d_ef is its own cotangent's and small rows stay small (control c of the CPU tests)
    _case("N-log_uniform_edge_cotangents", "narrow", *W1632, variant="log_uniform_edge_cotangents"),
    # an edge function alone whose first layer is a sqrt-eps LayerNorm over three log-uniform features: rows whose deviation is below sqrt(eps), where
    # the two eps modes differ by a factor, in front of a layer whose inputs and cotangents are exact (control a of the CPU tests)
    _case("N-ln-sqrt-first", "narrow", (3, 0, 0), [LNS, 4], [], [], variant="log_uniform_inputs", mask="formula"),
    # tests/test_gpu_chain_bw_narrow.py's ANY_MASK_CASE with smooth activations (relu is N-relu's alone) and a narrower node chain: as it stands the
    # rule gives that case mask 0 — nothing fused — on any row counts; with the node chain ["ln", 16, 9] the call is part fused, part generic
    # (mask 2: the fused node level reads the generic forward's ef' and the generic graph level's dXg, the generic edge level reads its dXn)
    _case("N-mixed", "narrow", ANY_MASK_CASE[0], ANY_MASK_CASE[1], [LN, 16, 9], ANY_MASK_CASE[3], mask="formula"),
    _case("W-plain", "wide", *WPLAIN),
    _case("W-tails", "wide", (40, 24, 8), [37, LNS, 35], [132, 20], [36, 12]),
    _case("W-gelu-last-act", "wide", (40, 24, 8), [64, 36], [36, 20], [36, 12], acts=(G_, G_, G_), last=(T_, G_, G_)),
    _case("W-log_uniform_cotangents", "wide", *WPLAIN, variant="log_uniform_cotangents"),
    _case("W-log_uniform_weights", "wide", *WPLAIN, variant="log_uniform_weights"),
    _case("W-cancelling_dW", "wide", *WPLAIN, acts=(I_, I_, I_), variant="cancelling_dW"),
]
CASE_IDS = [c["id"] for c in CASES]
NARROW_IDS = [c["id"] for c in CASES if c["family"] == "narrow"]
CASE = {c["id"]: c for c in CASES}
ENTRIES = ("generic", "narrow")


def entries(cid):
    """the backward (and forward) entries a case runs through"""
    return ENTRIES if CASE[cid]["family"] == "narrow" else ENTRIES[:1]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the batch
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pairs_csc(n, src, dst):
    k = np.unique(dst.astype(np.int64) * n + src.astype(np.int64))
    dst, src = k // n, k % n
    colptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(colptr, dst + 1, 1)
    return np.cumsum(colptr), src.astype(np.int64)


def _exact_csc(rng, n, e):
    """exactly e distinct directed pairs of an n-node graph (self loops allowed), in the reference's edge order"""
    assert 0 <= e <= n * n
    k = rng.permutation(n * n)[:e]
    return _pairs_csc(n, k % n, k // n)


HUB_GRAPH, HUB_NODE, EDGELESS_GRAPH, ONE_NODE_GRAPH, ORDINARY_GRAPH, NO_IN_NODE = 0, 150, 1, 2, 3, 7


@functools.lru_cache(maxsize=None)
def batch_parts():
    """[(colptr, rowval)] per graph, node ids local to the graph"""
    rng = np.random.default_rng(BATCH_SEED)
    n0 = 300
    k = rng.permutation(n0 * n0)[:2000]
    src, dst = k % n0, k // n0
    keep = dst != HUB_NODE
    hub_src = rng.choice(n0, 150, replace=False)
    parts = [_pairs_csc(n0, np.concatenate([src[keep], hub_src]), np.concatenate([dst[keep], np.full(150, HUB_NODE)]))]
    parts.append((np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int64)))            # 5 nodes, no edge
    parts.append((np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int64)))     # one node, its self loop
    k = rng.permutation(20 * 20)[:70]
    src, dst = k % 20, k // 20
    parts.append(_pairs_csc(20, src[dst != NO_IN_NODE], dst[dst != NO_IN_NODE]))
    rest = N_GRAPHS - len(parts)
    sizes = 3 + rng.multinomial(N_NODES - sum(len(p[0]) - 1 for p in parts) - 3 * rest, np.full(rest, 1.0 / rest))
    left = N_EDGES - sum(len(p[1]) for p in parts)
    room = sizes.astype(np.int64) ** 2
    assert rest <= left <= room.sum()
    e = np.maximum(1, left * room // room.sum())
    while e.sum() != left:  # the rounding's remainder, one edge at a time where there is room
        i = int(rng.integers(rest))
        if e.sum() < left and e[i] < room[i]:
            e[i] += 1
        elif e.sum() > left and e[i] > 1:
            e[i] -= 1
    parts += [_exact_csc(rng, int(n), int(m)) for n, m in zip(sizes, e)]
    return tuple(parts)


@functools.lru_cache(maxsize=None)
def batch():
    """the batch's global (colptr, rowval, node_off, edge_off), int64; its properties are asserted here"""
    parts = batch_parts()
    node_off = np.concatenate([[0], np.cumsum([len(p[0]) - 1 for p in parts])]).astype(np.int64)
    edge_off = np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])]).astype(np.int64)
    colptr = np.concatenate([[0]] + [p[0][1:] + eo for p, eo in zip(parts, edge_off)]).astype(np.int64)
    rowval = np.concatenate([p[1] + no for p, no in zip(parts, node_off)]).astype(np.int64)
    G, N, E = len(parts), len(colptr) - 1, len(rowval)
    assert (G, N, E) == (N_GRAPHS, N_NODES, N_EDGES) and all(v % 64 for v in (G, N, E)) and G == 2 * 64 + 3
    indeg = np.diff(colptr)
    nodes, edges = np.diff(node_off), np.diff(edge_off)
    assert nodes[HUB_GRAPH] == nodes.max() and indeg[node_off[HUB_GRAPH] + HUB_NODE] > 128                       # a hub in the large graph
    assert edges[EDGELESS_GRAPH] == 0 and nodes[EDGELESS_GRAPH] > 1                                                # a graph without edges
    assert nodes[ONE_NODE_GRAPH] == 1                                                                              # a single-node graph
    assert indeg[node_off[ORDINARY_GRAPH] + NO_IN_NODE] == 0 and edges[ORDINARY_GRAPH] > nodes[ORDINARY_GRAPH]     # a node without in-edges
    assert (nodes >= 1).all() and (edges[np.arange(G) != EDGELESS_GRAPH] >= 1).all()
    return colptr, rowval, node_off, edge_off


def csc(cid):
    """the graph data the case's references are computed on"""
    return BC.csc() if CASE[cid]["R"] > 1 else batch()


def rows(cid):
    c = csc(cid)
    return len(c[1]), len(c[0]) - 1, len(c[2]) - 1


# ---------------------------------------------------------------------------------------------------------------------------------------
# the draws
# ---------------------------------------------------------------------------------------------------------------------------------------
def relu_kink_rows(p, csc_, x):
    """(edge, node, graph) boolean rows on which some relu pre-activation z of the float64 forward of one replica lies within
    U.KINK_MARGIN . U.RTOL . S_z of the kink (S_z: the forward scale of the pre-activation, oracle chain_block_tapes)"""
    tapes, _ = O.chain_block_tapes(p, csc_, *(np.asarray(v, dtype=np.float64) for v in x))
    out = []
    for name, tape in zip(FN, tapes):
        bad = np.zeros(tape[0][0].shape[0], dtype=bool)
        for (W, b, act), (X, SX, y, Sy, _) in zip(p[name], tape):
            if not isinstance(W, str) and act == O.ACT_RELU:
                z = X @ np.asarray(W, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
                bad |= (np.abs(z) <= U.KINK_MARGIN * U.RTOL * Sy).any(axis=1)
        out.append(bad)
    return out


def kinkfree_inputs(rng, p, csc_, x, max_rounds=20):
    """redraws the own features of every offending row — the ef row of an edge, the nf row of a node, the gf row of a graph — until a round finds
    none; asserts that none is left.  Returns (x, rounds)."""
    x = [v.copy() for v in x]
    for k in range(max_rounds + 1):
        bad = relu_kink_rows(p, csc_, [v[0] for v in x])
        if not any(b.any() for b in bad):
            return tuple(x), k
        if k == max_rounds:
            break
        for v, b in zip(x, bad):
            v[0][b] = rng.random((int(b.sum()), v.shape[-1]), dtype=np.float32)
    raise AssertionError(f"rows within the kink margin after {max_rounds} rounds: {[int(b.sum()) for b in bad]}")


@functools.lru_cache(maxsize=None)
def data(cid):
    """dict(p, x, cot): packed [R][T][d] float32"""
    c = CASE[cid]
    rng = np.random.default_rng(15000 + CASE_IDS.index(cid))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    E, N, G = rows(cid)
    R, variant = c["R"], c["variant"]
    p = O.make_chain_block_params(rng, c["in_dims"], *c["widths"], acts=c["acts"], last_acts=c["last"])
    x = list(U.packed_inputs(rng, R, E, N, G, c["in_dims"]))
    outw = out_widths(cid)
    cot = [f32(rng.standard_normal((R, T, d))) if d else None for T, d in zip((E, N, G), outw)]
    if variant == "log_uniform_inputs":
        x = [None if v is None else BC.log_uniform(rng, v.shape, -3, 3) for v in x]
    elif variant == "log_uniform_cotangents":
        cot = [BC.log_uniform(rng, g.shape) for g in cot]
    elif variant == "log_uniform_edge_cotangents":
        cot = [BC.log_uniform(rng, cot[0].shape), np.zeros_like(cot[1]), np.zeros_like(cot[2])]
    elif variant == "mean_graph_input":
        W, b, a = p["graph"][0]
        W = W.copy()
        W[:, :outw[0]] /= np.float32(E)
        W[:, outw[0]:outw[0] + outw[1]] /= np.float32(N)
        p["graph"][0] = (W, b, a)
    elif variant == "log_uniform_weights":
        W, b, a = p["edge"][0]
        p["edge"][0] = (f32(W * 10.0 ** rng.uniform(-4, 4, size=W.shape)), b, a)
    elif variant == "cancelling_dW":  # a common mode of 1e4 on the features against cotangent columns that sum to zero over the rows
        x = [f32(v + 1e4) for v in x]
        g = cot[0].astype(np.float64)
        cot = [f32(g - g.mean(axis=1, keepdims=True)), np.zeros_like(cot[1]), np.zeros_like(cot[2])]
    elif variant == "kinkfree":
        assert R == 1
        x, _ = kinkfree_inputs(rng, p, csc(cid), x)
        assert not any(b.any() for b in relu_kink_rows(p, csc(cid), [v[0] for v in x])), cid
    else:
        assert variant == "plain", variant
    assert (R_ in [a for n in FN for w, b, a in p[n] if not isinstance(w, str)]) == (cid == "N-relu"), cid
    return dict(p=p, x=tuple(x), cot=tuple(cot), R=R)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the shape of a case: per function (k_in, [(J, K, kind)]) with kind "dense" | "ln" | "ln_sqrt", and what the rule and the predicates say
# ---------------------------------------------------------------------------------------------------------------------------------------
def shape(cid):
    c = CASE[cid]
    de, dn, dg = c["in_dims"]
    out, outs = [], []
    for t, ws in enumerate(c["widths"]):
        k_in = de + 2 * dn + dg if t == 0 else (outs[0] + dn + dg if t == 1 else outs[0] + outs[1] + dg)
        k, layers = k_in, []
        for w in ws:
            if isinstance(w, str):
                layers.append((k, k, w))
            else:
                layers.append((w, k, "dense"))
                k = w
        outs.append(k if ws else 0)
        out.append((k_in, layers))
    return out


def out_widths(cid):
    return [layers[-1][0] if layers else 0 for _, layers in shape(cid)]


def formula_mask(cid):
    """the mask include/gnx.h's rule gives on this case's row counts (tests/test_chain_bw_narrow_abi.py restates the rule)"""
    mask = 0
    for t, ((k_in, layers), T) in enumerate(zip(shape(cid), rows(cid))):
        ln = tuple(i for i, l in enumerate(layers) if l[2] != "dense")
        if layers and formula_takes(k_in, [l[0] for l in layers], ln, T):
            mask |= 1 << t
    return mask


def want_mask(cid):
    """the mask the case asserts"""
    m = CASE[cid]["mask"]
    return formula_mask(cid) if m == "formula" else m


def acts_of(cid):
    """per function, the Dense layers' activations by layer index (None for a LayerNorm)"""
    return [[None if isinstance(w, str) else a for w, b, a in data(cid)["p"][n]] for n in FN]


NARROW_MUST_NOT = {"bw_dx_generic", "bw_dx_chain", "bw_layernorm", "bw_gelu_preact", "bw_chain_fw_g"}


def expected_scopes(cid, entry):
    """(must, must_not, kernels): profiler scope names of the case through `entry`, under the default selection of kernels; `kernels` = {scope:
    number of kernels} where the count is pinned.  The generic entry restates csrc/gnx_backward.hip's chain_backward: the graph and node chains
    and the edge chain's layers behind the first go row-wise (pull_layers: bw_dx_chain where bw_use_mfma holds for (R . rows, J, K), k_dw_gemm
    where bw_use_mfma_dw does, bw_layernorm for a LayerNorm), the edge chain's first layer through the block pullback of (in_dims) => (J_0, 0, 0)
    (k_dw_gemm as tests/bw_x6_cases.py's _block_scopes restates it); bw_gelu_preact wherever a gelu layer is differentiated."""
    c = CASE[cid]
    if entry == "narrow":
        if want_mask(cid) != 7:  # part fused, part generic: the generic levels' scopes as the generic entry would run them
            must = ({"bw_delta"} if c["widths"][1] or c["widths"][2] else set()) | ({"bw_delta_edge"} if want_mask(cid) & 1 else set())
            kinds = [{kind for i, (J, K, kind) in enumerate(layers) if not (want_mask(cid) >> t) & 1} for t, (_, layers) in enumerate(shape(cid))]
            if any(k & {"ln", "ln_sqrt"} for k in kinds):
                must.add("bw_layernorm")
            if any(BC.bw_use_mfma(c["R"] * T, J, K) for t, ((_, layers), T) in enumerate(zip(shape(cid), rows(cid))) if not (want_mask(cid) >> t) & 1
                   for i, (J, K, kind) in enumerate(layers) if kind == "dense" and (t, i) != (0, 0)):
                must.add("bw_dx_chain")
            return must, set(), {}
        return {"bw_delta", "bw_delta_edge"}, set(NARROW_MUST_NOT), {"bw_delta": 2, "bw_delta_edge": 1}
    R = c["R"]
    dx = dw = ln = False
    acts = acts_of(cid)
    gelu = any(a == G_ for fa in acts for a in fa)
    for t, ((k_in, layers), T) in enumerate(zip(shape(cid), rows(cid))):
        for i, (J, K, kind) in enumerate(layers):
            if t == 0 and i == 0:
                continue
            if kind != "dense":
                ln = True
            elif BC.bw_use_mfma(R * T, J, K):
                dx = True
                dw |= BC.bw_use_mfma_dw(R * T, J, K)
    (J0, K0, kind0) = shape(cid)[0][1][0]
    E, N, G = rows(cid)
    de, dn, dg = c["in_dims"]
    if kind0 != "dense":  # a LayerNorm first: behind an identity Dense of its own width (ChainLnFirst), then a row-wise LayerNorm layer
        J0, a0, ln = K0, I_, True
    else:
        a0 = acts[0][0]
    if a0 != G_ and BC.bw_use_mfma(R * E, J0, de + 2 * dn + dg):  # the block pullback's matrix-core edge level: dW by segment of the input row
        dw |= BC.bw_use_mfma_dw(R * E, J0, de) or BC.bw_use_mfma_dw(R * N, J0, dn) or BC.bw_use_mfma_dw(R * G, J0, dg)
    must, must_not = set(), set()
    for flag, name in ((dx, "bw_dx_chain"), (dw, "k_dw_gemm"), (ln, "bw_layernorm"), (gelu, "bw_gelu_preact")):
        (must if flag else must_not).add(name)
    must.add("bw_delta")
    return must, must_not, {}


# ---------------------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------------------
def grad_names(p):
    return {n for n, d in zip(DX, p["in_dims"]) if d} | {f"{name}{i}.{k}" for name in FN for i in range(len(p[name])) for k in ("dW", "db")}


def torch_chain_grads(p, csc_, x, cot, dt):
    """Every gradient of a block with Chain update functions by torch autograd of tests/chain_torch.py's _torch_chain_block in `dt`, replica by
    replica on one set of parameter leaves, under tests/test_gpu_chain_bw_narrow.py's BwCall.ref names and layouts, as float64 numpy"""
    T = lambda v, grad=True: torch.tensor(v, dtype=dt, requires_grad=grad)
    W = {name: [(w, T(b), T(a)) if isinstance(w, str) else (T(w), T(b), a) for w, b, a in p[name]] for name in FN}
    R = next(v.shape[0] for v in x if v is not None)
    xs = [[None if v is None else T(v[r]) for v in x] for r in range(R)]
    loss = 0.0
    for r in range(R):
        outs, _ = _torch_chain_block(csc_, *xs[r], W)
        loss = loss + sum((o * T(c[r], False)).sum() for o, c in zip(outs, cot) if o is not None and c is not None)
    loss.backward()
    f = lambda t: (torch.zeros_like(t) if t.grad is None else t.grad).double().numpy()
    ref = {n: np.stack([f(xs[r][k]) for r in range(R)]) for k, n in enumerate(DX) if x[k] is not None}
    for name in FN:
        for i, (w, b, a) in enumerate(W[name]):
            if isinstance(w, str):
                ref[f"{name}{i}.dW"], ref[f"{name}{i}.db"] = f(b), f(a)
            else:
                ref[f"{name}{i}.dW"], ref[f"{name}{i}.db"] = f(w).T, f(b)
    return ref


def _drop_none(d):
    return {k: v for k, v in d.items() if v is not None}


@functools.lru_cache(maxsize=None)
def reference(cid):
    """(ref, S, yard): the float64 oracle's gradients, their scales, the float32 torch evaluation — {name: float64 array}"""
    d = data(cid)
    ref, S = O.chain_block_backward_sparse(d["p"], csc(cid), d["x"], d["cot"])
    ref, S = _drop_none(ref), _drop_none(S)
    yard = torch_chain_grads(d["p"], csc(cid), d["x"], d["cot"], F32)
    assert set(ref) == set(S) == set(yard) == grad_names(d["p"]), cid
    return ref, S, yard


def normwise_applies(cid, name):
    """whether the old normwise bar, max|got - ref| <= CHAIN_BAR . max(1, max|ref|), is asserted on a tensor as well — so that no tensor is held more
    loosely than tests/test_gpu_chain.py held it where S is the worst-case scale of several levels.  Everywhere but on the edge chain's weight
    gradients of the cancelling cases: there the sum cancels to 1e-4 of its terms, a normwise bar on the result is a bar on nothing the
    arithmetic controls (plain torch float32 misses it 10 .. 20 times over; tests/test_chain_bw_stress_cpu.py), and S is what holds them."""
    return not (CASE[cid]["variant"] == "cancelling_dW" and name.startswith("edge") and name.endswith(".dW"))


FW = ("ef_out", "nf_out", "gf_out")


@functools.lru_cache(maxsize=None)
def forward_reference(cid):
    """({ef_out, nf_out, gf_out}, their scales) of chain_block_forward_sparse"""
    d = data(cid)
    ref, S = O.chain_block_forward_sparse(d["p"], csc(cid), *d["x"], return_scale=True)
    return dict(zip(FW, ref)), dict(zip(FW, S))


# the properties the cases exist for, asserted where the cases are defined
def _assert_cases():
    kinds = lambda cid: [[l[2] for l in layers] for _, layers in shape(cid)]
    wmax = lambda cid: [8 if m <= 8 else (16 if m <= 16 else 32) for m in (max([k_in] + [l[0] for l in layers]) for k_in, layers in shape(cid))]
    assert wmax("N-w8") == [8, 8, 8] and wmax("N-w16-32") == [32, 16, 16]
    for cid in ("N-ln-both-modes", "N-log_uniform_inputs"):
        for ks in kinds(cid):
            assert "ln" in ks and "ln_sqrt" in ks, (cid, ks)
        assert kinds(cid)[2][0] != "dense" and kinds(cid)[2][-1] != "dense" and kinds(cid)[1][-1] != "dense"
    for cid in CASE_IDS:  # no LayerNorm over fewer than 3 elements
        assert all(l[0] >= 3 for _, layers in shape(cid) for l in layers if l[2] != "dense"), cid
    for cid in NARROW_IDS:
        assert want_mask(cid) == formula_mask(cid), (cid, formula_mask(cid))
    assert formula_mask("N-mixed") == 2
    for cid in CASE_IDS:
        if CASE[cid]["family"] == "wide":
            assert formula_mask(cid) == 0, cid
            for t, (k_in, layers) in enumerate(shape(cid)):  # every Dense layer of a wide case on the matrix cores (rows >= 64, J K >= 64)
                assert all(BC.bw_use_mfma(rows(cid)[t], J, K) for J, K, kind in layers if kind == "dense"), (cid, t)
    assert any(k == "ln_sqrt" for ks in kinds("W-tails") for k in ks)
    tails = [(t, i, J, K) for t, (_, layers) in enumerate(shape("W-tails")) for i, (J, K, kind) in enumerate(layers) if kind == "dense"]
    assert all(J % 16 and (K % 16 or (t, i) == (0, 0)) for t, i, J, K in tails), tails  # tile tails in J and K (K_e = 96 is the input's)
    g = kinds("N-gelu-hidden")
    assert g[0] == ["dense", "ln", "dense", "dense"] and g[1] == ["dense", "ln_sqrt", "dense", "dense"]
    assert CASE["N-R2"]["R"] == 2 and rows("N-R2") == (N_EDGES, N_NODES, 1)
    assert formula_mask("N-ln-sqrt-first") == 1 and kinds("N-ln-sqrt-first")[0] == ["ln_sqrt", "dense"]


_assert_cases()
