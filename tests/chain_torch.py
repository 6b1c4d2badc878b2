"""The torch restatement of a GNBlock with Chain update functions, shared by the Chain tests (no device, no library)."""
import numpy as np

from oracle import gn_oracle as O


def _torch_chain_block(csc, ef, nf, gf, W):
    """float64 torch restatement of the block with Chain update functions (one replica); W[name] = list of (weight, bias, act)."""
    import torch
    ACT = {0: lambda x: x, 1: torch.relu, 2: torch.tanh, 3: torch.sigmoid, 4: lambda x: torch.nn.functional.gelu(x, approximate="tanh")}
    colptr, rowval, node_off, edge_off = (torch.from_numpy(np.asarray(a)) for a in csc)
    N, G = len(colptr) - 1, len(node_off) - 1
    dst = torch.repeat_interleave(torch.arange(N), colptr[1:] - colptr[:-1])
    ng = torch.repeat_interleave(torch.arange(G), node_off[1:] - node_off[:-1])
    eg = torch.repeat_interleave(torch.arange(G), edge_off[1:] - edge_off[:-1])
    cat = lambda parts: torch.cat([q for q in parts if q is not None], dim=1)

    def chain(x, layers, pre):
        for w, b, a in layers:
            if isinstance(w, str):  # ("layernorm", gamma, beta): Flux 0.14 normalise (x - mean) / (sigma + eps), then gamma . xhat + beta
                mu = x.mean(dim=1, keepdim=True)
                var = ((x - mu) ** 2).mean(dim=1, keepdim=True)
                den = (var + 1e-5).sqrt() if O.ln_eps_mode(w) == 1 else var.sqrt() + 1e-5  # ("layernorm_sqrt_eps": / sqrt(sigma^2 + eps))
                x = b * ((x - mu) / den) + a
                continue
            z = x @ w.T + b
            pre.append((z, a))
            x = ACT[a](z)
        return x

    pre = []
    he = chain(cat([ef, None if nf is None else nf[rowval], None if nf is None else nf[dst], None if gf is None else gf[eg]]), W["edge"], pre)
    hn = hg = None
    if W["node"]:
        agg = torch.zeros((N, he.shape[1]), dtype=he.dtype).index_add(0, dst, he)
        hn = chain(cat([agg, nf, None if gf is None else gf[ng]]), W["node"], pre)
    if W["graph"]:  # (a block without a node function: its zero-width nf' is an empty segment of the graph function's input, gnblock.jl:63-69)
        se = torch.zeros((G, he.shape[1]), dtype=he.dtype).index_add(0, eg, he)
        sn = None if hn is None else torch.zeros((G, hn.shape[1]), dtype=he.dtype).index_add(0, ng, hn)
        hg = chain(cat([se, sn, gf]), W["graph"], pre)
    return (he, hn, hg), pre
