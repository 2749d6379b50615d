"""
numpy restatement of networkx 3.4.2's unweighted betweenness_centrality (betweenness.py:
_single_source_shortest_path_basic, _accumulate_basic, _accumulate_endpoints, _rescale) on CSR arrays, for the
tests where networkx itself is too slow (a 1 M-node graph is not held as a networkx object).  One source at a time,
level-synchronous and vectorised per level.  No reference code.
"""
import random

import networkx as nx
import numpy as np

#: The one tolerance of every betweenness comparison.  Each term is formed with networkx's own operations
#: (sigma sums of whole numbers, exact below 2^53; coeff = (1 + delta) / sigma; sigma(v) * coeff(w); bc += delta, or
#: delta + 1 with endpoints; bc *= the same scale), and every node adds its sources' terms in networkx's source order.
#: Only the order of the additions inside one delta(v) differs (networkx: reverse BFS order of the successors; here
#: and on the GPU: column order).  All terms are positive, so nothing cancels, but the worst-case bound of reordering a
#: positive sum of d terms is about d * 2^-53: ~1.1e-12 at the ~10^4-neighbour hubs of BA 1 M, i.e. no room there.
#: 1e-12 holds in practice because the rounding errors of a long sum behave like a random walk (growing like sqrt(d),
#: not d) and most sums are short; it is an empirical bound for the graphs tested, not a proven one.
RTOL = 1e-12


def csr_of(G, nodelist=None):
    """(row_ptr, col) of G's out-adjacency in `nodelist` order (default list(G)); parallel edges once."""
    nodelist = list(G) if nodelist is None else nodelist
    A = nx.to_scipy_sparse_array(G, nodelist=nodelist, weight=None, dtype=float, format='csr')
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int64)


def rescale_factor(n, normalized, directed, k, endpoints):
    """networkx's _rescale factor (None = no scaling)."""
    if normalized:
        if endpoints:
            scale = None if n < 2 else 1 / (n * (n - 1))
        elif n <= 2:
            scale = None
        else:
            scale = 1 / ((n - 1) * (n - 2))
    else:
        scale = None if directed else 0.5
    if scale is not None and k is not None:
        scale = scale * n / k
    return scale


def _out_arcs(row_ptr, col, rows):
    """(tail, head) of every arc leaving `rows`."""
    b, e = row_ptr[rows], row_ptr[rows + 1]
    deg = e - b
    tail = np.repeat(rows, deg)
    start = np.repeat(b - np.cumsum(deg) + deg, deg)
    head = col[start + np.arange(int(deg.sum()))]
    return tail, head


def betweenness_arrays(row_ptr, col, sources, directed, normalized=True, endpoints=False, k=None):
    """bc over the out-adjacency (row_ptr, col) of n = len(row_ptr) - 1 nodes from `sources` (row ids) in order."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n = len(row_ptr) - 1
    bc = np.zeros(n)
    for s in sources:
        D = np.full(n, -1, dtype=np.int64)
        sigma = np.zeros(n)
        D[s], sigma[s] = 0, 1.0
        levels = [np.array([s], dtype=np.int64)]
        while True:                                              # forward: sigma[w] += sigma[v] per shortest arc
            l = len(levels) - 1
            tail, head = _out_arcs(row_ptr, col, levels[-1])
            D[head[D[head] < 0]] = l + 1
            on = D[head] == l + 1
            if not on.any():
                break
            sigma += np.bincount(head[on], weights=sigma[tail[on]], minlength=n)
            levels.append(np.unique(head[on]))
        delta = np.zeros(n)
        for l in range(len(levels) - 1, 0, -1):                  # backward, deepest level first
            W = levels[l]
            coeff = np.zeros(n)
            coeff[W] = (1 + delta[W]) / sigma[W]
            tail, head = _out_arcs(row_ptr, col, levels[l - 1])
            on = D[head] == l
            terms = sigma[tail[on]] * coeff[head[on]]
            delta += np.bincount(tail[on], weights=terms, minlength=n)
        reached = np.concatenate(levels[1:]) if len(levels) > 1 else np.zeros(0, dtype=np.int64)
        if endpoints:
            bc[s] += sum(len(x) for x in levels) - 1
            bc[reached] += delta[reached] + 1
        else:
            bc[reached] += delta[reached]
    scale = rescale_factor(n, normalized, directed, k, endpoints)
    return bc if scale is None else bc * scale


def sample_sources(G, k, seed):
    """networkx's sources: list(G), or seed.sample(list(G), k) with seed an int or a random.Random."""
    nodes = list(G)
    if k is None:
        return nodes
    rng = random.Random(seed) if isinstance(seed, int) else seed
    return rng.sample(nodes, k)


def betweenness(G, k=None, normalized=True, endpoints=False, seed=None):
    """label -> value, as nx.betweenness_centrality(G, k, normalized, None, endpoints, seed) (seed: int or Random)."""
    nodelist = list(G)
    row_of = {v: i for i, v in enumerate(nodelist)}
    row_ptr, col = csr_of(G, nodelist)
    sources = [row_of[v] for v in sample_sources(G, k, seed)]
    bc = betweenness_arrays(row_ptr, col, sources, G.is_directed(), normalized, endpoints, k)
    return dict(zip(nodelist, map(float, bc)))
