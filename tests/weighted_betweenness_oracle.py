"""
numpy restatement of grx_weighted_betweenness (csrc/grx_weighted_betweenness.hip) on host CSR arrays, out and in:
the Jacobi Bellman-Ford relaxation of tests/sssp_oracle.py, the shortest-path DAG read off its converged distances
(arc u -> v of weight w is a DAG arc iff D(v) is finite, fl(D(u) + w) == D(v) and D(u) < D(v)), the forward rounds
that give a cell its depth and sigma once EVERY DAG predecessor is resolved, the backward levels deepest first with
the terms sigma(v) * coeff(x) added in arc order (hub rows: four strided partial sums, ((p0 + p1) + p2) + p3), and the
accumulation source by source.  Against networkx only the order of the additions inside one delta(v) differs, so the
tolerance is betweenness_oracle.RTOL with atol = 0: entries networkx has at exactly 0 must be exactly 0.
Also the weighted test graphs both test files share.  No reference code.
"""
import networkx as nx
import numpy as np

from tests import betweenness_oracle as bo
from tests import sssp_oracle as so

RTOL = bo.RTOL
HUB_PARTS = 4                                                   # WB_PARTS of the kernel


def with_weights(G, kind: str, seed: int = 0):
    """so.with_weights, and the kind 'dyadic': multiples of 0.25 in [0.25, 2.0] -- float weights whose sums are exact,
    so that lightest paths tie as often as with integers."""
    if kind != 'dyadic':
        return so.with_weights(G, kind, seed)
    H = G.copy()
    rng = np.random.default_rng(seed)
    for u, v in H.edges():
        H[u][v]['weight'] = 0.25 * float(rng.integers(1, 9))
    return H


def uneven_ties_graph():
    """20 nodes.  Node 1 has two lightest paths from node 0 with different numbers of arcs: 0 - 1 (weight 2) and
    0 - 2 - 1 (1 + 1).  Settling sigma(1) at its first tight predecessor (node 0, depth 0) would miss the second."""
    G = nx.Graph()
    G.add_weighted_edges_from([(0, 1, 2.0), (0, 2, 1.0), (2, 1, 1.0), (1, 3, 1.0)])
    G.add_weighted_edges_from((v, v + 1, 1.0) for v in range(3, 19))
    G.add_weighted_edges_from([(4, 9, 5.0), (3, 12, 9.0), (0, 19, 30.0), (6, 15, 2.0)])
    return G


def csr_pair(G, weight='weight'):
    """(labels, out CSR, in CSR) of G, each (row_ptr, col, w) with rows = the sorted labels; an undirected graph's out
    CSR is its in CSR."""
    labels, row_ptr, col, w = so.pulled_csr(G, weight)
    inn = (row_ptr, col, w)
    if not G.is_directed():
        return labels, inn, inn
    _, o_ptr, o_col, o_w = so.pulled_csr(G.reverse(copy=True), weight)
    return labels, (o_ptr, o_col, o_w), inn


def _arcs(csr, hub_degree):
    """The arcs of a CSR grouped by partial sum: (row, column, weight) of every arc in the order of its slot
    row * HUB_PARTS + part (arc order inside a slot; part = position % HUB_PARTS in a hub row, else 0), every arc's
    slot, and the number of rows."""
    row_ptr, col, w = csr
    n = len(row_ptr) - 1
    deg = np.diff(row_ptr)
    row = np.repeat(np.arange(n, dtype=np.int64), deg)
    pos = np.arange(len(col), dtype=np.int64) - row_ptr[row]
    part = np.where(deg[row] > hub_degree, pos % HUB_PARTS, 0) if hub_degree is not None else np.zeros_like(pos)
    slot = row * HUB_PARTS + part
    order = np.argsort(slot, kind='stable')
    return row[order], np.asarray(col, dtype=np.int64)[order], np.asarray(w, dtype=np.float64)[order], slot[order], n


def _by_parts(arcs, sel, terms):
    """Per row and lane ((p0 + p1) + p2) + p3 of the partial sums of `terms` (one row per arc of `sel`, ascending
    positions in the order of `_arcs`), each added in arc order; a row that is no hub has p0 only.  Adding the 0.0 of
    an arc that does not count changes no bit, and neither does leaving such an arc out."""
    slot, n = arcs[3][sel], arcs[4]
    p = np.zeros((n * HUB_PARTS, terms.shape[1]))
    if len(slot):
        starts = np.nonzero(np.diff(slot, prepend=-1))[0]
        p[slot[starts]] = np.add.reduceat(terms, starts, axis=0)
    p = p.reshape(n, HUB_PARTS, -1)
    return ((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]


def batch_passes(out_arcs, in_arcs, dist, sources):
    """(depth[n, B], sigma[n, B] before the backward pass, delta[n, B], levels) of one batch: lane b is source
    sources[b] with the converged distances dist[b]."""
    D = np.ascontiguousarray(np.asarray(dist).T)
    n, B = D.shape
    depth = np.where(np.isfinite(D), -1, -2).astype(np.int64)
    sigma = np.zeros((n, B))
    for b, s in enumerate(sources):
        if 0 <= s < n:
            depth[s, b], sigma[s, b] = 0, 1.0
    v, u, w, _, _ = in_arcs                                     # arc u -> v listed in v's row
    tight = np.isfinite(D[v]) & (D[u] + w[:, None] == D[v]) & (D[u] < D[v])
    level = 0
    while True:                                                 # forward: a cell waits for its deepest predecessor
        # only a row with a DAG predecessor resolved in the round before can resolve now: the others are left out
        fresh = np.zeros(n, dtype=bool)
        fresh[v[(tight & (depth[u] == level)).any(axis=1)]] = True
        sel = np.nonzero(fresh[v])[0]
        on, pre = tight[sel], depth[u[sel]]
        blocked = _by_parts(in_arcs, sel, (on & (pre < 0)).astype(np.float64)) > 0
        acc = _by_parts(in_arcs, sel, np.where(on & (pre >= 0), sigma[u[sel]], 0.0))
        ready = (depth == -1) & ~blocked & (acc > 0)
        if not ready.any():
            break
        level += 1
        depth[ready] = level
        sigma[ready] = acc[ready]
    counts = sigma.copy()
    r, x, xw, _, _ = out_arcs                                   # arc r -> x listed in r's row
    on = np.isfinite(D[x]) & (D[r] + xw[:, None] == D[x]) & (D[r] < D[x]) & (depth[r] > 0) & (depth[x] > 0)
    delta = np.zeros((n, B))
    coeff = np.zeros((n, B))
    for l in range(level, 0, -1):                               # backward, deepest level first
        at = depth == l
        sel = np.nonzero(at.any(axis=1)[r])[0]                  # the arcs of the rows with a cell at this level
        mine = on[sel] & (depth[r[sel]] == l)                   # every DAG successor is deeper: its coeff is final
        d = _by_parts(out_arcs, sel, np.where(mine, sigma[r[sel]] * coeff[x[sel]], 0.0))
        delta[at] = d[at]
        coeff[at] = (1.0 + delta[at]) / sigma[at]
    return depth, counts, delta, level


def single_source(out_arcs, in_arcs, D, s):
    """(depth, sigma before the backward pass, delta, levels) of one source with converged distances D."""
    depth, counts, delta, level = batch_passes(out_arcs, in_arcs, np.asarray(D)[None, :], [s])
    return depth[:, 0], counts[:, 0], delta[:, 0], level


def source_terms(out, inn, sources, hub_degree_out=None, hub_degree_in=None):
    """The passes of every source, which do not depend on the batch width: ([(s, depth, delta)] in the order of
    `sources`, levels, max sigma)."""
    sources = np.asarray(sources, dtype=np.int64)
    out_arcs, in_arcs = _arcs(out, hub_degree_out), _arcs(inn, hub_degree_in)
    terms, levels, max_sigma = [], 0, 0.0
    for first in range(0, len(sources), 64):
        group = sources[first:first + 64]
        dist, _ = so.relax(inn[0], np.asarray(inn[1], dtype=np.int64), np.asarray(inn[2], dtype=np.float64), group)
        depth, counts, delta, level = batch_passes(out_arcs, in_arcs, dist, group)
        levels = max(levels, level)
        max_sigma = max(max_sigma, float(counts.max()) if counts.size else 0.0)
        terms += [(int(s), depth[:, b].copy(), delta[:, b].copy()) for b, s in enumerate(group)]
    return terms, levels, max_sigma


def relaxation_rounds(inn, sources, batch: int = 0) -> int:
    """The relaxation rounds of the kernel, summed over its batches of S sources."""
    sources = np.asarray(sources, dtype=np.int64)
    S = so.batch_width(batch, len(sources))
    return sum(so.relax(inn[0], np.asarray(inn[1], dtype=np.int64), np.asarray(inn[2], dtype=np.float64),
                        sources[first:first + S])[1] for first in range(0, len(sources), S))


def accumulate(terms, n: int, endpoints, scale):
    """bc from the passes of `source_terms`: every node adds its sources' contributions in their order."""
    bc = np.zeros(n)
    for s, depth, delta in terms:
        inner = depth > 0
        if endpoints:
            bc[inner] += delta[inner] + 1.0
            if 0 <= s < n:
                bc[s] += float(int((depth >= 0).sum()) - 1)
        else:
            bc[inner] += delta[inner]
    return bc * scale


def betweenness_arrays(out, inn, sources, endpoints, scale, batch: int = 0, hub_degree_out=None, hub_degree_in=None,
                       info=None):
    """(bc, rounds, levels) as the kernel forms them.  out / inn: (row_ptr, col, w) of the out- and the in-adjacency;
    sources: row ids in accumulation order; hub_degree_*: rows longer than this add four strided partial sums (None: no
    hub rows); info: a dict that receives 'max_sigma', the largest number of lightest paths into any node."""
    terms, levels, max_sigma = source_terms(out, inn, sources, hub_degree_out, hub_degree_in)
    if info is not None:
        info['max_sigma'] = max_sigma
    return (accumulate(terms, len(out[0]) - 1, endpoints, scale), relaxation_rounds(inn, sources, batch), levels)


def betweenness(G, k=None, normalized=True, endpoints=False, seed=None, weight='weight', info=None):
    """label -> value, as nx.betweenness_centrality(G, k, normalized, weight, endpoints, seed) (seed: int or Random)."""
    labels, out, inn = csr_pair(G, weight)
    row_of = {v: i for i, v in enumerate(labels)}
    sources = [row_of[v] for v in bo.sample_sources(G, k, seed)]
    scale = bo.rescale_factor(len(labels), normalized, G.is_directed(), k, endpoints)
    bc, _, _ = betweenness_arrays(out, inn, sources, endpoints, 1.0 if scale is None else scale, info=info)
    return dict(zip(labels, map(float, bc)))
