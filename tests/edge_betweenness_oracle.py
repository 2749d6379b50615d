"""
numpy restatement of networkx 3.4.2's edge_betweenness_centrality (betweenness.py: edge_betweenness_centrality,
_single_source_shortest_path_basic / _single_source_dijkstra_path_basic, _accumulate_edges, _rescale_e) on CSR arrays,
for the sizes where networkx itself is too slow.  One source at a time, level-synchronous and vectorised per level, on
the helpers of tests/betweenness_oracle.py; the weighted form reads the shortest-path DAG of
tests/weighted_betweenness_oracle.py.  Every arc slot v -> w adds the term sigma(v) * coeff(w) of each source whose DAG
holds the arc; an undirected edge is the sum of its two slots; the scale is _rescale_e's as networkx calls it (without
k).  The order of the additions is numpy's, not the kernel's: the tolerance is betweenness_oracle.RTOL with atol = 0.
No reference code.
"""
import numpy as np

from tests import betweenness_oracle as bo
from tests import sssp_oracle as so
from tests import weighted_betweenness_oracle as wo

RTOL = bo.RTOL


def rescale_e_factor(n, normalized, directed):
    """networkx's _rescale_e factor as edge_betweenness_centrality calls it: k is not passed (1.0 = no scaling)."""
    if normalized:
        return 1.0 if n <= 1 else 1 / (n * (n - 1))
    return 1.0 if directed else 0.5


def _slots(row_ptr, rows):
    """The arc slots of `rows`, row after row."""
    b, deg = row_ptr[rows], row_ptr[rows + 1] - row_ptr[rows]
    return np.repeat(b - np.cumsum(deg) + deg, deg) + np.arange(int(deg.sum()))


def arc_sums(row_ptr, col, sources):
    """Per arc slot of the out CSR: the sum over `sources` of sigma(v) * coeff(w) where v -> w is a BFS DAG arc."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n = len(row_ptr) - 1
    tail_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    arc = np.zeros(len(col))
    for s in sources:
        D = np.full(n, -1, dtype=np.int64)
        sigma = np.zeros(n)
        D[s], sigma[s] = 0, 1.0
        levels = [np.array([s], dtype=np.int64)]
        while True:                                              # forward, as betweenness_oracle
            l = len(levels) - 1
            tail, head = bo._out_arcs(row_ptr, col, levels[-1])
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
            slots = _slots(row_ptr, levels[l - 1])
            slots = slots[D[col[slots]] == l]
            terms = sigma[tail_of[slots]] * coeff[col[slots]]
            arc[slots] += terms                                  # a slot occurs once per source
            delta += np.bincount(tail_of[slots], weights=terms, minlength=n)
    return arc


def weighted_arc_sums(out, inn, sources):
    """The same over the shortest-path DAG by weight: out / inn = (row_ptr, col, w) of the out- and in-adjacency."""
    sources = np.asarray(sources, dtype=np.int64)
    out_arcs, in_arcs = wo._arcs(out, None), wo._arcs(inn, None)
    r, x, xw = out_arcs[0], out_arcs[1], out_arcs[2]             # CSR order: slot j is arc r[j] -> x[j]
    arc = np.zeros(len(r))
    levels = 0
    for first in range(0, len(sources), 64):
        group = sources[first:first + 64]
        dist, _ = so.relax(inn[0], np.asarray(inn[1], dtype=np.int64), np.asarray(inn[2], dtype=np.float64), group)
        depth, sigma, delta, level = wo.batch_passes(out_arcs, in_arcs, dist, group)
        levels = max(levels, level)
        D = np.ascontiguousarray(np.asarray(dist).T)
        with np.errstate(divide='ignore', invalid='ignore'):
            coeff = np.where(depth > 0, (1.0 + delta) / sigma, 0.0)
        on = (np.isfinite(D[x]) & (D[r] + xw[:, None] == D[x]) & (D[r] < D[x]) & (depth[r] >= 0) &
              (depth[x] > depth[r]))
        terms = np.where(on, sigma[r] * coeff[x], 0.0)
        for b in range(terms.shape[1]):                          # source after source
            arc += terms[:, b]
    return arc, levels


def edge_values(row_ptr, col, arc, directed, scale):
    """(u, v, value) per edge from the per-arc sums: directed = every arc scaled; undirected = the arcs with u <= v, an
    edge being the sum of its two slots (a self-loop keeps its 0.0)."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n = len(row_ptr) - 1
    u = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    if directed:
        return u, col, arc * scale
    key = u * n + col                                            # ascending: rows in order, columns sorted
    mirror = np.searchsorted(key, col * n + u)
    assert np.array_equal(key[mirror], col * n + u), 'the CSR of an undirected graph must be symmetric'
    once = np.nonzero(u <= col)[0]
    both = np.where(u[once] == col[once], arc[once], arc[once] + arc[mirror[once]])
    return u[once], col[once], both * scale


def edge_betweenness(G, k=None, normalized=True, weight=None, seed=None):
    """{(u, v): value} as nx.edge_betweenness_centrality(G, k, normalized, weight, seed) (seed: int or Random), the
    keys with u before v in sorted-label order for an undirected graph."""
    directed = G.is_directed()
    if weight is None:
        labels = sorted(G)
        row_ptr, col = bo.csr_of(G, labels)
        row_of = {v: i for i, v in enumerate(labels)}
        arc = arc_sums(row_ptr, col, [row_of[v] for v in bo.sample_sources(G, k, seed)])
    else:
        labels, out, inn = wo.csr_pair(G, weight)
        row_ptr, col = np.asarray(out[0], dtype=np.int64), np.asarray(out[1], dtype=np.int64)
        row_of = {v: i for i, v in enumerate(labels)}
        arc, _ = weighted_arc_sums(out, inn, [row_of[v] for v in bo.sample_sources(G, k, seed)])
    if len(col) == 0:
        return {}
    u, v, val = edge_values(row_ptr, col, arc, directed, rescale_e_factor(len(labels), normalized, directed))
    return {(labels[a], labels[b]): float(c) for a, b, c in zip(u, v, val)}


def by_sorted_ends(G, values: dict) -> dict:
    """An edge dict of networkx with the ends of every undirected key in sorted order."""
    if G.is_directed():
        return dict(values)
    return {((a, b) if a <= b else (b, a)): c for (a, b), c in values.items()}
