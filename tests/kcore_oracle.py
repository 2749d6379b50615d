"""
Plain numpy restatement of the synchronous peeling of csrc/grx_kcore.hip over a CSR (row_ptr, col) of a graph's distinct
arcs without self-loops -- symmetric for an undirected graph; with the in-adjacency (in_row_ptr, in_col) as well for a
directed one:

    k = 0, layer = 1, every node alive, deg(v) = row length (directed: out-row + in-row)
    while a node is alive:
        k = max(k, min deg over the alive nodes)
        F = {alive v : deg(v) <= k}                  on the degrees at the start of the round
        core(v) = k, onion(v) = layer for v in F; F leaves
        for v in F, for every arc v-u with u still alive: deg(u) -= 1       (directed: out-arcs and in-arcs)
        layer += 1

core equals nx.core_number, onion equals nx.onion_layers (undirected).  Every round is a handful of whole-array numpy
calls (it rescans all n nodes per round, which the kernels do not), so BA 1 M / 10 M takes a few seconds.  Used by
tests only.
"""
from collections import namedtuple

import numpy as np

Result = namedtuple('Result', 'core onion n_rounds')


def symmetric_csr(n, edges):
    """(row_ptr, col) of the distinct arcs of an undirected edge list over rows 0 .. n - 1, ascending in each row."""
    e = np.asarray(list(edges), dtype=np.int64).reshape(-1, 2)
    return directed_csr(n, np.concatenate([e, e[:, ::-1]]))


def directed_csr(n, arcs):
    """(row_ptr, col) of the distinct arcs (u, v) as rows u, ascending in each row."""
    a = np.asarray(list(arcs), dtype=np.int64).reshape(-1, 2)
    key = np.unique(a[:, 0] * n + a[:, 1]) if len(a) else np.zeros(0, dtype=np.int64)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // max(n, 1), minlength=n), out=row_ptr[1:])
    return row_ptr, key % max(n, 1)


def graph_csrs(G):
    """(nodelist, row_ptr, col, in_row_ptr, in_col) of a networkx graph, rows in list(G) order; the in CSR is None for
    an undirected graph."""
    nodes = list(G)
    row_of = {v: i for i, v in enumerate(nodes)}
    edges = [(row_of[u], row_of[v]) for u, v in G.edges()]
    if not G.is_directed():
        return (nodes,) + symmetric_csr(len(nodes), edges) + (None, None)
    return ((nodes,) + directed_csr(len(nodes), edges)
            + directed_csr(len(nodes), [(v, u) for u, v in edges]))


def _row_entries(row_ptr, col, rows):
    """The concatenated entries of `rows`."""
    begin = row_ptr[rows]
    length = row_ptr[rows + 1] - begin
    total = int(length.sum())
    if total == 0:
        return np.zeros(0, dtype=np.int64)
    offset = np.cumsum(length) - length
    return col[np.repeat(begin - offset, length) + np.arange(total, dtype=np.int64)]


def core_numbers(row_ptr, col, in_row_ptr=None, in_col=None) -> Result:
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n = len(row_ptr) - 1
    deg = np.diff(row_ptr)
    if in_row_ptr is not None:
        in_row_ptr = np.asarray(in_row_ptr, dtype=np.int64)
        in_col = np.asarray(in_col, dtype=np.int64)
        deg = deg + np.diff(in_row_ptr)
    alive = np.ones(n, dtype=bool)
    core = np.zeros(n, dtype=np.int64)
    onion = np.zeros(n, dtype=np.int64)
    k, layer, left = 0, 1, n
    while left:
        k = max(k, int(deg[alive].min()))
        F = np.nonzero(alive & (deg <= k))[0]
        core[F] = k
        onion[F] = layer
        alive[F] = False
        left -= len(F)
        ends = _row_entries(row_ptr, col, F)
        if in_row_ptr is not None:
            ends = np.concatenate([ends, _row_entries(in_row_ptr, in_col, F)])
        ends = ends[alive[ends]]
        if len(ends):
            deg = deg - np.bincount(ends, minlength=n)
        layer += 1
    return Result(core, onion, layer - 1)
