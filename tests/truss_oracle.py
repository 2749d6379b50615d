"""
Plain numpy restatement of the level-synchronous edge peeling of csrc/grx_truss.hip over the CSR (row_ptr, col) of an
undirected graph's distinct arcs -- symmetric, columns ascending, no self-loops:

    sup(e) = |N(u) & N(v)| for every edge e = (u, v); an edge's id is the position of its arc with row < column
    k = 2, round = 1, every edge alive
    while an edge is alive:
        F = {alive e : sup(e) <= k - 2}          if empty: k = 2 + min sup over the alive edges, then F
        t(e) = k for e in F
        for e = (u, v) in F, for every w in N(u) & N(v) with a = (u, w), b = (v, w) not gone in an EARLIER round:
            neither in F:   sup(a) -= 1, sup(b) -= 1
            only a in F:    sup(b) -= 1  iff  id(e) < id(a)        (dedupe=False: always -- the triangle dies twice)
            only b in F:    sup(a) -= 1  iff  id(e) < id(b)
            both in F:      nothing
        F leaves; round += 1
    t(v) = max t(e) over the edges at v, 0 without an edge

t(e) is the largest k with e in nx.k_truss(G, k), t(v) the largest k with v among its nodes (``networkx_truss_numbers``
derives both from networkx itself).  Every round is a handful of whole-array numpy calls: the triangles of the round's
frontier come from one sorted search of (other end, common neighbour) keys among the arcs' keys.  Used by tests and
by tools/bench_truss.py (the decrement counts of the profile) only.
"""
from collections import namedtuple

import numpy as np

Result = namedtuple('Result', 'arc_truss node_truss n_rounds n_levels decrements frontier_max')

#: (edge, walked entry) pairs looked up per numpy call
_CHUNK_PAIRS = 1 << 24


class _Arcs:
    def __init__(self, row_ptr, col):
        self.row_ptr = np.asarray(row_ptr, dtype=np.int64)
        self.col = np.asarray(col, dtype=np.int64)[:int(self.row_ptr[-1])]
        self.n = len(self.row_ptr) - 1
        self.deg = np.diff(self.row_ptr)
        self.row = np.repeat(np.arange(self.n, dtype=np.int64), self.deg)
        self.key = self.row * self.n + self.col                 # ascending: rows in order, columns ascending
        assert np.all(np.diff(self.key) > 0), 'columns must ascend inside every row'
        assert not np.any(self.row == self.col), 'no self-loops'
        self.rev = np.searchsorted(self.key, self.col * self.n + self.row)
        assert len(self.key) == 0 or (self.rev.max() < len(self.key)
                                      and np.array_equal(self.key[self.rev], self.col * self.n + self.row)), 'symmetric'
        self.is_id = self.row < self.col

    def edge_id(self, j):
        return np.where(self.is_id[j], j, self.rev[j])

    def triangles(self, edges):
        """(e, a, b) for every edge e of `edges` (ids) and every common neighbour w of its ends: the ids of the two
        other edges of the triangle.  The shorter row is walked, the longer one searched."""
        out = []
        u, v = self.row[edges], self.col[edges]
        walk_u = self.deg[u] <= self.deg[v]
        p, q = np.where(walk_u, u, v), np.where(walk_u, v, u)
        length = self.deg[p]
        bounds = np.cumsum(length)
        start = 0
        while start < len(edges):
            stop = max(start + 1, int(np.searchsorted(bounds, (bounds[start - 1] if start else 0) + _CHUNK_PAIRS,
                                                      side='right')))
            ln = length[start:stop]
            total = int(ln.sum())
            if total:
                which = np.repeat(np.arange(start, stop, dtype=np.int64), ln)
                offset = np.cumsum(ln) - ln
                k = np.repeat(self.row_ptr[p[start:stop]] - offset, ln) + np.arange(total, dtype=np.int64)
                want = q[which] * self.n + self.col[k]
                lo = np.minimum(np.searchsorted(self.key, want), len(self.key) - 1)
                hit = self.key[lo] == want
                out.append((edges[which[hit]], self.edge_id(k[hit]), self.edge_id(lo[hit])))
            start = stop
        if not out:
            z = np.zeros(0, dtype=np.int64)
            return z, z, z
        return tuple(np.concatenate(part) for part in zip(*out))


def truss_numbers(row_ptr, col, dedupe: bool = True) -> Result:
    g = _Arcs(row_ptr, col)
    nnz = len(g.key)
    ids = np.nonzero(g.is_id)[0]
    sup = np.zeros(nnz, dtype=np.int64)
    e, _, _ = g.triangles(ids)
    if len(e):
        sup += np.bincount(e, minlength=nnz)
    state = np.zeros(nnz, dtype=np.int64)                       # 0 alive, r > 0: in F in round r
    state[~g.is_id] = -1
    truss = np.zeros(nnz, dtype=np.int32)
    thr, rnd, levels, last, left = 0, 0, 0, None, len(ids)
    decrements = frontier_max = 0
    while left:
        rnd += 1
        alive = state == 0
        F = np.nonzero(alive & (sup <= thr))[0]
        if not len(F):
            thr = int(sup[alive].min())
            F = np.nonzero(alive & (sup <= thr))[0]
        if thr != last:
            levels, last = levels + 1, thr
        truss[F] = truss[g.rev[F]] = thr + 2
        state[F] = rnd
        left -= len(F)
        frontier_max = max(frontier_max, len(F))
        e, a, b = g.triangles(F)
        keep = ~(((state[a] > 0) & (state[a] < rnd)) | ((state[b] > 0) & (state[b] < rnd)))
        e, a, b = e[keep], a[keep], b[keep]
        fa, fb = state[a] == rnd, state[b] == rnd
        neither = ~fa & ~fb
        only_a = fa & ~fb & ((e < a) if dedupe else True)
        only_b = fb & ~fa & ((e < b) if dedupe else True)
        targets = np.concatenate([a[neither], b[neither], b[only_a], a[only_b]])
        if len(targets):
            sup -= np.bincount(targets, minlength=nnz)
            decrements += len(targets)
    node = np.zeros(g.n, dtype=np.int64)
    if nnz:
        np.maximum.at(node, g.row, truss.astype(np.int64))
    return Result(truss, node, rnd, levels, decrements, frontier_max)


def graph_csr(G):
    """(nodelist, row_ptr, col) of an undirected networkx graph, rows in list(G) order."""
    from tests.kcore_oracle import symmetric_csr
    nodes = list(G)
    row_of = {v: i for i, v in enumerate(nodes)}
    return (nodes,) + symmetric_csr(len(nodes), [(row_of[u], row_of[v]) for u, v in G.edges()])


def networkx_truss_numbers(G):
    """({frozenset({u, v}): t(e)}, {v: t(v)}) from networkx alone: nx.k_truss(G, k) for k = 2, 3, 4, ... until the
    result is empty; t = the last k the edge (node) was seen in, 0 for a node that is in none."""
    import networkx as nx
    edge_t, node_t = {}, {v: 0 for v in G}
    k = 2
    while True:
        H = nx.k_truss(G, k)
        if H.number_of_nodes() == 0:
            return edge_t, node_t
        for u, v in H.edges():
            edge_t[frozenset((u, v))] = k
        for v in H:
            node_t[v] = k
        k += 1
