"""
Two independent host implementations of the graphlet degree vectors (Przulj 2007; orbits 0-14 of the connected graphs
on 2, 3 and 4 nodes, INDUCED subgraphs) that csrc/grx_graphlets.hip computes:

``brute_orbits(G)``      the definition, and the authority: every 3- and 4-subset of every connected component is looked
                         at, the connected induced ones are classified by their number of edges and each node's degree
                         inside the subset, and the node's orbit gets 1.  O(n^4) per component: small graphs only.

``orbits(row_ptr, col)`` the restatement of the kernel's method over the CSR of the distinct arcs (symmetric, columns
                         ascending, no diagonal entry): the non-induced counts N0 .. N14 per node from d, t(e), t(v),
                         S1(v), Q(v) (the 4-cycles through v, sum_{x != v} C(c(x), 2) over row v of A^2) and K4(v) (the
                         4-cliques, listed from the triangles), then the back-substitution through A (N = A o).  For
                         graphs too large for brute force.  Q and K4 are computed here, not taken from another oracle.

    orbit  0        edge                      8         4-cycle
           1, 2     path on 3: end, middle    9, 10, 11 paw: pendant; triangle node off the tail; triangle node on it
           3        triangle                  12, 13    diamond: degree-2 node; degree-3 node
           4, 5     path on 4: end, interior  14        4-clique
           6, 7     claw: leaf, centre
"""
import itertools
from collections import namedtuple

import numpy as np

Result = namedtuple('Result', 'orbits noninduced arc_triangles')

#: N = A o: row k holds the coefficients of o0 .. o14 (tests/test_graphlet_cpu.py re-derives every row)
A = np.array([
    [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [0, 1, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 1, 0, 0, 0, 2, 2, 1, 0, 4, 2, 6],
    [0, 0, 0, 0, 0, 1, 0, 0, 2, 0, 1, 2, 2, 4, 6],
    [0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 2, 1, 3],
    [0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 1],
    [0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 1, 3],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 2, 0, 3],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 2, 2, 6],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 2, 3],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 3],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 3],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1],
], dtype=np.int64)

#: (edges of the induced subgraph on 4 nodes, degree of the node inside it) -> orbit; 3 and 4 edges need the degree
#: sequence as well (path against claw, cycle against paw)
_PATH4 = {1: 4, 2: 5}
_CLAW = {1: 6, 3: 7}
_PAW = {1: 9, 2: 10, 3: 11}
_DIAMOND = {2: 12, 3: 13}


def brute_orbits(G):
    """{node: [o0 .. o14]} of an undirected networkx graph without self-loops, by enumeration."""
    import networkx as nx
    out = {v: [0] * 15 for v in G}
    for v in G:
        out[v][0] = G.degree(v)
    for comp in nx.connected_components(G):
        nodes = list(comp)
        k = len(nodes)
        if k < 3:
            continue
        adj = np.zeros((k, k), dtype=bool)
        at = {v: i for i, v in enumerate(nodes)}
        for u in nodes:
            for w in G[u]:
                assert w != u, 'no self-loops'
                adj[at[u], at[w]] = True
        adj = adj.tolist()
        for a, b, c in itertools.combinations(range(k), 3):
            ab, ac, bc = adj[a][b], adj[a][c], adj[b][c]
            edges = ab + ac + bc
            if edges == 3:
                for i in (a, b, c):
                    out[nodes[i]][3] += 1
            elif edges == 2:
                for i, deg in ((a, ab + ac), (b, ab + bc), (c, ac + bc)):
                    out[nodes[i]][deg] += 1                      # end: degree 1 -> orbit 1; middle: 2 -> orbit 2
        for sub in itertools.combinations(range(k), 4):
            deg = [sum(adj[i][j] for j in sub) for i in sub]
            edges = sum(deg) // 2
            if edges < 3 or min(deg) == 0:
                continue                                        # not connected (3 edges: a triangle beside a node)
            if edges == 3:
                table = _CLAW if max(deg) == 3 else _PATH4
            elif edges == 4:
                table = _PAW if max(deg) == 3 else None
            elif edges == 5:
                table = _DIAMOND
            else:
                table = None
            for i, d in zip(sub, deg):
                out[nodes[i]][8 if edges == 4 and table is None else 14 if edges == 6 else table[d]] += 1
    return out


def orbits(row_ptr, col) -> Result:
    """Result(orbits int64[15, n], noninduced int64[15, n], arc_triangles int32[nnz]) by the kernel's formulas."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n = len(row_ptr) - 1
    nnz = int(row_ptr[-1])
    col = np.asarray(col, dtype=np.int64)[:nnz]
    d = np.diff(row_ptr)
    row = np.repeat(np.arange(n, dtype=np.int64), d)
    assert not np.any(row == col), 'no self-loops'
    nbrs = [set(col[row_ptr[v]:row_ptr[v + 1]].tolist()) for v in range(n)]
    assert all(v in nbrs[u] for v in range(n) for u in nbrs[v]), 'symmetric'

    def per_row(values):
        """sum of the per-arc `values` over every row"""
        total = np.concatenate([[0], np.cumsum(values, dtype=np.int64)])
        return total[row_ptr[1:]] - total[row_ptr[:-1]]

    # t(e) per arc, the triangles once each (a < b < c), K4 from them
    t_arc = np.zeros(nnz, dtype=np.int64)
    t_of = {}
    triangles = []
    for j in range(nnz):
        u, v = int(row[j]), int(col[j])
        if u < v:
            common = nbrs[u] & nbrs[v]
            t_of[(u, v)] = t_of[(v, u)] = len(common)
            triangles.extend((u, v, w) for w in common if w > v)
        # (v, u) with v < u came first: rows ascend
        t_arc[j] = t_of[(u, v)]
    t = per_row(t_arc) // 2
    k4 = np.zeros(n, dtype=np.int64)
    n12 = np.zeros(n, dtype=np.int64)
    for a, b, c in triangles:
        n12[a] += t_of[(b, c)] - 1
        n12[b] += t_of[(a, c)] - 1
        n12[c] += t_of[(a, b)] - 1
        for x in nbrs[a] & nbrs[b] & nbrs[c]:
            if x > c:
                k4[[a, b, c, x]] += 1
    # Q(v) = sum_{x != v} C(c(x), 2), c = row v of A^2
    q = np.zeros(n, dtype=np.int64)
    for v in range(n):
        nb = col[row_ptr[v]:row_ptr[v + 1]]
        if len(nb):
            two_hop = np.concatenate([col[row_ptr[u]:row_ptr[u + 1]] for u in nb])
            c = np.bincount(two_hop[two_hop != v])
            q[v] = int((c * (c - 1) // 2).sum())

    du = d[col]
    s1 = per_row(du - 1)
    non = np.zeros((15, n), dtype=np.int64)
    non[0] = d
    non[1] = s1
    non[2] = d * (d - 1) // 2
    non[3] = t
    non[4] = per_row(s1[col] - (d[row] - 1)) - 2 * t
    non[5] = per_row((d[row] - 1) * (du - 1) - t_arc)
    non[6] = per_row((du - 1) * (du - 2) // 2)
    non[7] = d * (d - 1) * (d - 2) // 6
    non[8] = q
    non[9] = per_row(t[col] - t_arc)
    non[10] = per_row(t_arc * (du - 2))
    non[11] = t * (d - 2)
    non[12] = n12
    non[13] = per_row(t_arc * (t_arc - 1) // 2)
    non[14] = k4
    o = non.copy()
    for k in range(13, -1, -1):
        o[k] -= A[k, k + 1:] @ o[k + 1:]
    return Result(o, non, t_arc.astype(np.int32))


def graph_orbits(G):
    """{node: [o0 .. o14]} of a networkx graph through ``orbits`` (rows in list(G) order)."""
    from tests.truss_oracle import graph_csr
    nodes, row_ptr, col = graph_csr(G)
    o = orbits(row_ptr, col).orbits
    return {v: o[:, i].tolist() for i, v in enumerate(nodes)}
