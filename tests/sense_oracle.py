"""
numpy / scipy restatements of the networkx 3.4.2 loops behind graphrole_amd.node_measures, with the iteration
counts networkx does not return: pagerank_alg.py::_pagerank_scipy and eigenvector.py::eigenvector_centrality, plus
the array forms the full-size tests use (a 1 M-node graph is not held as a networkx object).  No reference code.
"""
import math

import networkx as nx
import numpy as np
import scipy.sparse as sp


def pagerank(G, alpha=0.85, max_iter=100, tol=1e-6, weight='weight'):
    """(label -> value, iterations) of networkx's _pagerank_scipy (personalization / nstart / dangling None)."""
    nodelist = list(G)
    A = nx.to_scipy_sparse_array(G, nodelist=nodelist, weight=weight, dtype=float)
    x, it = pagerank_matrix(A, alpha, max_iter, tol)
    return dict(zip(nodelist, map(float, x))), it


def pagerank_matrix(A, alpha=0.85, max_iter=100, tol=1e-6):
    """The loop of _pagerank_scipy on an adjacency matrix (row = source)."""
    N = A.shape[0]
    S = np.asarray(A.sum(axis=1)).ravel()
    S[S != 0] = 1.0 / S[S != 0]
    Q = sp.csr_array(sp.spdiags(S.T, 0, *A.shape))
    A = Q @ A
    x = np.repeat(1.0 / N, N)
    p = np.repeat(1.0 / N, N)
    dangling_weights = p
    is_dangling = np.where(S == 0)[0]
    for it in range(1, max_iter + 1):
        xlast = x
        x = alpha * (x @ A + sum(x[is_dangling]) * dangling_weights) + (1 - alpha) * p
        err = np.absolute(x - xlast).sum()
        if err < N * tol:
            return x, it
    raise nx.PowerIterationFailedConvergence(max_iter)


def eigenvector(G, max_iter=100, tol=1e-6, weight='weight'):
    """(label -> value, iterations) of networkx's eigenvector_centrality (nstart None)."""
    nstart = {v: 1 for v in G}
    nstart_sum = sum(nstart.values())
    x = {k: v / nstart_sum for k, v in nstart.items()}
    nnodes = G.number_of_nodes()
    for it in range(1, max_iter + 1):
        xlast = x
        x = xlast.copy()
        for n in x:
            for nbr in G[n]:
                w = G[n][nbr].get(weight, 1) if weight else 1
                x[nbr] += xlast[n] * w
        norm = math.hypot(*x.values()) or 1
        x = {k: v / norm for k, v in x.items()}
        if sum(abs(x[n] - xlast[n]) for n in x) < nnodes * tol:
            return x, it
    raise nx.PowerIterationFailedConvergence(max_iter)


def csr_adjacency(g):
    """scipy adjacency (row = source, weights or 1) of a graphrole_amd CSRGraph in label order."""
    w = g.w if g.w is not None else np.ones(len(g.col))
    return sp.csr_array((w, g.col.astype(np.int64), g.row_ptr), shape=(g.n, g.n))


def clustering_arrays(g):
    """nx.clustering of an undirected CSRGraph without self-loops, from per-node triangle counts: with the arcs
    oriented from lower to higher (degree, index), a triangle a -> b -> c, a -> c counts once at a (row sums of
    P = (L L) o L), once at c (column sums of P) and once at b (row sums of (L^T L) o L)."""
    n = g.n
    deg = np.diff(g.row_ptr)
    rows = np.repeat(np.arange(n, dtype=np.int64), deg)
    col = g.col.astype(np.int64)
    assert not np.any(rows == col)
    keep = (deg[rows] < deg[col]) | ((deg[rows] == deg[col]) & (rows < col))
    L = sp.csr_array((np.ones(int(keep.sum()), dtype=np.int64), (rows[keep], col[keep])), shape=(n, n))
    P = (L @ L).multiply(L)
    B = (L.T @ L).multiply(L)
    T = (np.asarray(P.sum(axis=1)).ravel() + np.asarray(P.sum(axis=0)).ravel()
         + np.asarray(B.sum(axis=1)).ravel()).astype(np.int64)
    out = np.zeros(n)
    nz = T > 0
    out[nz] = (2 * T[nz]).astype(np.float64) / (deg[nz] * (deg[nz] - 1)).astype(np.float64)
    return out
