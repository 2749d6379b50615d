"""
Array restatement of grx_square_clustering (csrc/grx_square_clustering.hip) over (row_ptr, col) -- the CSR of the
distinct arcs of an undirected graph: symmetric, columns ascending and distinct inside a row, a diagonal entry a
self-loop.  For a row v with the entries N (d of them) and k_u the length of row u:
    K1   = sum_{u in N} k_u
    c(x) = |{u in N : x in row u}| for x != v        one np.unique(..., return_counts=True) over the concatenated rows
    Q    = sum_x c (c - 1) / 2                       networkx's `clustering` numerator
    S    = sum_{x in N, x != v} c(x),  L = |{x in N, x != v : x has a diagonal entry}|
    potential = (d - 1) (K1 - d) - (S - L + (d - 1) [v has a diagonal entry]) - Q
    C4   = Q / potential if potential > 0 else Q     Python's int / int; networkx divides only when potential > 0 and
                                                     leaves its numerator otherwise (not 0 only beside self-loops)
A row costs its own K1 wedges, so a few hundred rows of a graph whose whole A^2 would not fit are affordable.
"""
import numpy as np


def csr_from_pairs(n, pairs):
    """(row_ptr int64[n+1], col int32[nnz]) of the undirected graph with the edges `pairs` ((u, v) once per edge, any
    orientation, duplicates merged, (v, v) a self-loop)."""
    pairs = np.asarray(list(pairs), dtype=np.int64).reshape(-1, 2)
    key = np.unique(np.concatenate([pairs[:, 0] * n + pairs[:, 1], pairs[:, 1] * n + pairs[:, 0]]))
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // max(n, 1), minlength=n), out=row_ptr[1:])
    return row_ptr, (key % max(n, 1)).astype(np.int32)


def wedge_counts(row_ptr, col):
    """K1 int64[n]: the wedges v -> u -> x of every row v, the quantity the kernel bins its rows by."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    k = np.diff(row_ptr)
    total = np.concatenate([[0], np.cumsum(k[np.asarray(col, dtype=np.int64)[:row_ptr[-1]]])])
    return total[row_ptr[1:]] - total[row_ptr[:-1]]


def square_clustering(row_ptr, col, rows=None):
    """(Q int64[r], potential int64[r], C4 float64[r]) of the rows `rows` (None = every row, in order)."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n = len(row_ptr) - 1
    col = np.asarray(col, dtype=np.int64)[:row_ptr[-1]]
    k = np.diff(row_ptr)
    loop = np.zeros(n, dtype=np.int64)
    loop[col[col == np.repeat(np.arange(n), k)]] = 1
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    Q = np.zeros(len(rows), dtype=np.int64)
    P = np.zeros(len(rows), dtype=np.int64)
    C = np.zeros(len(rows), dtype=np.float64)
    for i, v in enumerate(rows):
        nb = col[row_ptr[v]:row_ptr[v + 1]]
        d, lens = len(nb), k[nb]
        k1 = int(lens.sum())
        # the concatenated rows of the neighbours
        at = np.arange(k1) - np.repeat(np.cumsum(lens) - lens, lens) + np.repeat(row_ptr[nb], lens)
        x, c = np.unique(col[at], return_counts=True)
        c = c[x != v].astype(np.int64)
        x = x[x != v]
        q = int((c * (c - 1) // 2).sum())
        others = nb[nb != v]
        found = np.searchsorted(x, others)
        found[found == len(x)] = 0
        s = int(c[found][x[found] == others].sum()) if len(x) else 0
        two_t = s - int(loop[others].sum()) + (d - 1) * int(loop[v])
        p = (d - 1) * (k1 - d) - two_t - q
        Q[i], P[i] = q, p
        C[i] = q / p if p > 0 else float(q)
    return Q, P, C
