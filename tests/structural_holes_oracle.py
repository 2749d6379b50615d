"""
Array restatements of grx_structural_holes (csrc/grx_structural_holes.hip) over (row_ptr, col, z, out_row_ptr) -- a
structurally symmetric CSR with ascending columns, its symmetric mutual weights (None = all 1) and the row pointers that
tell len(G[u]) (None = the CSR's own):

  exact   every quotient z / S, z / X and every product P * P, P * M as one fp64 operation, as the kernel forms them,
          every sum by math.fsum (S included): what the kernel would give with correctly rounded sums.  Small cases.
  sparse  scipy.sparse: (P + P P) o mask and (P M^T) o mask.  The large case.

and the builders of that CSR from a networkx graph of either kind, and the tolerances, defined once.
"""
import math

import networkx as nx
import numpy as np

#: constraint and local constraint: every term is >= 0, so device and oracle differ only in how a sum of k <= (row
#: length) terms is rounded -- at most (k - 1) 2^-53 relative, twice in a row (S, then the sum over w), doubled by the
#: square: under 5e-13 for rows of up to 2 000 entries.  The test graphs keep their largest row at or below MAX_ROW.
RTOL = 1e-12
MAX_ROW = 2000
#: effective size: each of the d(u) terms 1 - r lies in [0, 1] and r carries at most (k + 2) 2^-53 absolute error:
#: |got - want| <= ES_ATOL * max(d(u), 1), absolute because the terms cancel
ES_ATOL = 1e-12


def mutual_csr(G, weight=None, nodes=None):
    """(row_ptr, col, z, out_row_ptr) of a networkx Graph or DiGraph with rows in the order of `nodes` (default:
    sorted): row u lists set(nx.all_neighbors(G, u)) ascending, z is networkx's mutual_weight (an undirected edge 2 w, a
    loop twice, a missing attribute 1, weight=None every edge 1), out_row_ptr counts len(G[u])."""
    nodes = sorted(G) if nodes is None else list(nodes)
    row_of = {v: i for i, v in enumerate(nodes)}

    def one_way(u, v):
        if not G.has_edge(u, v):
            return 0
        return G[u][v].get(weight, 1) if weight is not None else 1

    row_ptr, out_row_ptr, col, z = [0], [0], [], []
    for u in nodes:
        for v in sorted(set(nx.all_neighbors(G, u)), key=row_of.get):
            col.append(row_of[v])
            z.append(float(one_way(u, v) + one_way(v, u)))
        row_ptr.append(len(col))
        out_row_ptr.append(out_row_ptr[-1] + len(G[u]))
    return (np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int32), np.asarray(z, dtype=np.float64),
            np.asarray(out_row_ptr, dtype=np.int64))


def csr_from_pairs(n, pairs, z_of=None):
    """Symmetric CSR of the undirected pairs (u, v) (u == v: a diagonal entry): (row_ptr, col, z or None); z_of(u, v)
    with u <= v gives the mutual weight of a pair."""
    entries = {}
    for u, v in pairs:
        a, b = min(u, v), max(u, v)
        val = 1.0 if z_of is None else float(z_of(a, b))
        entries[(a, b)] = val
        entries[(b, a)] = val
    keys = sorted(entries)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount([k[0] for k in keys], minlength=n), out=row_ptr[1:])
    col = np.asarray([k[1] for k in keys], dtype=np.int32)
    z = None if z_of is None else np.asarray([entries[k] for k in keys], dtype=np.float64)
    return row_ptr, col, z


def exact(row_ptr, col, z=None, out_row_ptr=None):
    """(constraint fp64[n], effective_size fp64[n], local fp64[nnz])."""
    rp = np.asarray(row_ptr, dtype=np.int64).tolist()
    cl = np.asarray(col, dtype=np.int64).tolist()
    n, nnz = len(rp) - 1, rp[-1]
    zz = [1.0] * nnz if z is None else np.asarray(z, dtype=np.float64).tolist()
    orp = rp if out_row_ptr is None else np.asarray(out_row_ptr, dtype=np.int64).tolist()
    S = [math.fsum(zz[rp[u]:rp[u + 1]]) for u in range(n)]
    X = [max(zz[rp[u]:rp[u + 1]], default=0.0) for u in range(n)]
    pos = [dict(zip(cl[rp[u]:rp[u + 1]], range(rp[u], rp[u + 1]))) for u in range(n)]
    local = [0.0] * nnz
    keep = [0.0] * nnz                                          # 1 - redundancy of the arc
    for u in range(n):
        su = S[u]
        for j in range(rp[u], rp[u + 1]):
            v = cl[j]
            xv, in_v = X[v], pos[v]
            ta, tb = [], []
            for ku in range(rp[u], rp[u + 1]):
                w = cl[ku]
                kv = in_v.get(w)
                if kv is None:
                    continue
                puw = zz[ku] / su if su != 0.0 else 0.0
                pwv = zz[kv] / S[w] if S[w] != 0.0 else 0.0
                mvw = zz[kv] / xv if xv != 0.0 else 0.0
                ta.append(puw * pwv)
                tb.append(puw * mvw)
            puv = zz[j] / su if su != 0.0 else 0.0
            t = puv + math.fsum(ta)
            local[j] = t * t
            keep[j] = 1.0 - math.fsum(tb)
    con = np.array([math.fsum(local[rp[u]:rp[u + 1]]) if orp[u + 1] > orp[u] else math.nan for u in range(n)])
    es = np.array([math.fsum(keep[rp[u]:rp[u + 1]]) if orp[u + 1] > orp[u] else math.nan for u in range(n)])
    return con, es, np.asarray(local, dtype=np.float64)


def sparse(row_ptr, col, z=None, out_row_ptr=None):
    """The same three arrays from scipy.sparse products."""
    import scipy.sparse as sp
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n, nnz = len(row_ptr) - 1, int(row_ptr[-1])
    zz = np.ones(nnz) if z is None else np.asarray(z, dtype=np.float64)
    deg = np.diff(row_ptr)
    rows = np.repeat(np.arange(n, dtype=np.int64), deg)
    Z = sp.csr_matrix((zz, (rows, col)), shape=(n, n))
    mask = sp.csr_matrix((np.ones(nnz), (rows, col)), shape=(n, n))
    S = np.asarray(Z.sum(axis=1)).ravel()
    X = np.asarray(Z.max(axis=1).todense()).ravel() if nnz else np.zeros(n)
    with np.errstate(divide='ignore'):
        inv_s = np.where(S != 0, 1.0 / np.where(S != 0, S, 1.0), 0.0)
        inv_x = np.where(X != 0, 1.0 / np.where(X != 0, X, 1.0), 0.0)
    P = sp.diags(inv_s) @ Z
    M = sp.diags(inv_x) @ Z
    T = (P + (P @ P).multiply(mask)).tocsr()
    local = np.asarray(T[rows, col]).ravel() ** 2 if nnz else np.zeros(0)
    con = np.asarray(T.power(2).sum(axis=1)).ravel()
    es = deg - np.asarray((P @ M.T).multiply(mask).sum(axis=1)).ravel()
    out_deg = deg if out_row_ptr is None else np.diff(np.asarray(out_row_ptr, dtype=np.int64))
    con = np.where(out_deg > 0, con, np.nan)
    es = np.where(out_deg > 0, es, np.nan)
    return con, es, local


def assert_close(got, want, row_ptr, what=''):
    """(constraint, effective_size, local) triples, an entry None where it was not computed: NaNs in the same places,
    RTOL on constraint and local, ES_ATOL * max(d, 1) on effective size."""
    deg = np.maximum(np.diff(np.asarray(row_ptr, dtype=np.int64)), 1)
    for k, name in enumerate(('constraint', 'effective_size', 'local')):
        if got[k] is None or want[k] is None:
            continue
        g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, name, 'NaN places')
        ok = ~np.isnan(w)
        err = np.abs(g[ok] - w[ok])
        bound = ES_ATOL * deg[ok] if name == 'effective_size' else RTOL * np.abs(w[ok])
        worst = int(np.argmax(err - bound)) if len(err) else 0
        assert np.all(err <= bound), (what, name, float(err[worst]), float(bound[worst]))
