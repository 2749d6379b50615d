"""
Array restatements of grx_clustering (csrc/grx_clustering.hip) over (row_ptr, col, fwd, bwd, max_weight) -- a
structurally symmetric CSR with ascending columns that lists every neighbour in either direction, the weight of u -> v
(fwd) and of v -> u (bwd) at arc (u, v) with a negative value for an absent direction, bwd None for an undirected graph
and fwd None for an undirected graph without weights:

  exact   every quotient w / max_weight, every cube root, every product s * s and s * sum and the add of the two
          directions as one fp64 operation, as the kernel forms them, every sum by math.fsum: what the kernel would give
          with correctly rounded sums.  Small cases.
  sparse  scipy.sparse: the row sums of ((S S) o S) with the diagonal of S removed.  The large case.

and the builders of those arrays from a networkx graph of either kind or from a list of pairs, and the tolerances,
defined once.
"""
import math

import networkx as nx
import numpy as np

#: clustering and its numerator t: every term is >= 0, so device, oracle and networkx differ only by rounding.  Per
#: term a few ulp: here a division, a cube root (libm's and the device's are each within 1 ulp, not correctly rounded),
#: two products and -- directed -- one add per factor, against networkx's three divisions, two products and one cube
#: root; then (k - 1) 2^-53 relative for each of the two nested sums of k <= (row length) terms, and one final
#: division: together under 5e-13 for rows of up to 2 000 entries.  The test graphs keep their largest row at or below
#: MAX_ROW.
RTOL = 1e-12
MAX_ROW = 2000


def directional_csr(G, weight=None, nodes=None):
    """(row_ptr, col, fwd, bwd, max_weight) of a networkx Graph or DiGraph with rows in the order of `nodes` (default:
    sorted): row u lists set(nx.all_neighbors(G, u)) ascending (u itself when it has a loop).  Directed: fwd / bwd hold
    the weight of u -> v / v -> u, -1 where the arc is absent; undirected: fwd the weight, bwd None, and with
    weight=None fwd None as well.  A missing attribute counts 1, weight=None every edge 1; max_weight is networkx's
    (over every edge, loops included; 1 without weights or edges)."""
    nodes = sorted(G) if nodes is None else list(nodes)
    row_of = {v: i for i, v in enumerate(nodes)}
    directed = G.is_directed()

    def one_way(u, v):
        if not G.has_edge(u, v):
            return -1.0
        return float(G[u][v].get(weight, 1)) if weight is not None else 1.0

    row_ptr, col, fwd, bwd = [0], [], [], []
    for u in nodes:
        for v in sorted(set(nx.all_neighbors(G, u)), key=row_of.get):
            col.append(row_of[v])
            fwd.append(one_way(u, v))
            bwd.append(one_way(v, u))
        row_ptr.append(len(col))
    if weight is None or G.number_of_edges() == 0:
        max_weight = 1.0
    else:
        max_weight = float(max(d.get(weight, 1) for _, _, d in G.edges(data=True)))
    fwd_a = np.asarray(fwd, dtype=np.float64) if (directed or weight is not None) else None
    bwd_a = np.asarray(bwd, dtype=np.float64) if directed else None
    return np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int32), fwd_a, bwd_a, max_weight


def csr_from_pairs(n, pairs, w_of=None):
    """Symmetric CSR of the undirected pairs (u, v) (u == v: a diagonal entry): (row_ptr, col, fwd or None,
    max_weight); w_of(u, v) with u <= v gives the weight of a pair."""
    entries = {}
    for u, v in pairs:
        a, b = min(u, v), max(u, v)
        val = 1.0 if w_of is None else float(w_of(a, b))
        entries[(a, b)] = val
        entries[(b, a)] = val
    keys = sorted(entries)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount([k[0] for k in keys], minlength=n), out=row_ptr[1:])
    col = np.asarray([k[1] for k in keys], dtype=np.int32)
    if w_of is None:
        return row_ptr, col, None, 1.0
    fwd = np.asarray([entries[k] for k in keys], dtype=np.float64)
    return row_ptr, col, fwd, float(fwd.max()) if len(fwd) else 1.0


def _root(w, max_weight):
    q = w / max_weight
    return 1.0 if q == 1.0 else float(np.cbrt(q))


def arc_values(row_ptr, fwd, bwd, max_weight):
    """(s per arc, directions present per arc) as Python lists."""
    nnz = int(row_ptr[-1])
    if fwd is None:
        return [1.0] * nnz, [1] * nnz
    f = np.asarray(fwd, dtype=np.float64).tolist()
    if bwd is None:
        return [_root(x, max_weight) for x in f], [1] * nnz
    b = np.asarray(bwd, dtype=np.float64).tolist()
    s = [(_root(x, max_weight) if x >= 0 else 0.0) + (_root(y, max_weight) if y >= 0 else 0.0) for x, y in zip(f, b)]
    return s, [(x >= 0) + (y >= 0) for x, y in zip(f, b)]


def denominators(row_ptr, col, dirs, directed):
    """d (d - 1) resp. 2 (dt (dt - 1) - 2 db) of every row, as Python ints."""
    rp, cl = np.asarray(row_ptr).tolist(), np.asarray(col).tolist()
    out = []
    for u in range(len(rp) - 1):
        off = [j for j in range(rp[u], rp[u + 1]) if cl[j] != u]
        d = len(off)
        dt = sum(dirs[j] for j in off)
        out.append(2 * (dt * (dt - 1) - 2 * (dt - d)) if directed else d * (d - 1))
    return out


def exact(row_ptr, col, fwd=None, bwd=None, max_weight=1.0):
    """(clustering fp64[n], t fp64[n])."""
    rp = np.asarray(row_ptr, dtype=np.int64).tolist()
    cl = np.asarray(col, dtype=np.int64).tolist()
    n = len(rp) - 1
    s, dirs = arc_values(row_ptr, fwd, bwd, max_weight)
    den = denominators(row_ptr, col, dirs, bwd is not None)
    pos = [dict(zip(cl[rp[u]:rp[u + 1]], range(rp[u], rp[u + 1]))) for u in range(n)]
    t = [0.0] * n
    for u in range(n):
        terms = []
        for j in range(rp[u], rp[u + 1]):
            v = cl[j]
            if v == u:
                continue
            in_v = pos[v]
            inner = []
            for ku in range(rp[u], rp[u + 1]):
                w = cl[ku]
                kv = in_v.get(w)
                if kv is None or w == u or w == v:
                    continue
                inner.append(s[ku] * s[kv])
            terms.append(s[j] * math.fsum(inner))
        t[u] = math.fsum(terms)
    c = np.array([0.0 if t[u] == 0 else t[u] / den[u] for u in range(n)], dtype=np.float64)
    return c, np.asarray(t, dtype=np.float64)


def sparse(row_ptr, col, fwd=None, bwd=None, max_weight=1.0):
    """The same two arrays from scipy.sparse products."""
    import scipy.sparse as sp
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n, nnz = len(row_ptr) - 1, int(row_ptr[-1])
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    if fwd is None:
        s, dirs = np.ones(nnz), np.ones(nnz)
    else:
        def root(x):
            q = np.where(x >= 0, x, 0.0) / max_weight
            return np.where(x >= 0, np.where(q == 1.0, 1.0, np.cbrt(q)), 0.0)
        f = np.asarray(fwd, dtype=np.float64)
        if bwd is None:
            s, dirs = root(f), np.ones(nnz)
        else:
            b = np.asarray(bwd, dtype=np.float64)
            s, dirs = root(f) + root(b), (f >= 0).astype(np.float64) + (b >= 0)
    off = rows != col
    S = sp.csr_matrix((s[off], (rows[off], col[off])), shape=(n, n))
    t = np.asarray((S @ S).multiply(S).sum(axis=1)).ravel() if nnz else np.zeros(n)
    d = np.bincount(rows[off], minlength=n).astype(np.float64)
    dt = np.bincount(rows[off], weights=dirs[off], minlength=n)
    den = 2 * (dt * (dt - 1) - 2 * (dt - d)) if bwd is not None else d * (d - 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        c = np.where(t == 0, 0.0, t / np.where(t == 0, 1.0, den))
    return c, t


def assert_close(got, want, what=''):
    """Exact zeros in the same places, RTOL relative elsewhere."""
    g, w = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g == 0, w == 0), (what, 'zero places', np.nonzero((g == 0) != (w == 0))[0][:5])
    err, bound = np.abs(g - w), RTOL * np.abs(w)
    worst = int(np.argmax(err - bound)) if len(err) else 0
    assert np.all(err <= bound), (what, worst, float(err[worst]), float(bound[worst]))
