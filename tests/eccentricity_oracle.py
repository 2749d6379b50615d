"""
numpy restatement of grx_eccentricity (csrc/grx_closeness.hip) and of the bounds method of
graphrole_amd.eccentricity on CSR arrays: what one kernel call leaves in its four arrays, bounds updates included,
and the rounds of the host driver with its source-selection rule.  One BFS per source (tests/closeness_oracle.py's
bfs_levels) into a dense sources x nodes distance table: for small graphs only.  No reference code.

As the kernel, ``eccentricity_pass`` PULLS over the CSR it is given: the BFS from a source walks the arcs of the
transposed CSR.  An undirected graph's CSR is both.
"""
import networkx as nx
import numpy as np

from tests.betweenness_oracle import csr_of  # noqa: F401  (re-exported)
from tests.closeness_oracle import bfs_levels, transpose

INF = int(np.iinfo(np.int32).max)


def distance_table(row_ptr, col, sources):
    """int64[len(sources), n]: distances from every source along the transposed CSR, -1 = not reached; a source
    outside [0, n) reaches nothing, itself included."""
    n = len(row_ptr) - 1
    t_ptr, t_col = transpose(row_ptr, col)
    D = np.full((len(sources), n), -1, dtype=np.int64)
    for k, s in enumerate(np.asarray(sources, dtype=np.int64).tolist()):
        if 0 <= s < n:
            D[k] = bfs_levels(t_ptr, t_col, s)
    return D


def eccentricity_pass(row_ptr, col, sources, lower=None, upper=None, want_upper=False):
    """(source_ecc int32[len(sources)], reach int64[n], lower int32[n], upper int32[n] or None) as one grx_eccentricity
    call defines them.  lower=None: accumulate = 0 (lower = 0, and with want_upper upper = INT32_MAX; without it there
    is no upper and no pass B); otherwise the call continues from copies of `lower` and `upper` (upper may be None)."""
    n = len(row_ptr) - 1
    D = distance_table(row_ptr, col, sources)
    if lower is None:
        lower = np.zeros(n, dtype=np.int32)
        upper = np.full(n, INF, dtype=np.int32) if want_upper else None
    else:
        lower = np.array(lower, dtype=np.int32)
        upper = None if upper is None else np.array(upper, dtype=np.int32)
    source_ecc = D.max(axis=1, initial=0).clip(min=0).astype(np.int32)
    reach = (D > 0).sum(axis=0).astype(np.int64)
    # pass A: the per-target maximum distance over the levels >= 1
    lower = np.maximum(lower, D.max(axis=0, initial=0).clip(min=0).astype(np.int32))
    if upper is not None:
        # pass B: every (source, node) pair with a path, the source itself at distance 0 included
        for k in range(len(D)):
            hit = D[k] >= 0
            e = int(source_ecc[k])
            upper[hit] = np.minimum(upper[hit], (D[k][hit] + e).astype(np.int32))
            lower[hit] = np.maximum(lower[hit], (e - D[k][hit]).astype(np.int32))
    return source_ecc, reach, lower, upper


def select_sources(lower, upper, degree, batch):
    """The selection rule of the bounds method, written out with sorts: among the unresolved rows (lower < upper) half
    the batch by the largest upper bound, then the other half by the smallest lower bound among the rows not yet
    taken; ties by larger degree, then smaller row.  Every unresolved row when no more than `batch` are left."""
    open_rows = np.nonzero(np.asarray(lower) < np.asarray(upper))[0]
    if len(open_rows) <= batch:
        return open_rows
    by_upper = sorted(open_rows.tolist(), key=lambda v: (-int(upper[v]), -int(degree[v]), v))
    taken = by_upper[:batch // 2]
    rest = set(open_rows.tolist()) - set(taken)
    by_lower = sorted(rest, key=lambda v: (int(lower[v]), -int(degree[v]), v))
    return np.array(sorted(taken + by_lower[:batch - batch // 2]), dtype=np.int64)


def not_connected(directed):
    return nx.NetworkXError('Found infinite path length because the digraph is not strongly connected' if directed
                            else 'Found infinite path length because the graph is not connected')


def require_full_reach(reach, sources, directed):
    n = len(reach)
    if np.any(reach + np.bincount(sources, minlength=n) != len(sources)):
        raise not_connected(directed)


def bounds_rounds(row_ptr, col, batch):
    """The rounds of the bounds method on a symmetric CSR: yields (sources, lower, upper) after every round until no
    row is unresolved; raises networkx's error after the first round when the graph is not connected."""
    n = len(row_ptr) - 1
    degree = np.diff(np.asarray(row_ptr, dtype=np.int64))
    lower = np.zeros(n, dtype=np.int32)
    upper = np.full(n, INF, dtype=np.int32)
    first = True
    while np.any(lower < upper):
        sources = select_sources(lower, upper, degree, batch)
        _, reach, lower, upper = eccentricity_pass(row_ptr, col, sources, lower, upper)
        if first:
            require_full_reach(reach, sources, False)
            first = False
        yield sources, lower, upper


def eccentricity(row_ptr, col, method='all', batch=64, directed=False):
    """int64[n]: every row's eccentricity along the arcs of the TRANSPOSE of (row_ptr, col) -- pass the in-adjacency
    of a directed graph -- by either method; (values, rounds, sources used)."""
    n = len(row_ptr) - 1
    if method == 'all' or directed:
        sources = np.arange(n, dtype=np.int64)
        ecc, reach, _, _ = eccentricity_pass(row_ptr, col, sources)
        require_full_reach(reach, sources, directed)
        return ecc.astype(np.int64), 1, n
    rounds = used = 0
    lower = np.zeros(n, dtype=np.int32)
    for sources, lower, _ in bounds_rounds(row_ptr, col, batch):
        rounds += 1
        used += len(sources)
    return lower.astype(np.int64), rounds, used


def pull_csr(G, nodelist):
    """(row_ptr, col) to pull over for the BFS along G's out-arcs: the in-adjacency (an undirected graph's own CSR)."""
    return csr_of(G.reverse(copy=False) if G.is_directed() else G, nodelist)
