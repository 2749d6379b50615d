"""
numpy restatement of grx_weighted_distances (csrc/grx_sssp.hip): Jacobi Bellman-Ford rounds on the pulled CSR from
+inf, a batch of sources at a time, then the per-target running sums in source order.  With weights >= 0 the fixed
point is the minimum over the paths of the left-to-right fp64 sum of the arc weights -- networkx's Dijkstra distance,
bit for bit (tests/test_weighted_distances_cpu.py checks that) -- so the kernel is compared with this module exactly:
distances, sums and the number of rounds.  Also the weighted test graphs both test files share.
"""
import networkx as nx
import numpy as np

#: harmonic and non-integer closeness against networkx: two sequential sums of at most 2 000 non-negative terms in
#: different orders differ by at most 2 (n - 1) 2^-53 ~ 4.4e-13 relative (closeness_oracle.HARMONIC_RTOL is the same)
RTOL = 1e-12

MIXED = (0.0, 1e-17, 0.1, 0.3, 1.0, 3.0, 1e16)                  # zero weights, ties, absorption


def with_weights(G, kind: str, seed: int = 0):
    """A copy of G with seeded edge weights: 'uniform' floats in [0.05, 1), 'ints' 1..5, 'mixed' drawn from MIXED."""
    H = G.copy()
    rng = np.random.default_rng(seed)
    for u, v in H.edges():
        if kind == 'uniform':
            H[u][v]['weight'] = float(rng.uniform(0.05, 1.0))
        elif kind == 'ints':
            H[u][v]['weight'] = int(rng.integers(1, 6))
        else:
            H[u][v]['weight'] = float(MIXED[int(rng.integers(0, len(MIXED)))])
    return H


def detour_graph():
    """5 nodes: the direct arc 0 - 4 weighs 10, the lightest path 0 - 1 - 2 - 3 - 4 has four hops and weighs 4."""
    G = nx.Graph()
    G.add_weighted_edges_from([(0, 4, 10.0), (0, 1, 1.0), (1, 2, 1.0), (2, 3, 1.0), (3, 4, 1.0)])
    return G


def pulled_csr(G, weight='weight'):
    """(labels, row_ptr, col, w) of the CSR a walk along G's out-arcs pulls over: row v lists the u with an arc
    u -> v and its weight (a missing attribute counts 1; weight=None: every arc 1).  Rows are the sorted labels."""
    labels = sorted(G.nodes)
    row_of = {v: i for i, v in enumerate(labels)}
    into = G.pred if G.is_directed() else G.adj
    row_ptr, col, w = [0], [], []
    for v in labels:
        for u, data in sorted(into[v].items(), key=lambda item: row_of[item[0]]):
            col.append(row_of[u])
            w.append(1.0 if weight is None else float(data.get(weight, 1)))
        row_ptr.append(len(col))
    return labels, np.array(row_ptr, dtype=np.int64), np.array(col, dtype=np.int64), np.array(w, dtype=np.float64)


def batch_width(batch: int, n_sources: int) -> int:
    """The library's choice of S for batch = 0 on a graph whose state fits the budget at every width."""
    if batch:
        return batch
    return 16 if n_sources <= 16 else 32 if n_sources <= 32 else 64


def relax(row_ptr, col, w, sources):
    """(dist[len(sources), n], rounds) of one batch: rounds until one changes nothing, that one included."""
    n = len(row_ptr) - 1
    D = np.full((n, len(sources)), np.inf)
    for b, s in enumerate(sources):
        if 0 <= s < n:
            D[s, b] = 0.0
    starts = row_ptr[:-1][np.diff(row_ptr) > 0]
    filled = np.nonzero(np.diff(row_ptr) > 0)[0]
    rounds = 0
    while True:
        rounds += 1
        new = D.copy()
        if len(col):
            cand = D[col] + w[:, None]                          # fl(dist(u, b) + w(u -> v)) per arc
            new[filled] = np.minimum(D[filled], np.minimum.reduceat(cand, starts, axis=0))
        if np.array_equal(new, D):
            return np.ascontiguousarray(D.T), rounds
        D = new


def weighted_distances(row_ptr, col, w, sources, batch: int = 0):
    """(reach int64[n], dsum, harmonic, far fp64[n], source_ecc fp64[len(sources)], dist[len(sources), n], rounds) as
    the kernel forms them: the sums left to right in the order of `sources`."""
    n = len(row_ptr) - 1
    sources = np.asarray(sources, dtype=np.int64)
    S = batch_width(batch, len(sources))
    parts, rounds = [], 0
    for first in range(0, len(sources), S):
        dist, r = relax(row_ptr, col, w, sources[first:first + S])
        parts.append(dist)
        rounds += r
    dist = np.concatenate(parts) if parts else np.empty((0, n))
    reach = np.zeros(n, dtype=np.int64)
    dsum, harmonic, far = np.zeros(n), np.zeros(n), np.zeros(n)
    source_ecc = np.zeros(len(sources))
    rows = np.arange(n)
    for b, s in enumerate(sources):
        d = dist[b]
        finite = np.isfinite(d)
        ok = finite & (rows != s)
        reach += ok
        dsum[ok] += d[ok]
        pos = ok & (d > 0)
        harmonic[pos] += 1.0 / d[pos]
        far[ok] = np.maximum(far[ok], d[ok])
        source_ecc[b] = d[finite].max() if finite.any() else 0.0
    return reach, dsum, harmonic, far, source_ecc, dist, rounds


def closeness(reach, dsum, n: int, wf_improved: bool = True):
    """networkx's closeness from len(sp) - 1 = reach and totsp = dsum, its own three IEEE operations."""
    out = np.zeros(len(reach))
    for v in range(len(reach)):
        if dsum[v] > 0.0 and n > 1:
            c = float(reach[v]) / float(dsum[v])
            if wf_improved:
                c *= float(reach[v]) / (n - 1)
            out[v] = c
    return out


def networkx_matrix(G, sources, weight='weight'):
    """dist[len(sources), n] of nx.single_source_dijkstra_path_length, columns = sorted labels, inf = no path."""
    labels = sorted(G.nodes)
    row_of = {v: i for i, v in enumerate(labels)}
    out = np.full((len(sources), len(labels)), np.inf)
    for b, s in enumerate(sources):
        for v, d in nx.single_source_dijkstra_path_length(G, s, weight=weight).items():
            out[b, row_of[v]] = d
    return out
