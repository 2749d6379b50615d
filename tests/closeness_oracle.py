"""
numpy restatement of the per-target distance sums behind networkx 3.4.2's closeness_centrality
(closeness.py:107-137) and harmonic_centrality (harmonic.py:68-89) on CSR arrays, for the tests where networkx itself
is too slow (a 1 M-node graph is not held as a networkx object).  Level-synchronous BFS over CSR arrays, 64 sources
at a time in the bits of one uint64 per node, vectorised per level; one source at a time for closeness(G, u).
No reference code.

Exactness: reach and dsum are integer sums.  The harmonic sum is formed exactly in Python integers,
sum over levels l of c_l * int(fl(1 / l) * 2^84) -- fl(1 / l) is a whole multiple of 2^-84 for l < 2^31 -- and
rounded once by ``float(Fraction(total, 2**84))``: the correctly rounded sum of the fp64 terms 1 / d.
"""
import math
from fractions import Fraction

import networkx as nx
import numpy as np

from tests.betweenness_oracle import _out_arcs, csr_of  # noqa: F401  (csr_of re-exported)

HARM_SHIFT = 84

#: networkx adds the terms 1 / d one after another in its own order; the exact sum differs from that by at most a
#: few ulps of the short sums of the tested graphs
HARMONIC_RTOL = 1e-12


def q(level: int) -> int:
    """fl(1 / level) * 2^84 as an exact integer."""
    num, den = (1.0 / level).as_integer_ratio()
    scaled = Fraction(num, den) * 2 ** HARM_SHIFT
    assert scaled.denominator == 1
    return int(scaled)


def bfs_levels(row_ptr, col, s):
    """Distances from row s along (row_ptr, col): int64[n], -1 = not reached."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n = len(row_ptr) - 1
    D = np.full(n, -1, dtype=np.int64)
    D[s] = 0
    frontier = np.array([s], dtype=np.int64)
    level = 0
    while len(frontier):
        _, head = _out_arcs(row_ptr, col, frontier)
        head = np.unique(head[D[head] < 0])
        level += 1
        D[head] = level
        frontier = head
    return D


def transpose(row_ptr, col):
    """(row_ptr, col) of the transposed CSR."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n = len(row_ptr) - 1
    tail = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    order = np.argsort(col, kind='stable')
    t_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(col, minlength=n), out=t_ptr[1:])
    return t_ptr, tail[order]


def level_counts(row_ptr, col, sources, in_adjacency=None):
    """Per-level reach counts of the BFS from `sources` (row ids, repeats count again) walking (row_ptr, col) from
    each source: a list over levels l = 1, 2, ... of int64[n] (how many sources reach v at distance l).  64 sources at
    a time, level-synchronous: each node ORs its in-neighbours' frontier bits (in_adjacency: the transposed CSR, when
    the caller has it)."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n = len(row_ptr) - 1
    t_ptr, t_col = transpose(row_ptr, col) if in_adjacency is None else in_adjacency
    starts = t_ptr[:-1]
    nonempty = np.nonzero(np.diff(t_ptr) > 0)[0]
    sources = np.asarray(list(sources), dtype=np.int64)
    counts = []
    for first in range(0, len(sources), 64):
        chunk = sources[first:first + 64]
        bits = np.left_shift(np.uint64(1), np.arange(len(chunk), dtype=np.uint64))
        frontier = np.zeros(n, dtype=np.uint64)
        np.bitwise_or.at(frontier, chunk, bits)
        visited = frontier.copy()
        level = 0
        while frontier.any():
            nxt = np.zeros(n, dtype=np.uint64)
            if len(nonempty):
                nxt[nonempty] = np.bitwise_or.reduceat(frontier[t_col], starts[nonempty])
            frontier = nxt & ~visited
            visited |= frontier
            level += 1
            c = np.bitwise_count(frontier).astype(np.int64)
            if level > len(counts):
                counts.append(np.zeros(n, dtype=np.int64))
            counts[level - 1] += c
    while counts and not counts[-1].any():
        counts.pop()
    return counts


def distance_sums(row_ptr, col, sources, in_adjacency=None, targets=None):
    """(reach int64[n], dsum int64[n], harm: list of exact integers sum_l c_l q(l)) of level_counts; with `targets`
    (row ids) harm is formed for those rows only (0 elsewhere)."""
    n = len(row_ptr) - 1
    counts = level_counts(row_ptr, col, sources, in_adjacency)
    reach = np.zeros(n, dtype=np.int64)
    dsum = np.zeros(n, dtype=np.int64)
    harm = [0] * n
    for l, c in enumerate(counts, start=1):
        reach += c
        dsum += l * c
        ql = q(l)
        rows = np.nonzero(c)[0] if targets is None else np.asarray(targets, dtype=np.int64)
        for v in rows.tolist():
            harm[v] += int(c[v]) * ql
    return reach, dsum, harm


def harm_to_float(total: int) -> float:
    return float(Fraction(total, 2 ** HARM_SHIFT))


def closeness_from_sums(reach, dsum, n, wf_improved=True):
    """networkx's formula from len(sp) - 1 = reach and totsp = dsum, in Python floats."""
    out = []
    for r, t in zip(np.asarray(reach).tolist(), np.asarray(dsum).tolist()):
        c = 0.0
        if t > 0 and n > 1:
            c = ((r + 1) - 1.0) / t
            if wf_improved:
                c *= ((r + 1) - 1.0) / (n - 1)
        out.append(c)
    return out


def _reversed_csr(G, nodelist):
    H = G.reverse(copy=False) if G.is_directed() else G
    return csr_of(H, nodelist)


def closeness(G, wf_improved=True):
    """label -> nx.closeness_centrality(G, wf_improved=wf_improved): every node a source along the out-arcs."""
    nodelist = list(G)
    row_ptr, col = csr_of(G, nodelist)
    reach, dsum, _ = distance_sums(row_ptr, col, range(len(nodelist)))
    return dict(zip(nodelist, closeness_from_sums(reach, dsum, len(nodelist), wf_improved)))


def closeness_of(G, u, wf_improved=True):
    """nx.closeness_centrality(G, u): one BFS from u along the reversed arcs."""
    nodelist = list(G)
    row_ptr, col = _reversed_csr(G, nodelist)
    D = bfs_levels(row_ptr, col, nodelist.index(u))
    r, t = int((D > 0).sum()), int(D[D > 0].sum())
    return closeness_from_sums([r], [t], len(nodelist), wf_improved)[0]


def harmonic(G, sources=None):
    """label -> the correctly rounded sum of 1 / d(v, u) over the sources v (default: every node)."""
    nodelist = list(G)
    row_of = {v: i for i, v in enumerate(nodelist)}
    row_ptr, col = csr_of(G, nodelist)
    src = range(len(nodelist)) if sources is None else [row_of[v] for v in dict.fromkeys(sources) if v in row_of]
    _, _, harm = distance_sums(row_ptr, col, src)
    return {v: harm_to_float(h) for v, h in zip(nodelist, harm)}


def harmonic_fsum(G, sources=None):
    """label -> math.fsum of 1 / d over nx.shortest_path_length: the correctly rounded sum, from networkx's BFS."""
    nodes = list(G) if sources is None else list(dict.fromkeys(v for v in sources if v in G))
    terms = {v: [] for v in G}
    for s in nodes:
        for v, d in nx.single_source_shortest_path_length(G, s).items():
            if d > 0:
                terms[v].append(1 / d)
    return {v: math.fsum(t) for v, t in terms.items()}
