"""
Graphs large enough to take every capped grid-stride launch through a second trip, with an exact expected answer.

Most launches of graphrole_amd/csrc are sized by grx_grid(items, per_block, cap) and loop ``for (i = first; i < items;
i += gridDim.x * per_block)``: the second trip of that loop exists only above cap * per_block items -- half a million
rows for most of them -- where the plain Python oracles of this directory cannot run in seconds.  So the test graph is C
copies of one small motif, INTERLEAVED: row j of copy c gets the label j * C + c.

* The map is monotone inside a copy: every row of the big CSR is row j of the motif with its neighbours in the same
  relative order, so the arc order, the id-based orientation and the hub membership carry over, and the expected output
  is the motif's oracle output, tiled: node arrays ``tile_nodes`` (np.repeat(x0, C)), per-arc arrays through the arc map
  ``tile`` returns, parent ids ``tile_ids`` (p * C + c).
* Consecutive labels belong to different copies: every adjacency list spans the whole label range and crosses every
  trip boundary.
* A traversal from the source j * C + c stays in copy c: the rows of the other copies are unreached.  ``tiled_*`` below
  build the expected per-target sums copy by copy from a solver on the motif -- an oracle, or the kernel itself on the
  motif alone -- with that copy's sources in caller order.

tests/test_tiled_graphs_cpu.py proves these constructions against the oracles themselves at C = 3 and C = 5;
tests/test_gpu_second_trip.py uses them at the sizes that wrap.  The other second-trip tests of the suite are
measures_oracle.GRAPHS['rows32' | 'rows4' | 'elements'], test_second_trip_of_the_grid_stride_loops in
test_gpu_clustering.py and test_gpu_structural_holes.py, aggx_oracle.LENGTHS and the full-size tests.
"""
import functools
from collections import namedtuple

import networkx as nx
import numpy as np

from tests import eccentricity_oracle as eo
from tests import neighbor_sense_oracle as nso
from tests import similarity_oracle as sim
from tests import sssp_oracle as so
from tests import weighted_betweenness_oracle as wo

#: rows = the sorted labels 0 .. n - 1; (row_ptr, col, w) is the out-adjacency = the in-adjacency of an undirected motif;
#: a directed one also has `inn`, the (row_ptr, col, w) of its in-adjacency (what a walk along the out-arcs pulls over)
Motif = namedtuple('Motif', 'G n row_ptr col w inn')

STAR_ARMS = 150             # above HUB_FACTOR * 4 lanes: the centre is a hub row of every motif (all have < 12 arcs a row)
DIRECTED_ARMS = 220         # three in four survive in each direction: hub rows in the out- and in the in-adjacency
LONG_ARMS = (1100, 1030)    # above NS_LONG_ROW = 1024: the rows grx_neighbor_roles walks with a whole workgroup


# ------------------------------------------------------------------------------------------------------- the tiling
def tile(row_ptr, col, C, values=None):
    """(n, row_ptr, col, values, arc_src) of C interleaved copies of the CSR (row_ptr, col[, values]): row j * C + c is
    row j of copy c.  arc_src int64[nnz]: the motif arc every arc of the tiling is a copy of, so a per-arc array x0 of
    the motif tiles to x0[arc_src]."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)[:row_ptr[-1]]
    n0, C = len(row_ptr) - 1, int(C)
    n = n0 * C
    deg = np.repeat(np.diff(row_ptr), C)
    big_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=big_ptr[1:])
    rows = np.repeat(np.arange(n, dtype=np.int64), deg)
    arc_src = row_ptr[rows // C] + (np.arange(len(rows), dtype=np.int64) - big_ptr[rows])
    big_col = col[arc_src] * C + rows % C
    return n, big_ptr, big_col, None if values is None else np.asarray(values)[arc_src], arc_src


def copies_for(n0, threshold):
    """The smallest C with n0 * C > threshold."""
    return int(threshold) // int(n0) + 1


def tile_nodes(x0, C):
    """A per-node array of the motif (nodes on the last axis) for the tiling."""
    return np.repeat(np.asarray(x0), C, axis=-1)


def tile_ids(p0, C):
    """A per-node array of motif row ids (parents, labels named by a row) for the tiling: p * C + c, negatives kept."""
    p0 = np.asarray(p0)
    big = np.repeat(p0.astype(np.int64), C) * C + np.tile(np.arange(C, dtype=np.int64), len(p0))
    return np.where(np.repeat(p0, C) < 0, np.repeat(p0, C), big).astype(p0.dtype)


def spread_sources(n0, C, count, seed=0):
    """`count` source labels j * C + c in a shuffled order: motif rows j drawn at random (one of them twice) in the first
    copy, a middle copy and the last copy, the largest label among them."""
    rng = np.random.default_rng(seed)
    j = rng.integers(0, n0, size=count)
    j[-1] = j[0]
    c = np.array([0, C // 2, C - 1])[np.arange(count) % 3]
    j[1], c[1] = n0 - 1, C - 1                                  # the last row of the tiling
    c[-1] = c[0]                                                # the repeat: the same label twice
    return j * C + c


# ------------------------------------------------------------------------------------------------------- the motifs
def _pieces(star_arms):
    """The structural motif on the nodes 0 .. n - 1 in construction order: K7, a wheel, a 5 x 5 grid, a path, a pendant
    tree and a star, joined by a few bridges, and two isolated rows."""
    G = nx.complete_graph(7)                                                            # 0 .. 6
    G = nx.disjoint_union(G, nx.wheel_graph(9))                                         # 7 (hub) .. 15
    G = nx.disjoint_union(G, nx.convert_node_labels_to_integers(nx.grid_2d_graph(5, 5)))   # 16 .. 40
    G = nx.disjoint_union(G, nx.path_graph(20))                                         # 41 .. 60
    G = nx.disjoint_union(G, nx.random_labeled_tree(12, seed=4))                        # 61 .. 72
    G = nx.disjoint_union(G, nx.star_graph(star_arms))                                  # 73 (centre) ..
    G.add_edges_from([(3, 9), (12, 16), (40, 41), (28, 61), (73, 20)])                  # the bridges
    last = G.number_of_nodes()
    G.add_nodes_from([last, last + 1])                                                  # isolated
    return G


def _square_pieces(G):
    """Rows in each wedge tier of grx_square_clustering, all on squares: 56 centres with 56 leaves each; two rows joined
    to every centre (3 000 + wedges: dense tier), one joined to 30 of them (1 700: LDS tier); and K(2, 40)."""
    first = G.number_of_nodes()
    centres = list(range(first, first + 56))
    G.add_nodes_from(centres)
    at = first + 56
    for c in centres:
        G.add_edges_from((c, at + t) for t in range(56))
        at += 56
    G.add_edges_from((at, c) for c in centres)
    G.add_edges_from((at + 1, c) for c in centres)
    G.add_edges_from((at + 2, c) for c in centres[:30])
    G.add_edge(at + 2, 0)
    at += 3
    G.add_edges_from((s, at + 2 + t) for s in (at, at + 1) for t in range(40))
    G.add_edge(at, 5)
    return G


def _shuffled(G, seed, pin=()):
    """G with its n nodes relabelled 0 .. n - 1 by a seeded permutation; pin: (node, label) pairs that hold after it."""
    n = G.number_of_nodes()
    assert sorted(G) == list(range(n))
    perm = np.random.default_rng(seed).permutation(n)
    for node, label in pin:
        other = int(np.nonzero(perm == label)[0][0])
        perm[other], perm[node] = perm[node], label
    return nx.relabel_nodes(G, {v: int(perm[v]) for v in G})


def _weighted(G, kind, seed):
    """G with the weights of `kind`, and the two hand-made weighted pieces of the oracle modules behind it: the detour
    (the lightest path has more hops than the direct arc) and the uneven ties (two lightest paths of different lengths)."""
    H = wo.with_weights(G, kind, seed)
    for piece, bridge in ((so.detour_graph(), 2), (wo.uneven_ties_graph(), 30)):
        first = H.number_of_nodes()
        H = nx.disjoint_union(H, piece)
        H.add_edge(bridge, first, weight=2.0)
    return H


def _directed(G, seed):
    """A digraph on G's nodes: each edge keeps both of its arcs, or only one of them, with weights of their own."""
    rng = np.random.default_rng(seed)
    D = nx.DiGraph()
    D.add_nodes_from(G)
    for u, v in G.edges():
        which = rng.integers(0, 4)
        if which != 0:
            D.add_edge(u, v, weight=float(rng.uniform(0.05, 1.0)))
        if which != 1:
            D.add_edge(v, u, weight=float(rng.uniform(0.05, 1.0)))
    return D


@functools.lru_cache(maxsize=None)
def motif(kind):
    """'structural'; 'squares' (with rows in every wedge tier); 'long_stars' (two rows above NS_LONG_ROW arcs, at the
    first and at the last label, weighted); the symmetric weights 'ints', 'dyadic' and 'uniform'; 'directed'."""
    pin = ()
    if kind == 'structural':
        G = _pieces(STAR_ARMS)
    elif kind == 'squares':
        G = _square_pieces(_pieces(STAR_ARMS))
    elif kind == 'long_stars':
        G = _pieces(LONG_ARMS[0])
        first = G.number_of_nodes()
        G = nx.disjoint_union(G, nx.star_graph(LONG_ARMS[1]))
        G.add_edge(first, 5)
        pin = ((73, 0), (first, G.number_of_nodes() - 1))
        G = wo.with_weights(G, 'uniform', 3)
    elif kind in ('ints', 'dyadic', 'uniform'):
        G = _weighted(_pieces(STAR_ARMS), kind, 11)
    elif kind == 'directed':
        G = _directed(_weighted(_pieces(DIRECTED_ARMS), 'uniform', 12), 13)
    else:
        raise KeyError(kind)
    G = _shuffled(G, 17, pin)
    weighted = kind not in ('structural', 'squares')
    labels, row_ptr, col, w = so.pulled_csr(G, 'weight' if weighted else None)
    assert labels == list(range(len(labels)))
    inn = None
    if G.is_directed():
        inn = (row_ptr, col, w)
        _, row_ptr, col, w = so.pulled_csr(G.reverse(copy=True), 'weight')
    return Motif(G, len(labels), row_ptr, col, w if weighted else None, inn)


# ----------------------------------------------------------------------- expected values of a traversal on a tiling
def _by_copy(sources, C):
    """(motif rows, copies, [(copy, positions in `sources` of its sources, in caller order)])."""
    sources = np.asarray(sources, dtype=np.int64)
    j, c = sources // C, sources % C
    return j, c, [(int(k), np.nonzero(c == k)[0]) for k in np.unique(c)]


def tiled_weighted_distances(solve, n0, C, sources):
    """grx_weighted_distances of `sources` (labels of the tiling) from ``solve(motif rows)`` = the same seven outputs on
    the motif: source_ecc, the distance rows and the rounds from the whole list (every batch holds the same lanes), the
    per-target sums and extremes copy by copy from that copy's sources in caller order; a row of another copy is at
    inf and adds nothing."""
    j, c, groups = _by_copy(sources, C)
    n = n0 * C
    whole = solve(j)
    reach = np.zeros(n, dtype=np.int64)
    dsum, harmonic, far = np.zeros(n), np.zeros(n), np.zeros(n)
    for k, at in groups:
        part = solve(j[at])
        reach[k::C], dsum[k::C], harmonic[k::C], far[k::C] = part[0][:n0], part[1][:n0], part[2][:n0], part[3][:n0]
    dist = None
    if whole[5] is not None:
        dist = np.full((len(j), n), np.inf)
        for b in range(len(j)):
            dist[b, c[b]::C] = whole[5][b]
    return reach, dsum, harmonic, far, whole[4], dist, whole[6]


def tiled_betweenness(solve, n0, C, sources):
    """grx_weighted_betweenness of `sources` from ``solve(motif rows)`` = (bc, rounds, levels) on the motif: bc copy by
    copy from that copy's sources in caller order, rounds and levels from the whole list."""
    j, _, groups = _by_copy(sources, C)
    bc = np.zeros(n0 * C)
    for k, at in groups:
        bc[k::C] = solve(j[at])[0][:n0]
    _, rounds, levels = solve(j)
    return bc, rounds, levels


def tiled_eccentricity(solve, n0, C, sources, lower=None, upper=None, want_upper=False):
    """One grx_eccentricity call on the tiling from ``solve(motif rows, lower, upper)`` = (source_ecc, reach, lower,
    upper) of one call on the motif; lower / upper: the bounds of the tiling carried in (None: the call initialises
    them, upper only with want_upper).  A copy without a source keeps its bounds and reaches nothing."""
    j, _, groups = _by_copy(sources, C)
    n = n0 * C
    carried = lower is not None
    if not carried:
        lower = np.zeros(n, dtype=np.int32)
        upper = np.full(n, eo.INF, dtype=np.int32) if want_upper else None
    else:
        lower = np.array(lower, dtype=np.int32)
        upper = None if upper is None else np.array(upper, dtype=np.int32)
    source_ecc = np.zeros(len(j), dtype=np.int32)
    reach = np.zeros(n, dtype=np.int64)
    for k, at in groups:
        part = solve(j[at], lower[k::C].copy() if carried else None,
                     upper[k::C].copy() if carried and upper is not None else None)
        source_ecc[at] = part[0]
        reach[k::C], lower[k::C] = part[1][:n0], part[2][:n0]
        if upper is not None:
            upper[k::C] = part[3][:n0]
    return source_ecc, reach, lower, upper


# -------------------------------------------------------- the oracles that loop over rows or queries, for a large input
def neighbor_roles(row_ptr, col, w, P, mode='mean'):
    """neighbor_sense_oracle.neighbor_roles with the rows of one length summed together: the same ``_slot_sum`` over the
    same terms in the same order for every row, so the same bits, without a Python loop over the rows."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    P = np.asarray(P, dtype=np.float64)
    n, r = len(row_ptr) - 1, P.shape[1]
    deg = np.diff(row_ptr)
    out = np.zeros((r, n))
    for d in np.unique(deg[deg > 0]).tolist():
        rows = np.nonzero(deg == d)[0]
        slots = nso.SLOTS if d <= nso.LONG_ROW else nso.LONG_SLOTS
        for first in range(0, len(rows), max(1, (1 << 22) // (d * r))):
            some = rows[first:first + max(1, (1 << 22) // (d * r))]
            arcs = row_ptr[some][None, :] + np.arange(d, dtype=np.int64)[:, None]       # [d, rows]
            terms = P[col[arcs]]                                                        # [d, rows, r]
            if w is None:
                total, den = nso._slot_sum(terms, slots), np.full(len(some), float(d))
            else:
                wi = np.asarray(w, dtype=np.float64)[arcs]
                total, den = nso._slot_sum(wi[:, :, None] * terms, slots), nso._slot_sum(wi, slots)
            if mode == 'mean':
                with np.errstate(divide='ignore', invalid='ignore'):
                    total = np.where((den != 0.0)[:, None], total / den[:, None], 0.0)
            out[:, some] = total.T
    return out


def similar_rows_many_queries(X, Q, k, metric):
    """similarity_oracle.similar_rows(X, Q, None, k, metric) for many queries and few candidates: its keys and its
    scores, the order (key, then the smaller row) by one stable sort instead of a lexsort per query."""
    key = sim.keys(Q, X, metric)
    nq, n = key.shape
    order = np.argsort(key, axis=1, kind='stable')[:, :k]
    index = np.full((nq, k), -1, dtype=np.int32)
    index[:, :order.shape[1]] = order
    score = np.full((nq, k), np.nan)
    score[:, :order.shape[1]] = sim.score_of(np.take_along_axis(key, order, axis=1), metric)
    return index, score
