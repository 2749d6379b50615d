"""
Two independent host implementations of the triad census of a directed graph (Holland and Leinhardt's 16 isomorphism
classes of three nodes with their arcs, in the order of networkx's TRIAD_NAMES).

``brute_census(G, v=None)`` is the definition: every 3-subset (with v: every one that holds v), classified by the arcs
present.  ``census(row_ptr, col, codes)`` is the numpy restatement of csrc/grx_triads.hip on the arrays the kernel
reads -- the structurally symmetric all-neighbours CSR without diagonal and one direction code per arc slot (u, v):
1 = only u -> v, 2 = only v -> u, 3 = both -- with the same intermediate quantities: the neighbour classes (o, i, m),
common(u, v) per arc, the closed triads by type per node, the non-induced wedges and the back-substitution matrix.
"""
import itertools
from collections import namedtuple

import networkx as nx
import numpy as np
from networkx.algorithms.triads import TRIAD_NAMES, TRICODES

NAMES = tuple(TRIAD_NAMES)
COLUMNS = [f'triad_{name}' for name in NAMES]
T = {name: k for k, name in enumerate(NAMES)}
#: the type of the triad (a, b, c) with the 6-bit code c(a, b) | c(a, c) << 2 | c(b, c) << 4, where bit 0 of c(x, y) is
#: the arc x -> y and bit 1 the arc y -> x: networkx's own table
TYPE_OF_CODE = np.array(TRICODES, dtype=np.int64) - 1
WEDGES = ('021D', '021U', '021C', '111D', '111U', '201')        # the six open connected types
CLOSED = ('030T', '030C', '120D', '120U', '120C', '210', '300')  # the seven closed ones
#: the type of the wedge whose centre sees its two ends in the classes (x, z); O, I, M = 1, 2, 3 = the direction code of
#: the slot (centre, end)
WEDGE_OF = {(1, 1): '021D', (2, 2): '021U', (1, 2): '021C', (2, 1): '021C', (3, 2): '111D', (2, 3): '111D',
            (3, 1): '111U', (1, 3): '111U', (3, 3): '201'}
#: row = closed type, column = wedge type: how many of the three wedges left by dropping one pair of the closed triad
#: are of that type
MATRIX = np.array([
    [1, 1, 1, 0, 0, 0],          # 030T
    [0, 0, 3, 0, 0, 0],          # 030C
    [1, 0, 0, 2, 0, 0],          # 120D
    [0, 1, 0, 0, 2, 0],          # 120U
    [0, 0, 1, 1, 1, 0],          # 120C
    [0, 0, 0, 1, 1, 1],          # 210
    [0, 0, 0, 0, 0, 3],          # 300
], dtype=np.int64)

Census = namedtuple('Census', 'columns totals common wedges closed matrix')


def pair_code(G, a, b):
    return (1 if G.has_edge(a, b) else 0) | (2 if G.has_edge(b, a) else 0)


def brute_census(G, v=None):
    """{name: count} over all 3-subsets of G's nodes, or over those that hold v."""
    out = dict.fromkeys(NAMES, 0)
    nodes = list(G)
    if v is None:
        triples = itertools.combinations(nodes, 3)
    else:
        triples = ((v, a, b) for a, b in itertools.combinations([x for x in nodes if x != v], 2))
    for a, b, c in triples:
        code = pair_code(G, a, b) | pair_code(G, a, c) << 2 | pair_code(G, b, c) << 4
        out[NAMES[TYPE_OF_CODE[code]]] += 1
    return out


def brute_columns(G, nodes=None):
    """int64[16, n]: brute_census(G, v) for every v (rows in the order of `nodes`, default sorted) from one pass over
    all 3-subsets, as arrays."""
    nodes = sorted(G) if nodes is None else list(nodes)
    n = len(nodes)
    A = nx.to_numpy_array(G, nodelist=nodes, weight=None, dtype=np.int64) if n else np.zeros((0, 0), dtype=np.int64)
    c = (A != 0) + 2 * (A.T != 0)
    out = np.zeros((16, n), dtype=np.int64)
    if n < 3:
        return out
    a, b, d = (np.array(x, dtype=np.int64) for x in zip(*itertools.combinations(range(n), 3)))
    t = TYPE_OF_CODE[c[a, b] | c[a, d] << 2 | c[b, d] << 4]
    for node in (a, b, d):
        np.add.at(out, (t, node), 1)
    return out


def graph_arrays(G, nodes=None):
    """(nodes, row_ptr int64, col int32, codes uint8) of a DiGraph without self-loops: rows in the order of `nodes`
    (default sorted)."""
    nodes = sorted(G) if nodes is None else list(nodes)
    at = {v: k for k, v in enumerate(nodes)}
    rows = [[] for _ in nodes]
    for u, v in G.edges():
        assert u != v
        rows[at[u]].append(at[v])
        rows[at[v]].append(at[u])
    row_ptr = np.zeros(len(nodes) + 1, dtype=np.int64)
    col, codes = [], []
    for k, r in enumerate(rows):
        r = sorted(set(r))
        row_ptr[k + 1] = row_ptr[k] + len(r)
        col.extend(r)
        codes.extend(pair_code(G, nodes[k], nodes[x]) for x in r)
    return nodes, row_ptr, np.array(col, dtype=np.int32), np.array(codes, dtype=np.uint8)


def _comb2(x):
    return x * (x - 1) // 2


def census(row_ptr, col, codes):
    """The kernel's method on its own arrays: Census(columns int64[16, n], totals int64[16], common int32[nnz], wedges
    int64[6, n] = the non-induced wedge counts, closed int64[7, n], matrix)."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n = len(row_ptr) - 1
    nnz = int(row_ptr[-1])
    col = np.asarray(col, dtype=np.int64)[:nnz]
    codes = np.asarray(codes, dtype=np.int64)[:nnz]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    # (a) the classes of every row's neighbours
    cnt = np.zeros((4, n), dtype=np.int64)
    np.add.at(cnt, (codes, rows), 1)
    o, i, m = cnt[1], cnt[2], cnt[3]
    d = o + i + m
    pairs_a, pairs_m = int((o + i).sum()) // 2, int(m.sum()) // 2
    # (b) one intersection per adjacent pair
    key = rows * max(n, 1) + col
    common = np.zeros(nnz, dtype=np.int32)
    closed = np.zeros((16, n), dtype=np.int64)
    opp = np.zeros((2, n), dtype=np.int64)                      # closed triads by the class of the opposite pair
    deg = np.diff(row_ptr)
    slot = np.nonzero(rows < col)[0]                            # the pairs, at their slot (u, v) with u < v
    pu, pv = rows[slot], col[slot]
    walk_u = deg[pu] <= deg[pv]
    walked, searched = np.where(walk_u, pu, pv), np.where(walk_u, pv, pu)
    pair = np.repeat(np.arange(len(slot), dtype=np.int64), deg[walked])
    first = np.cumsum(deg[walked]) - deg[walked]
    k = row_ptr[walked][pair] + np.arange(len(pair), dtype=np.int64) - first[pair]      # the walked rows, every entry
    w = col[k]
    lo = np.minimum(np.searchsorted(key, searched[pair] * max(n, 1) + w), max(nnz - 1, 0))
    hit = key[lo] == searched[pair] * max(n, 1) + w if nnz else np.zeros(0, dtype=bool)
    pair, k, lo, w = pair[hit], k[hit], lo[hit], w[hit]
    per_pair = np.bincount(pair, minlength=len(slot)).astype(np.int32)
    common[slot] = per_pair
    common[np.searchsorted(key, pv * max(n, 1) + pu)] = per_pair
    once = w > pv[pair]                                         # the closed triad u < v < w
    pair, k, lo, w = pair[once], k[once], lo[once], w[once]
    u, v = pu[pair], pv[pair]
    cuv = codes[slot][pair]
    cuw, cvw = np.where(walk_u[pair], codes[k], codes[lo]), np.where(walk_u[pair], codes[lo], codes[k])
    t = TYPE_OF_CODE[cuv | cuw << 2 | cvw << 4]
    for node, opposite in ((u, cvw), (v, cuw), (w, cuv)):
        np.add.at(closed, (t, node), 1)
        np.add.at(opp, ((opposite == 3).astype(np.int64), node), 1)
    # (c) per row y over its entries u; x = the class of y as seen from u = the mirror of the slot's code
    x = np.where(codes == 3, 3, 3 - codes)
    S = np.zeros((4, 4, n), dtype=np.int64)                     # S[x][z][y] = sum of cnt_z(u), u seeing y as x
    for z in (1, 2, 3):
        np.add.at(S, (x, z, rows), cnt[z][col])
    C = np.zeros((2, n), dtype=np.int64)                        # common(y, u) over the asymmetric / mutual pairs at y
    np.add.at(C, ((codes == 3).astype(np.int64), rows), common.astype(np.int64))
    # finish
    seen_as = {1: i, 2: o, 3: m}                                # how many neighbours see y as O, I, M
    centre = {'021D': _comb2(o), '021U': _comb2(i), '021C': o * i, '111D': m * i, '111U': m * o, '201': _comb2(m)}
    wedges = np.zeros((6, n), dtype=np.int64)
    for k, name in enumerate(WEDGES):
        wedges[k] = centre[name]
    for (xc, z), name in WEDGE_OF.items():
        wedges[WEDGES.index(name)] += S[xc, z] - (seen_as[xc] if xc == z else 0)
    closed7 = np.stack([closed[T[name]] for name in CLOSED])
    columns = np.zeros((16, n), dtype=np.int64)
    for k, name in enumerate(CLOSED):
        columns[T[name]] = closed7[k]
    for k, name in enumerate(WEDGES):
        columns[T[name]] = wedges[k] - MATRIX[:, k] @ closed7
    n_a, n_m = o + i, m
    D_a, D_m = S[1].sum(axis=0) + S[2].sum(axis=0), S[3].sum(axis=0)
    deg_a, deg_m = S[:, 1].sum(axis=0) + S[:, 2].sum(axis=0), S[:, 3].sum(axis=0)
    columns[T['012']] = n_a * (n - d) - D_a + C[0] + pairs_a - deg_a + opp[0]
    columns[T['102']] = n_m * (n - d) - D_m + C[1] + pairs_m - deg_m + opp[1]
    columns[T['003']] = _comb2(n - 1) - columns[1:].sum(axis=0) if n else 0
    totals = columns.sum(axis=1)
    assert not np.any(totals % 3)
    return Census(columns, totals // 3, common, wedges, closed7, MATRIX)


def graph_census(G, nodes=None):
    """(nodes, Census) of a DiGraph by the formulas."""
    nodes, row_ptr, col, codes = graph_arrays(G, nodes)
    return nodes, census(row_ptr, col, codes)


def tiled_motif(C):
    """The directed motif of tests/tiled_graphs.py for the triad kernel: ((row_ptr, col, codes) of the motif -- its
    all-neighbours CSR and the code of every slot --, C, (n, row_ptr, col, codes, arc_src) of C interleaved copies).
    The tiling is monotone inside a copy, so the code of a slot and the mirror at its reverse carry over, and the
    connected and closed columns and common(u, v) of the tiling are the motif's own, tiled; the null and dyadic columns
    are not (they count the nodes and the pairs of the whole graph)."""
    from tests import tiled_graphs as tg
    D = nx.DiGraph(tg.motif('directed').G)
    D.remove_edges_from(list(nx.selfloop_edges(D)))
    nodes, row_ptr, col, codes = graph_arrays(D)
    assert nodes == list(range(len(nodes)))
    n, big_ptr, big_col, big_codes, arc_src = tg.tile(row_ptr, col, C, codes)
    return (row_ptr, col, codes), int(C), (n, big_ptr, big_col.astype(np.int32), big_codes, arc_src)


def as_dict(values):
    return {name: int(x) for name, x in zip(NAMES, values)}


def all_digraphs(k):
    """Every digraph on the labelled nodes 0 .. k - 1 without self-loops, by the bits of its arc mask."""
    arcs = [(a, b) for a in range(k) for b in range(k) if a != b]
    for mask in range(1 << len(arcs)):
        G = nx.DiGraph()
        G.add_nodes_from(range(k))
        G.add_edges_from(arc for bit, arc in enumerate(arcs) if mask >> bit & 1)
        yield G
