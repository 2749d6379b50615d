"""
The graphs that tests/test_gpu_structural_holes.py and tests/test_gpu_clustering.py both run their kernels on: the
smallest shapes that reach each path of the shared row-intersection stages (csrc/grx_rowjoin.h).  Plain builders, no
fixtures; the oracles next to this file turn the pairs into the arrays of each kernel.
"""
import functools
import random

import networkx as nx
import numpy as np

WEIGHTS = {
    'unweighted': None,
    'integer': lambda a, b: 1 + (7 * a + 13 * b) % 5,
    'float': lambda a, b: 0.1 + ((31 * a + 17 * b) % 97) / 13.0,
}


def _pairs_of(G):
    return [(int(u), int(v)) for u, v in G.edges]


@functools.lru_cache(maxsize=None)
def _named_pairs(key):
    if key == 'n1':
        return 1, ()
    if key == 'n1_loop':
        return 1, ((0, 0),)
    if key == 'n2':
        return 2, ((0, 1),)
    if key == 'n3_path':
        return 3, ((0, 1), (1, 2))
    if key == 'n3_triangle':
        return 3, ((0, 1), (1, 2), (0, 2))
    graphs = {
        'path': lambda: nx.path_graph(300),
        'star1500': lambda: nx.star_graph(1500),               # a hub with no triangle
        'K70': lambda: nx.complete_graph(70),                   # 68 common neighbours per arc, rows above a wavefront
        'K40_40': lambda: nx.complete_bipartite_graph(40, 40),  # every intersection empty
        'wheel1500': lambda: nx.wheel_graph(1500),              # short rows searched against a 1 499-arc hub row
        'ba2000': lambda: nx.barabasi_albert_graph(2000, 5, seed=7),
    }
    G = graphs[key]()
    return G.number_of_nodes(), tuple(_pairs_of(G))


def _threshold_pairs(entries):
    """A centre (row 0) with `entries` neighbours that form a ring with chords: the centre's row has exactly `entries`
    entries, every other row at most 5, and every arc of the centre has common neighbours."""
    pairs = [(0, k) for k in range(1, entries + 1)]
    pairs += [(k, k % entries + 1) for k in range(1, entries + 1)]
    pairs += [(k, (k + 6) % entries + 1) for k in range(1, entries + 1, 3)]
    return entries + 1, pairs


def _digraph():
    D = nx.gnm_random_graph(40, 150, seed=4, directed=True)
    rng = random.Random(4)
    D.add_edges_from([(0, 1), (1, 0), (2, 3), (3, 2), (5, 5)])  # reciprocal pairs and a loop
    D.add_edges_from([(40, 0), (40, 7)])                        # 40: out-arcs only
    D.add_edges_from([(3, 41), (9, 41)])                        # 41: in-arcs only
    D.add_node(42)
    for u, v in D.edges:
        D[u][v]['weight'] = rng.choice([0.5, 1.0, 2.0, 7.25])
    return D


def _ba60000():
    """(n, row_ptr, col, values) of BA 60 000 / m = 5: large enough to wrap the grid-stride loops of grx_rowjoin.h."""
    from graphrole_amd import synth
    n = 60000
    src, dst = synth.ba_edges(n, 5, seed=3)
    rows, cols = np.concatenate([src, dst]), np.concatenate([dst, src])
    key = np.unique(rows.astype(np.int64) * n + cols)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // n, minlength=n), out=row_ptr[1:])
    col = (key % n).astype(np.int32)
    lo, hi = np.minimum(key // n, key % n), np.maximum(key // n, key % n)
    return n, row_ptr, col, 0.1 + ((31 * lo + 17 * hi) % 97) / 13.0         # symmetric values
