"""
The small-graph atlas the measure tests share: the disjoint union of all 1252 non-null graphs on 1-7 nodes
(networkx's Atlas of Graphs) from the committed fixture tests/golden/atlas_union.npz (tools/make_golden_atlas.py) --
8475 nodes, 12342 edges, 1610 components, 296 isolated nodes, maximum degree 6 -- as networkx graphs under two
relabellings of the node ids:

    'identity'  atlas node i keeps the id i: every component is contiguous in id space
    'perm'      atlas node i gets the id perm[i] (seeded): the components are interleaved

and in three variants: 'undirected', 'directed' (every edge u -> v, v -> u or both, seeded) and 'weighted' (undirected,
integer weights 1 .. 3, seeded).  ``cone`` adds one apex joined to every node.  Nothing here reads networkx's own atlas
file: the GPU tests run from the fixture alone (tests/test_atlas_cpu.py compares it with ``nx.graph_atlas_g()``).

Arrays "in atlas order" have one entry per atlas node i; ``by_label`` turns one into the Series the public functions of
graphrole_amd return (index = the sorted labels), ``atlas_order`` maps such a Series back.
"""
import functools
import os

import networkx as nx
import numpy as np
import pandas as pd

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'atlas_union.npz')
RELABELLINGS = ('identity', 'perm')
VARIANTS = ('undirected', 'directed', 'weighted')
FORWARD, BACKWARD, BOTH = 0, 1, 2                              # the orientation codes of the fixture
#: the slow networkx columns the fixture stores, each in atlas order
STORED = ('betweenness', 'betweenness_endpoints', 'betweenness_directed', 'betweenness_weighted', 'constraint',
          'constraint_weighted', 'effective_size', 'effective_size_weighted')


@functools.lru_cache(maxsize=None)
def load():
    """The fixture's arrays as a dict (read once; do not write into them)."""
    with np.load(FIXTURE) as z:
        data = {k: z[k] for k in z.files}
    for a in data.values():
        a.setflags(write=False)
    return data


def n_nodes() -> int:
    return len(load()['atlas_id'])


def relabelling(relabel: str) -> np.ndarray:
    """label[i] of atlas node i."""
    assert relabel in RELABELLINGS, relabel
    return np.arange(n_nodes(), dtype=np.int64) if relabel == 'identity' else load()['perm'].astype(np.int64)


def arcs(variant: str):
    """(src, dst, weight or None) in atlas node ids: the edges as stored, or for 'directed' the arcs of the seeded
    orientation (an edge with code BOTH gives two)."""
    f = load()
    src, dst = f['src'].astype(np.int64), f['dst'].astype(np.int64)
    if variant == 'undirected':
        return src, dst, None
    if variant == 'weighted':
        return src, dst, f['weight'].astype(np.int64)
    assert variant == 'directed', variant
    fwd, bwd = f['orient'] != BACKWARD, f['orient'] != FORWARD
    return np.concatenate([src[fwd], dst[bwd]]), np.concatenate([dst[fwd], src[bwd]]), None


def _build(variant, label, n):
    G = nx.DiGraph() if variant == 'directed' else nx.Graph()
    G.add_nodes_from(label[:n].tolist())                       # atlas order: under 'perm' list(G) is not sorted
    src, dst, w = arcs(variant)
    if w is None:
        G.add_edges_from(zip(label[src].tolist(), label[dst].tolist()))
    else:
        G.add_weighted_edges_from(zip(label[src].tolist(), label[dst].tolist(), w.tolist()))
    return G


@functools.lru_cache(maxsize=None)
def graph(variant: str = 'undirected', relabel: str = 'identity'):
    """The union as a networkx graph (cached: do not change it)."""
    return _build(variant, relabelling(relabel), n_nodes())


@functools.lru_cache(maxsize=None)
def cone(relabel: str = 'identity'):
    """The undirected union plus an apex (label n) joined to every node: one hub row of n arcs over every small
    structure (cached: do not change it)."""
    G = _build('undirected', relabelling(relabel), n_nodes())
    apex = n_nodes()
    G.add_edges_from((apex, v) for v in list(G))
    return G


def apex() -> int:
    return n_nodes()


@functools.lru_cache(maxsize=None)
def bounds():
    """(first, size): the first atlas node and the number of nodes of every atlas graph, in atlas order."""
    atlas_id = load()['atlas_id']
    first = np.concatenate([[0], np.flatnonzero(np.diff(atlas_id)) + 1]).astype(np.int64)
    return first, np.diff(np.concatenate([first, [len(atlas_id)]]))


@functools.lru_cache(maxsize=None)
def small_graphs(variant: str = 'undirected'):
    """[(atlas id, first atlas node, networkx graph on the local nodes 0 .. k - 1)] of every atlas graph, rebuilt from
    the fixture (cached: do not change them)."""
    first, size = bounds()
    src, dst, w = arcs(variant)
    owner = np.searchsorted(first, src, side='right') - 1
    order = np.argsort(owner, kind='stable')
    cuts = np.searchsorted(owner[order], np.arange(len(first) + 1))
    ids = load()['atlas_id'][first]
    out = []
    for i, (lo, k) in enumerate(zip(first.tolist(), size.tolist())):
        G = nx.DiGraph() if variant == 'directed' else nx.Graph()
        G.add_nodes_from(range(k))
        e = order[cuts[i]:cuts[i + 1]]
        if w is None:
            G.add_edges_from(zip((src[e] - lo).tolist(), (dst[e] - lo).tolist()))
        else:
            G.add_weighted_edges_from(zip((src[e] - lo).tolist(), (dst[e] - lo).tolist(), w[e].tolist()))
        out.append((int(ids[i]), lo, G))
    return out


def place(values_by_atlas_graph, dtype=np.float64) -> np.ndarray:
    """Per-graph values into the union by label: `values_by_atlas_graph` has one entry per atlas graph in atlas order,
    a mapping local node -> value or a sequence over the local nodes (a value may be a vector: the result then has
    one row per node); the result is in atlas order."""
    first, size = bounds()
    assert len(values_by_atlas_graph) == len(first)
    out = None
    for lo, k, values in zip(first.tolist(), size.tolist(), values_by_atlas_graph):
        assert len(values) == k
        block = np.asarray([values[v] for v in range(k)], dtype=dtype)
        if out is None:
            out = np.empty((n_nodes(),) + block.shape[1:], dtype=dtype)
        out[lo:lo + k] = block
    return out


def by_label(column, relabel: str, name=None) -> pd.Series:
    """An array in atlas order as a Series behind the sorted labels."""
    label = relabelling(relabel)
    out = np.empty_like(np.asarray(column))
    out[label] = column
    return pd.Series(out, index=pd.Index(np.arange(len(label))), name=name)


def atlas_order(series, relabel: str) -> np.ndarray:
    """The values of a Series (or the rows of a frame) indexed by the sorted labels 0 .. n - 1, in atlas order."""
    assert np.array_equal(np.asarray(series.index), np.arange(n_nodes()))
    return series.to_numpy()[relabelling(relabel)]


def stored(name: str, relabel: str = 'identity') -> pd.Series:
    """A stored networkx column behind the sorted labels."""
    assert name in STORED, name
    return by_label(load()[name], relabel, name)


def of_dict(values: dict, index) -> np.ndarray:
    """networkx's label -> value dict as an array in the order of `index`."""
    return np.array([values[v] for v in index])
