"""
Biconnected components on the MI355X: graphrole_amd.biconnected_component_counts, articulation_points and
biconnected_components equal to networkx computed here (integers and sets: exact) on every graph kind, hub rows and a
599-level path included; kernels.biconnected equal to tests/biconnected_oracle.py on the same CSR, a valid BFS forest,
the same bytes in every run and with or without the forest outputs; igraph and CSRGraph inputs; and the karate
sense-making run with the column.
"""
from collections import Counter

import networkx as nx
import numpy as np
import pytest

from tests import biconnected_oracle as bo

pytestmark = pytest.mark.gpu


def _multigraph():
    return nx.MultiGraph([(0, 1), (0, 1), (1, 2), (2, 0), (2, 3), (3, 3), (3, 4), (4, 5), (5, 3), (5, 6), (5, 6)])


def _disconnected():
    G = nx.disjoint_union(nx.barabasi_albert_graph(200, 2, seed=1), nx.cycle_graph(9))
    G.add_nodes_from([1000, 1001])
    return G


GRAPHS = {
    'karate': nx.karate_club_graph,
    'er300': lambda: nx.gnm_random_graph(300, 1200, seed=1),
    'sparse300': lambda: nx.gnm_random_graph(300, 330, seed=2),
    'tree300': lambda: nx.barabasi_albert_graph(300, 1, seed=2),
    'ba2000': lambda: nx.barabasi_albert_graph(2000, 5, seed=3),
    'star': lambda: nx.star_graph(1500),
    'barbell': lambda: nx.barbell_graph(6, 4),
    'windmill': lambda: nx.windmill_graph(5, 4),
    'cycle9': lambda: nx.cycle_graph(9),
    'grid': lambda: nx.grid_2d_graph(6, 7),
    'path600': lambda: nx.path_graph(600),
    'disconnected': _disconnected,
    'multigraph': _multigraph,
    'strings': lambda: nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
    'n1': lambda: nx.empty_graph(1),
    'n2': lambda: nx.path_graph(2),
    'n3': lambda: nx.path_graph(3),
}


def _nx_counts(G):
    c = Counter(v for comp in nx.biconnected_components(G) for v in comp)
    return {v: c.get(v, 0) for v in G}


def _frozen(components):
    return {frozenset(c) for c in components}


def _check_public(G_in, S):
    """The three public functions on G_in against networkx on the simple graph S with the same nodes."""
    from graphrole_amd import articulation_points, biconnected_component_counts, biconnected_components
    counts = biconnected_component_counts(G_in)
    assert counts.name == 'biconnected_components' and counts.dtype == np.int64
    assert list(counts.index) == sorted(S)
    assert counts.to_dict() == _nx_counts(S)
    points = articulation_points(G_in)
    assert set(points) == set(nx.articulation_points(S)) and len(points) == len(set(points))
    assert points == [v for v in counts.index if v in set(points)]          # index order
    comps = biconnected_components(G_in)
    assert len(comps) == len(_frozen(comps))
    assert _frozen(comps) == _frozen(nx.biconnected_components(S))


@pytest.mark.parametrize('key', list(GRAPHS))
def test_matches_networkx(key):
    G = GRAPHS[key]()
    _check_public(G, nx.Graph(G))


def test_hub_graphs_have_hub_rows():
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    for key in ('star', 'ba2000'):
        out = NetworkxInterface(GRAPHS[key]())._structure_csrs()[0]
        assert out.n_hubs > 0, key


def _kernel_run(G, want_forest=True):
    from graphrole_amd import kernels as K
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    s_out = NetworkxInterface(G)._structure_csrs()[0]
    n = s_out.n
    count, parent, label, n_components = K.biconnected(s_out, want_forest=want_forest)
    host = [None if t is None else K.to_host(t)[:n].copy() for t in (count, parent, label)]
    row_ptr = K.to_host(s_out.row_ptr).astype(np.int64)
    col = K.to_host(s_out.col)[:s_out.nnz].astype(np.int64)
    return host, n_components, (row_ptr, col)


@pytest.mark.parametrize('key', ['star', 'ba2000', 'sparse300', 'disconnected', 'path600'])
def test_kernel_equals_oracle_on_the_same_csr(key):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    G = GRAPHS[key]()
    (count, parent, label), n_components, (row_ptr, col) = _kernel_run(G)
    n = len(row_ptr) - 1
    assert count.dtype == np.int64 and parent.dtype == np.int32 and label.dtype == np.int32
    want = bo.biconnected(row_ptr, col)
    assert np.array_equal(count, want.count)
    assert np.array_equal(parent, want.parent)                  # the same stated parent rule
    assert n_components == want.n_components
    # labels up to renaming: the same partition of the non-root vertices, -1 exactly for the roots
    assert np.array_equal(label < 0, want.parent < 0)
    pairs = set(zip(label.tolist(), want.label.tolist()))
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})
    assert len(pairs) - bool((label < 0).any()) == n_components
    # a valid BFS forest: the roots are the smallest id of each connected component, and every parent is one level
    # nearer to its root (want.level: the BFS distances from those roots)
    _, comp = connected_components(csr_matrix((np.ones(len(col)), col, row_ptr), shape=(n, n)), directed=False)
    smallest = np.full(comp.max() + 1, n)
    np.minimum.at(smallest, comp, np.arange(n))
    assert np.array_equal(np.nonzero(parent < 0)[0], np.sort(smallest))
    nonroot = parent >= 0
    assert np.array_equal(want.level[parent[nonroot]], want.level[nonroot] - 1)
    assert np.all(comp[parent[nonroot]] == comp[nonroot])
    # the same bytes in a second run, and the same counts without the forest outputs
    (count2, parent2, label2), n2, _ = _kernel_run(G)
    assert count2.tobytes() == count.tobytes() and parent2.tobytes() == parent.tobytes()
    assert label2.tobytes() == label.tobytes() and n2 == n_components
    (count3, parent3, label3), n3, _ = _kernel_run(G, want_forest=False)
    assert parent3 is None and label3 is None
    assert count3.tobytes() == count.tobytes() and n3 == n_components


def test_igraph_with_loops_and_parallel_edges():
    from tests.test_igraph_adapter_cpu import _pair, _random_multigraph
    edges = _random_multigraph(np.random.default_rng(5), 400, 450, False, True, True)
    ig, H = _pair(400, edges, False)
    _check_public(ig, nx.Graph(H))


def test_csr_input_equals_networkx_input():
    from graphrole_amd import biconnected_component_counts, biconnected_components
    from graphrole_amd.graph.csr import CSRGraph
    G = nx.barabasi_albert_graph(2000, 5, seed=3)
    G.add_edges_from((v, 2000 + v) for v in range(50))           # pendant nodes: articulation points
    src, dst = np.array(list(G.edges)).T
    g = CSRGraph(G.number_of_nodes(), src, dst)
    a, b = biconnected_component_counts(g), biconnected_component_counts(G)
    assert a.to_numpy().tobytes() == b.to_numpy().tobytes() and list(a.index) == list(b.index)
    assert b.to_dict() == _nx_counts(G)
    assert _frozen(biconnected_components(g)) == _frozen(biconnected_components(G))


def test_karate_end_to_end_sense_making():
    from graphrole_amd import RecursiveFeatureExtractor, RoleExtractor, biconnected_component_counts, node_measures
    G = nx.karate_club_graph()
    features = RecursiveFeatureExtractor(G).extract_features()
    np.random.seed(0)
    role_extractor = RoleExtractor(n_roles=3)
    role_extractor.extract_role_factors(features)
    M = node_measures(G, ['degree', 'biconnected_components'])
    assert list(M.columns) == ['degree', 'biconnected_components']
    assert M['biconnected_components'].dtype == np.int64
    assert M['biconnected_components'].to_dict() == _nx_counts(G)
    assert M['biconnected_components'].to_numpy().tobytes() == biconnected_component_counts(G).to_numpy().tobytes()
    E = role_extractor.sense_making(M)
    assert E.shape == (3, 2) and list(E.columns) == list(M.columns)
    assert np.all(E.to_numpy() >= 0)


def test_directed_raises_before_any_device_work(monkeypatch):
    from graphrole_amd import (articulation_points, biconnected_component_counts, biconnected_components,
                               kernels as K, node_measures)
    from graphrole_amd.graph.interface.networkx import NetworkxInterface

    def no_device(*args, **kwargs):
        raise AssertionError('device work for a directed graph')

    monkeypatch.setattr(K, 'biconnected', no_device)
    monkeypatch.setattr(NetworkxInterface, '_device_graph', no_device)
    D = nx.gnm_random_graph(30, 90, seed=2, directed=True)
    for call in (lambda: biconnected_component_counts(D), lambda: articulation_points(D),
                 lambda: biconnected_components(D), lambda: node_measures(D, ['biconnected_components'])):
        with pytest.raises(NotImplementedError, match='directed'):
            call()
