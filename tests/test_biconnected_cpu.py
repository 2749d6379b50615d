"""
-m "not gpu": biconnected components without a device.  tests/biconnected_oracle.py (the numpy restatement of
csrc/grx_biconnected.hip, Tarjan-Vishkin on a BFS forest) against networkx -- per-node counts, the set of components
and the articulation set, exactly -- on a few thousand seeded small graphs, then the Python layer of
graphrole_amd.biconnected_component_counts / articulation_points / biconnected_components / node_measures over a CPU
double of kernels.biconnected (the oracle on the double's CSR arrays).  The device numbers are pinned in
tests/test_gpu_biconnected.py.
"""
import itertools
import random
import types
from collections import Counter

import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import biconnected_oracle as bo
from tests import fake_kernels


def _nx_counts(G):
    c = Counter(v for comp in nx.biconnected_components(G) for v in comp)
    return {v: c.get(v, 0) for v in G}


def _check_against_networkx(G):
    nodes, row_ptr, col = bo.graph_csr(G)
    r = bo.biconnected(row_ptr, col)
    want = _nx_counts(G)
    assert {v: int(r.count[i]) for i, v in enumerate(nodes)} == want
    comps = {frozenset(nodes[i] for i in c) for c in bo.components(r.parent, r.label)}
    assert comps == {frozenset(c) for c in nx.biconnected_components(G)}
    assert r.n_components == len(comps)
    assert {nodes[i] for i in np.nonzero(r.count > 1)[0]} == set(nx.articulation_points(G))
    # the forest and the numbering the later steps rely on
    n = len(nodes)
    nonroot = r.parent >= 0
    assert np.all(r.level[nonroot] == r.level[r.parent[nonroot]] + 1) and np.all(r.level[~nonroot] == 0)
    assert sorted(r.pre.tolist()) == list(range(n))
    for v in np.nonzero(nonroot)[0]:
        p = r.parent[v]
        assert r.pre[p] < r.pre[v] and r.pre[v] + r.size[v] <= r.pre[p] + r.size[p]
    return r


def _with_loops(G, rng, k):
    for v in rng.sample(list(G), min(k, len(G))):
        G.add_edge(v, v)
    return G


def _families(seed):
    rng = random.Random(seed)
    n = rng.randint(4, 28)
    yield nx.gnm_random_graph(n, rng.randint(0, 2 * n), seed=seed)
    yield nx.gnm_random_graph(n, rng.randint(n // 2, n + 2), seed=seed + 1)          # sparse: bridges, components
    yield nx.barabasi_albert_graph(n, 1, seed=seed)
    yield nx.barabasi_albert_graph(n, 2, seed=seed)
    yield nx.random_labeled_tree(n, seed=seed)
    yield nx.barbell_graph(rng.randint(3, 6), rng.randint(0, 4))
    yield nx.grid_2d_graph(rng.randint(1, 5), rng.randint(2, 5))
    yield nx.star_graph(rng.randint(1, 12))
    yield nx.windmill_graph(rng.randint(2, 5), rng.randint(2, 5))
    yield nx.disjoint_union(nx.gnm_random_graph(n, n + rng.randint(0, n), seed=seed + 2),
                            nx.disjoint_union(nx.cycle_graph(rng.randint(3, 9)), nx.empty_graph(2)))
    yield _with_loops(nx.gnm_random_graph(n, rng.randint(n // 2, 2 * n), seed=seed + 3), rng, 3)
    H = nx.gnm_random_graph(n, rng.randint(n // 2, 2 * n), seed=seed + 4)
    yield nx.relabel_nodes(H, dict(zip(H, rng.sample(list(H), len(H)))))              # ids against the BFS order


@pytest.mark.parametrize('block', range(10))
def test_oracle_equals_networkx_on_seeded_graphs(block):
    checked = 0
    for seed in range(block * 25, block * 25 + 25):
        for G in _families(7919 * seed):
            _check_against_networkx(G)
            checked += 1
    assert checked == 25 * 12


def test_oracle_small_and_degenerate_graphs():
    for G in (nx.empty_graph(1), nx.empty_graph(2), nx.path_graph(2), nx.empty_graph(3), nx.path_graph(3),
              nx.cycle_graph(3), nx.Graph([(0, 0)]), nx.Graph([(0, 0), (0, 1), (1, 1)]),
              nx.Graph([(0, 1), (2, 2)]), nx.path_graph(40), nx.cycle_graph(9), nx.complete_graph(6)):
        _check_against_networkx(G)
    r = _check_against_networkx(nx.Graph([(0, 0), (1, 2)]))
    assert r.count.tolist() == [0, 1, 1] and r.label.tolist() == [-1, -1, 2]


def test_oracle_every_graph_on_five_nodes():
    """Every graph on 5 labelled nodes (1 024 of them): all placements of non-tree edges between same-level and
    adjacent-level vertices at that size."""
    pairs = list(itertools.combinations(range(5), 2))
    for mask in range(1 << len(pairs)):
        G = nx.empty_graph(5)
        G.add_edges_from(p for k, p in enumerate(pairs) if mask >> k & 1)
        _check_against_networkx(G)


def test_oracle_non_tree_edges_same_and_adjacent_level():
    # root 0; level 1: 1, 2; level 2: 3 (under 1), 4 (under 2)
    tree = [(0, 1), (0, 2), (1, 3), (2, 4)]
    for extra in ([(1, 2)], [(3, 4)], [(1, 4)], [(2, 3)], [(1, 2), (3, 4)], [(2, 3), (1, 4)]):
        G = nx.Graph(tree + extra)
        r = _check_against_networkx(G)
        nodes = list(G)
        for u, w in extra:
            iu, iw = nodes.index(u), nodes.index(w)
            assert abs(r.level[iu] - r.level[iw]) <= 1
    r = _check_against_networkx(nx.Graph(tree + [(2, 3)]))
    assert r.parent.tolist() == [-1, 0, 0, 1, 2]                 # 3 keeps its smallest neighbour one level up


# ------------------------------------------------------------------------------------------ Python layer, CPU double
@pytest.fixture
def cpu_backend():
    import torch
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.calls = []

    def biconnected(csr, want_forest=True):
        double.calls.append(csr)
        r = bo.biconnected(csr.row_ptr, csr.col)
        return (torch.from_numpy(r.count), torch.from_numpy(r.parent.astype(np.int32)),
                torch.from_numpy(r.label.astype(np.int32)), r.n_components)

    double.biconnected = biconnected
    backend.use(double)
    yield double
    backend.use(None)


def _multigraph():
    return nx.MultiGraph([(0, 1), (0, 1), (1, 2), (2, 0), (2, 3), (3, 3), (3, 4), (4, 5), (5, 3), (5, 6), (5, 6)])


def _disconnected():
    G = nx.disjoint_union(nx.barabasi_albert_graph(60, 2, seed=1), nx.cycle_graph(9))
    G.add_nodes_from([1000, 1001])
    return G


GRAPHS = {
    'karate': nx.karate_club_graph,
    'sparse': lambda: nx.gnm_random_graph(120, 130, seed=3),
    'multigraph': _multigraph,
    'disconnected': _disconnected,
    'strings': lambda: nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
    'grid': lambda: nx.grid_2d_graph(4, 5),
    'n1': lambda: nx.empty_graph(1),
}


@pytest.mark.parametrize('key', list(GRAPHS))
def test_public_functions(cpu_backend, key):
    from graphrole_amd import articulation_points, biconnected_component_counts, biconnected_components
    G = GRAPHS[key]()
    S = nx.Graph(G)                                              # parallel edges count once
    counts = biconnected_component_counts(G)
    assert isinstance(counts, pd.Series) and counts.name == 'biconnected_components' and counts.dtype == np.int64
    assert list(counts.index) == sorted(G)
    assert counts.to_dict() == _nx_counts(S)
    points = articulation_points(G)
    assert isinstance(points, list) and points == sorted(nx.articulation_points(S))
    comps = biconnected_components(G)
    assert isinstance(comps, list) and all(isinstance(c, set) for c in comps)
    assert len(comps) == len({frozenset(c) for c in comps})
    assert {frozenset(c) for c in comps} == {frozenset(c) for c in nx.biconnected_components(S)}
    # the kernel got the structure CSR of the adapter
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    s_out = NetworkxInterface(G)._structure_csrs()[0]
    for csr in cpu_backend.calls:
        assert np.array_equal(csr.row_ptr, s_out.row_ptr) and np.array_equal(csr.col, s_out.col)


def test_catalogue_opt_in_and_cache(cpu_backend):
    from graphrole_amd import measures, node_measures
    assert measures.available_measures(False, False) == ['degree', 'weighted_degree', 'clustering', 'effective_size',
                                                         'pagerank', 'eigenvector']
    assert measures.available_measures(True, True) == ['degree', 'weighted_degree', 'in_degree', 'out_degree',
                                                       'pagerank']
    assert 'biconnected_components' in measures.CATALOGUE and 'biconnected_components' in measures.OPT_IN
    assert measures.CATALOGUE['biconnected_components'] == 'Counter(v for c in nx.biconnected_components(G) for v in c)'
    G = nx.karate_club_graph()
    M = node_measures(G, ['weighted_degree', 'biconnected_components', 'biconnected_components'])
    assert len(cpu_backend.calls) == 1                          # cached inside one call
    assert list(M.columns) == ['weighted_degree', 'biconnected_components', 'biconnected_components']
    M = node_measures(G, ['weighted_degree', 'biconnected_components'])
    assert M['biconnected_components'].dtype == np.int64
    assert list(M.index) == sorted(G)
    assert M['biconnected_components'].to_dict() == _nx_counts(G)
    assert 'biconnected_components' not in node_measures(G, ['weighted_degree']).columns


def test_directed_and_unknown_inputs(cpu_backend):
    from graphrole_amd import (articulation_points, biconnected_component_counts, biconnected_components,
                               node_measures)
    D = nx.gnm_random_graph(30, 90, seed=2, directed=True)
    for call in (lambda: biconnected_component_counts(D), lambda: articulation_points(D),
                 lambda: biconnected_components(D), lambda: node_measures(D, ['biconnected_components']),
                 lambda: biconnected_component_counts(nx.MultiDiGraph(D))):
        with pytest.raises(NotImplementedError, match='directed'):
            call()
    for fn in (biconnected_component_counts, articulation_points, biconnected_components):
        with pytest.raises(TypeError, match='supported libraries'):
            fn({'not': 'a graph'})
    assert cpu_backend.calls == []


def test_csr_and_igraph_inputs(cpu_backend):
    from graphrole_amd import biconnected_component_counts, biconnected_components
    from graphrole_amd.graph.csr import CSRGraph
    from tests.test_igraph_adapter_cpu import _pair, _random_multigraph
    G = nx.barabasi_albert_graph(60, 2, seed=8)
    src, dst = np.array(list(G.edges)).T
    a = biconnected_component_counts(CSRGraph(60, src, dst))
    assert a.to_numpy().tobytes() == biconnected_component_counts(G).to_numpy().tobytes()
    edges = _random_multigraph(np.random.default_rng(3), 70, 90, False, True, True)
    ig, H = _pair(70, edges, False)
    assert biconnected_component_counts(ig).to_dict() == _nx_counts(nx.Graph(H))
    assert ({frozenset(c) for c in biconnected_components(ig)}
            == {frozenset(c) for c in nx.biconnected_components(nx.Graph(H))})


def test_ctypes_signature_present():
    from graphrole_amd import _lib
    assert len(_lib._SIGNATURES['grx_biconnected'][1]) == 13
    assert len(_lib._SIGNATURES['grx_biconnected_workspace_bytes'][1]) == 1
    assert {'grx_biconnected', 'grx_biconnected_workspace_bytes'} <= set(_lib.EXPORTED_SYMBOLS)
