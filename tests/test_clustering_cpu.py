"""
-m "not gpu": the weighted and the directed clustering coefficient without a device.  tests/clustering_oracle.py (the two
array restatements of grx_clustering) against nx.clustering inside the tolerance the oracle module derives, and bit for
bit where no weight is involved; then the Python layer of graphrole_amd.clustering / average_clustering /
node_measures(..., clustering_weight=) over a CPU double of kernels.clustering (the exact oracle on the double's
arrays); the refusals; the catalogue; the ctypes signature, the header and the argument validation of the library.  The
device numbers are pinned in tests/test_gpu_clustering.py.
"""
import ctypes
import os
import random
import re
import types

import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import clustering_oracle as co
from tests import fake_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = 240


def _random_graph(i):
    """Graph i of the family of tests/test_structural_holes_cpu.py: undirected and directed, self-loops, integer / float
    / zero / missing weights, isolated nodes, directed nodes with in-arcs only."""
    rng = random.Random(1000 + i)
    n = rng.randint(2, 25)
    directed = i % 2 == 1
    G = nx.gnp_random_graph(n, rng.choice([0.08, 0.2, 0.45]), seed=i, directed=directed)
    if i % 3 == 0:
        G.add_edges_from((v, v) for v in rng.sample(list(G), min(3, n)))
    if i % 5 == 0:
        G.add_nodes_from([n, n + 1])                            # isolated
    if directed and i % 7 == 1:
        G.add_edges_from((v, n + 2) for v in rng.sample(range(n), min(2, n)))      # n + 2 has in-arcs only
    kind = i % 4
    for u, v in G.edges:
        if kind == 0:
            G[u][v]['weight'] = rng.choice([0, 1, 2, 5])        # integers and zeros
        elif kind == 1:
            G[u][v]['weight'] = rng.random()
        elif kind == 2 and rng.random() < 0.5:
            G[u][v]['weight'] = rng.choice([0.0, 0.25, 3.5])    # some edges without the attribute: they count 1
    return G


def _all_zero(G, weight):
    return weight is not None and G.number_of_edges() > 0 and max(d.get(weight, 1) for _, _, d in G.edges(data=True)) == 0


def _networkx_column(G, weight, nodes=None):
    want = nx.clustering(G, weight=weight)
    return np.array([want[v] for v in (sorted(G) if nodes is None else nodes)], dtype=np.float64)


def _check_against_networkx(G, weight, what):
    want = _networkx_column(G, weight)
    arrays = co.directional_csr(G, weight)
    for restate in (co.exact, co.sparse):
        got, t = restate(*arrays)
        co.assert_close(got, want, (what, restate.__name__))
        assert np.array_equal(t == 0, want == 0)
    if weight is None:
        assert np.array_equal(co.exact(*arrays)[0], want), what        # integers only: networkx's own quotient


@pytest.mark.parametrize('batch', range(8))
def test_oracles_against_networkx(batch):
    """240 graphs of at most 28 nodes, each with weight=None and weight='weight': zeros in the same places."""
    for i in range(30 * batch, 30 * batch + 30):
        G = _random_graph(i)
        for weight in (None, 'weight'):
            if _all_zero(G, weight):
                with pytest.raises(ZeroDivisionError):
                    nx.clustering(G, weight=weight)
                continue
            _check_against_networkx(G, weight, (i, weight))


def test_graphs_whose_weights_are_all_zero_are_few():
    skipped = sum(_all_zero(_random_graph(i), 'weight') for i in range(FAMILY))
    assert skipped < 0.02 * FAMILY, skipped


def test_oracles_against_networkx_on_karate_and_named_graphs():
    K = nx.karate_club_graph()                                  # carries its own integer weights
    _check_against_networkx(K, 'weight', 'karate weighted')
    _check_against_networkx(K, None, 'karate')
    _check_against_networkx(nx.star_graph(12), None, 'star')
    _check_against_networkx(nx.complete_graph(9), None, 'K9')
    _check_against_networkx(nx.complete_bipartite_graph(4, 5), None, 'K4,5')
    _check_against_networkx(nx.wheel_graph(14), None, 'wheel')
    _check_against_networkx(nx.path_graph(2), None, 'P2')
    _check_against_networkx(nx.empty_graph(3), None, 'empty')
    D = nx.DiGraph([(0, 1), (1, 0), (1, 2), (3, 1), (2, 2), (2, 4), (0, 2), (3, 0)])   # reciprocal pair, loop,
    for weight in (None, 'weight'):                                                   # out-only 3, in-only 4
        _check_against_networkx(D, weight, ('digraph', weight))
    D[1][2]['weight'] = 2.5
    D[0][1]['weight'] = 0.0
    _check_against_networkx(D, 'weight', 'digraph weighted')
    assert np.all(co.exact(*co.directional_csr(nx.complete_graph(9)))[0] == 1.0)
    assert np.all(co.exact(*co.directional_csr(nx.complete_graph(9, create_using=nx.DiGraph)))[0] == 1.0)


def test_oracle_layout():
    D = nx.DiGraph()
    D.add_weighted_edges_from([(0, 1, 2.0), (1, 0, 4.0), (1, 2, 0.0), (2, 2, 8.0), (3, 1, 1.0)])
    rp, col, fwd, bwd, mw = co.directional_csr(D, 'weight')
    assert rp.tolist() == [0, 1, 4, 6, 7] and col.tolist() == [1, 0, 2, 3, 1, 2, 1]
    assert fwd.tolist() == [2, 4, 0, -1, -1, 8, 1] and bwd.tolist() == [4, 2, -1, 1, 0, 8, -1]
    assert mw == 8.0                                            # the loop counts in the maximum
    s, dirs = co.arc_values(rp, fwd, bwd, mw)
    assert dirs == [2, 2, 1, 1, 1, 2, 1] and s[2] == 0.0        # a zero weight is a present direction
    assert co.denominators(rp, col, dirs, True) == [2 * (2 * 1 - 2), 2 * (4 * 3 - 2), 0, 0]
    rp, col, fwd, bwd, mw = co.directional_csr(D, None)
    assert fwd.tolist() == [1, 1, 1, -1, -1, 1, 1] and mw == 1.0
    U = nx.barabasi_albert_graph(40, 3, seed=2)
    rp, col, fwd, bwd, mw = co.directional_csr(U, None)
    assert fwd is None and bwd is None and mw == 1.0
    rp2, col2, f2, mw2 = co.csr_from_pairs(40, list(U.edges))
    assert np.array_equal(rp2, rp) and np.array_equal(col2, col) and f2 is None and mw2 == 1.0
    rp3, col3, f3, mw3 = co.csr_from_pairs(40, list(U.edges), lambda a, b: 1 + (a + b) % 4)
    assert np.array_equal(col3, col) and mw3 == f3.max() == 4.0
    G = nx.Graph(U)
    for u, v in G.edges:
        G[u][v]['weight'] = 1 + (min(u, v) + max(u, v)) % 4
    assert np.array_equal(co.directional_csr(G, 'weight')[2], f3)


# ------------------------------------------------------------------------------------------------- exact properties
@pytest.mark.parametrize('seed', range(6))
def test_unweighted_forms_equal_networkx_bit_for_bit_and_constant_weights_change_nothing(seed):
    for directed in (False, True):
        G = nx.gnp_random_graph(30, 0.3, seed=seed, directed=directed)
        G.add_edges_from([(0, 0), (3, 3)])
        plain = co.exact(*co.directional_csr(G, None))[0]
        assert np.array_equal(plain, _networkx_column(G, None))
        for constant in (1, 3, 0.1, 7.25):
            nx.set_edge_attributes(G, constant, 'weight')
            assert np.array_equal(co.exact(*co.directional_csr(G, 'weight'))[0], plain), (directed, constant)


# ------------------------------------------------------------------------------------------ Python layer, CPU double
@pytest.fixture
def cpu_backend():
    import torch
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.calls = []

    from tests import test_sense_cpu as sense               # the doubles of the existing clustering column
    double.row_counts = sense._row_counts
    double.triangle_counts = sense._triangle_counts
    double.local_structure = sense._local_structure
    double.pagerank = sense._pagerank                       # the default table
    double.eigenvector_centrality = sense._eigenvector

    def host(x):
        return None if x is None else np.asarray(x, dtype=np.float64)

    def clustering(csr, fwd=None, bwd=None, max_weight=1.0, want_triangles=False, lanes=None):
        fwd, bwd = host(fwd), host(bwd)
        nnz = int(csr.row_ptr[-1])
        fwd, bwd = (None if fwd is None else fwd[:nnz]), (None if bwd is None else bwd[:nnz])
        double.calls.append(dict(csr=csr, fwd=fwd, bwd=bwd, max_weight=max_weight, triangles=want_triangles))
        c, t = co.exact(csr.row_ptr, csr.col, fwd, bwd, max_weight)
        return torch.from_numpy(c), (torch.from_numpy(t) if want_triangles else None)

    double.clustering = clustering
    backend.use(double)
    yield double
    backend.use(None)


def _series_close(series, G, weight, nodes=None):
    assert isinstance(series, pd.Series) and series.name == 'clustering' and series.dtype == np.float64
    index = sorted(G) if nodes is None else sorted(set(nodes))
    assert list(series.index) == index
    co.assert_close(series.to_numpy(), _networkx_column(G, weight, index))


def _weighted_digraph(n=25, m=90, seed=3):
    G = nx.gnm_random_graph(n, m, seed=seed, directed=True)
    rng = random.Random(seed)
    for u, v in G.edges:
        G[u][v]['weight'] = rng.choice([0.5, 1.0, 2.0, 7.25])
    G.add_edges_from([(0, 0, {'weight': 30.0}), (4, 4, {'weight': 0.5})])      # the heaviest edge is a loop
    G.add_node(n)                                               # isolated
    G.add_edge(1, n + 1, weight=2.0)                            # n + 1 has an in-arc only
    return G


def _with_loops(G):
    G.add_edges_from([(0, 0), (7, 7), (19, 19)])
    return G


API_GRAPHS = {
    'karate': nx.karate_club_graph,
    'strings': lambda: nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
    'loops': lambda: _with_loops(nx.gnp_random_graph(20, 0.3, seed=6)),
    'digraph': _weighted_digraph,
    'isolated': lambda: nx.disjoint_union(nx.path_graph(4), nx.empty_graph(2)),
}


@pytest.mark.parametrize('key', list(API_GRAPHS))
@pytest.mark.parametrize('weight', [None, 'weight'])
def test_clustering_and_its_average_of_every_node(cpu_backend, key, weight):
    from graphrole_amd import average_clustering, clustering
    G = API_GRAPHS[key]()
    _series_close(clustering(G, weight=weight), G, weight)
    if G.is_directed() or weight is not None:
        (call,) = cpu_backend.calls
        assert not call['triangles'] and (call['bwd'] is not None) == G.is_directed()
        if weight is None:
            assert call['max_weight'] == 1.0
    else:
        assert cpu_backend.calls == []                          # the existing column: triangle counts
    for count_zeros in (True, False):
        if key == 'isolated' and not count_zeros:               # a path and two isolated nodes: no non-zero value
            for average in (average_clustering, nx.average_clustering):
                with pytest.raises(ZeroDivisionError):
                    average(G, weight=weight, count_zeros=False)
            continue
        got = average_clustering(G, weight=weight, count_zeros=count_zeros)
        want = nx.average_clustering(G, weight=weight, count_zeros=count_zeros)
        assert isinstance(got, float) and abs(got - want) <= co.RTOL * want


def test_unweighted_forms_are_networkx_bit_for_bit(cpu_backend):
    from graphrole_amd import clustering, node_measures
    for key in ('loops', 'digraph', 'karate'):
        G = API_GRAPHS[key]()
        assert np.array_equal(clustering(G).to_numpy(), _networkx_column(G, None)), key
    G = API_GRAPHS['loops']()
    old = node_measures(G, ['clustering'])['clustering']
    got = clustering(G)
    assert np.array_equal(got.to_numpy(), old.to_numpy()) and list(got.index) == list(old.index)


def test_kernel_arguments_of_both_kinds_of_graph(cpu_backend):
    from graphrole_amd import clustering
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    G = nx.karate_club_graph()
    clustering(G, weight='weight')
    (call,) = cpu_backend.calls
    _, out, _ = NetworkxInterface(G)._device_graph()
    assert np.array_equal(call['csr'].row_ptr, out.row_ptr) and np.array_equal(call['csr'].col, out.col)
    assert np.array_equal(call['fwd'], out.w) and call['bwd'] is None
    assert call['max_weight'] == max(d['weight'] for _, _, d in G.edges(data=True))
    cpu_backend.calls.clear()
    D = nx.DiGraph()
    D.add_weighted_edges_from([('a', 'b', 1.5), ('b', 'a', 2.0), ('b', 'c', 4.0), ('c', 'c', 9.0), ('d', 'b', 0.0)])
    adapter = NetworkxInterface(D)
    host = adapter._device_graph()[0]
    internal = {v: int(host.inv[i]) for i, v in enumerate(sorted(D))}
    for weight, want, mw in (('weight', {('a', 'b'): (1.5, 2.0), ('b', 'c'): (4.0, -1.0), ('c', 'c'): (9.0, 9.0),
                                         ('d', 'b'): (0.0, -1.0)}, 9.0),
                             (None, {('a', 'b'): (1.0, 1.0), ('b', 'c'): (1.0, -1.0), ('c', 'c'): (1.0, 1.0),
                                     ('d', 'b'): (1.0, -1.0)}, 1.0)):
        cpu_backend.calls.clear()
        _series_close(clustering(adapter.G, weight=weight), D, weight)
        (call,) = cpu_backend.calls
        csr = call['csr']
        rows = np.repeat(np.arange(csr.n), np.diff(csr.row_ptr))
        got = {(int(r), int(c)): (float(f), float(b)) for r, c, f, b in zip(rows, csr.col, call['fwd'], call['bwd'])}
        full = {}
        for (u, v), (f, b) in want.items():
            full[(internal[u], internal[v])] = (f, b)
            full[(internal[v], internal[u])] = (b, f)
        assert got == full and call['max_weight'] == mw
        for r in range(csr.n):                                  # ascending and distinct inside a row
            assert np.all(np.diff(csr.col[csr.row_ptr[r]:csr.row_ptr[r + 1]]) > 0)


def test_nodes_argument_and_string_labels(cpu_backend):
    from graphrole_amd import average_clustering, clustering
    G = API_GRAPHS['strings']()
    bunch = ['node-30', 'node-02', 'node-11', 'node-02']
    _series_close(clustering(G, nodes=bunch, weight='weight'), G, 'weight', bunch)
    _series_close(clustering(G, nodes=iter(['node-33'])), G, None, ['node-33'])      # the existing column, sliced
    assert len(clustering(G, nodes=[])) == 0
    D = _weighted_digraph()
    _series_close(clustering(D, nodes=[26, 3, 25], weight='weight'), D, 'weight', [26, 3, 25])
    got = average_clustering(D, nodes=[2, 3, 9], weight='weight')
    assert abs(got - nx.average_clustering(D, nodes=[2, 3, 9], weight='weight')) <= co.RTOL * got
    for call in (lambda: clustering(G, nodes=['node-00', 'nobody']), lambda: clustering(D, nodes=[99], weight='weight'),
                 lambda: average_clustering(D, nodes=[99])):
        with pytest.raises(KeyError):
            call()


def test_empty_graphs_and_averages_without_values(cpu_backend):
    from graphrole_amd import average_clustering, clustering
    for E in (nx.Graph(), nx.DiGraph()):
        for weight in (None, 'weight'):
            got = clustering(E, weight=weight)
            assert len(got) == 0 and got.name == 'clustering' and got.dtype == np.float64
            with pytest.raises(ZeroDivisionError):
                average_clustering(E, weight=weight)
            with pytest.raises(ZeroDivisionError):
                nx.average_clustering(E, weight=weight)
    P = nx.path_graph(5)                                        # no triangle: every value 0
    assert average_clustering(P) == 0.0
    for call in (lambda: average_clustering(P, count_zeros=False),
                 lambda: average_clustering(nx.DiGraph(P), count_zeros=False),
                 lambda: nx.average_clustering(P, count_zeros=False)):
        with pytest.raises(ZeroDivisionError):
            call()
    got = clustering(nx.DiGraph(P))
    assert np.all(got.to_numpy() == 0.0) and got.dtype == np.float64


def test_node_measures_keyword(cpu_backend):
    from graphrole_amd import clustering, node_measures
    G = nx.karate_club_graph()
    M = node_measures(G, ['clustering', 'degree', 'clustering'], clustering_weight='weight')
    assert list(M.columns) == ['clustering', 'degree', 'clustering'] and list(M.index) == sorted(G)
    co.assert_close(M['clustering'].iloc[:, 0].to_numpy(), _networkx_column(G, 'weight'))
    assert len(cpu_backend.calls) == 1                          # computed once for both columns
    assert M['degree'].to_dict() == dict(G.degree())
    assert np.array_equal(M['clustering'].iloc[:, 1].to_numpy(), clustering(G, weight='weight').to_numpy())
    cpu_backend.calls.clear()
    M = node_measures(G, clustering_weight='weight')            # the default table of an undirected graph has the column
    co.assert_close(M['clustering'].to_numpy(), _networkx_column(G, 'weight'))
    D = _weighted_digraph()
    M = node_measures(D, ['out_degree', 'clustering'], clustering_weight='weight')
    assert list(M.index) == sorted(D)
    co.assert_close(M['clustering'].to_numpy(), _networkx_column(D, 'weight'))
    node_measures(G, ['degree'], clustering_weight='anything')  # not validated unless 'clustering' is named


def test_without_the_keyword_nothing_changes(cpu_backend):
    from graphrole_amd import node_measures
    G = nx.karate_club_graph()
    M = node_measures(G, ['clustering'])
    assert np.array_equal(M['clustering'].to_numpy(), _networkx_column(G, None))      # the weights are not read
    assert cpu_backend.calls == []
    D = _weighted_digraph()
    with pytest.raises(NotImplementedError, match=r'nx\.clustering'):
        node_measures(D, ['clustering'])
    with pytest.raises(NotImplementedError, match=r'nx\.clustering'):
        node_measures(nx.MultiGraph([(0, 1), (0, 1), (1, 2)]), ['clustering'])
    assert 'clustering' not in node_measures(D).columns
    assert 'clustering' not in node_measures(D, clustering_weight='weight').columns    # the default table is pinned
    assert cpu_backend.calls == []


def test_csr_graph_input(cpu_backend):
    from graphrole_amd import clustering
    from graphrole_amd.graph.csr import CSRGraph
    G = nx.karate_club_graph()
    src, dst, w = zip(*G.edges(data='weight'))
    C = CSRGraph(34, src, dst, weights=np.asarray(w, dtype=np.float64))
    for weight in (None, 'weight'):
        assert np.array_equal(clustering(C, weight=weight).to_numpy(), clustering(G, weight=weight).to_numpy())
    D = _weighted_digraph()
    src, dst, w = zip(*D.edges(data='weight'))
    C = CSRGraph(D.number_of_nodes(), src, dst, weights=np.asarray(w), directed=True)
    for weight in (None, 'weight'):
        assert np.array_equal(clustering(C, weight=weight).to_numpy(), clustering(D, weight=weight).to_numpy())


def test_refusals_make_no_kernel_call(cpu_backend):
    from graphrole_amd import average_clustering, clustering, node_measures
    from graphrole_amd.graph.csr import CSRGraph
    G = nx.karate_club_graph()
    for call in (lambda: clustering(G, weight='capacity'), lambda: average_clustering(G, weight='capacity'),
                 lambda: clustering(G, weight=lambda u, v, d: 1),
                 lambda: node_measures(G, ['clustering'], clustering_weight='w')):
        with pytest.raises(NotImplementedError, match=r'nx\.clustering\(G, weight='):
            call()
    for M in (nx.MultiGraph([(0, 1), (0, 1), (1, 2)]), nx.MultiDiGraph([(0, 1), (1, 0), (1, 2)])):
        for call in (lambda: clustering(M), lambda: clustering(M, weight='weight'), lambda: average_clustering(M),
                     lambda: node_measures(M, ['clustering'], clustering_weight='weight')):
            with pytest.raises(NotImplementedError, match='multigraph'):
                call()
        with pytest.raises(nx.NetworkXNotImplemented):
            nx.clustering(M)
    for bad in (-1.0, float('nan'), float('inf')):
        for B in (nx.path_graph(4), nx.path_graph(4, create_using=nx.DiGraph)):
            B[1][2]['weight'] = bad
            for call in (lambda: clustering(B, weight='weight'), lambda: average_clustering(B, weight='weight'),
                         lambda: node_measures(B, ['clustering'], clustering_weight='weight')):
                with pytest.raises(ValueError, match='finite and >= 0'):
                    call()
        C = CSRGraph(3, [0, 1], [1, 2], weights=[1.0, bad], directed=True)
        with pytest.raises(ValueError, match='finite and >= 0'):
            clustering(C, weight='weight')
    for Z in (nx.complete_graph(4), nx.complete_graph(4, create_using=nx.DiGraph)):
        nx.set_edge_attributes(Z, 0.0, 'weight')
        for call in (lambda: clustering(Z, weight='weight'),
                     lambda: node_measures(Z, ['clustering'], clustering_weight='weight')):
            with pytest.raises(ValueError, match='every edge weight is 0'):
                call()
        with pytest.raises(ZeroDivisionError):
            nx.clustering(Z, weight='weight')
    with pytest.raises(TypeError, match='supported libraries'):
        clustering({'not': 'a graph'})
    assert cpu_backend.calls == []
    B = nx.path_graph(4, create_using=nx.DiGraph)
    B[1][2]['weight'] = -1.0
    clustering(B)                                               # weight=None never reads the attribute
    assert len(cpu_backend.calls) == 1


def test_igraph_parallel_edges_are_refused(cpu_backend):
    from graphrole_amd import clustering
    from tests.test_igraph_adapter_cpu import _pair
    ig, H = _pair(6, [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4)], True)
    _series_close(clustering(ig), H, None)
    calls = len(cpu_backend.calls)
    assert calls == 1
    ig, _ = _pair(6, [(0, 1), (0, 1), (1, 2)], True)
    with pytest.raises(NotImplementedError, match='multigraph'):
        clustering(ig)
    assert len(cpu_backend.calls) == calls


def test_catalogue_and_opt_in_are_unchanged():
    from graphrole_amd import measures
    names = list(measures.CATALOGUE)
    assert len(names) == 16 and len(measures.OPT_IN) == 8 and names[-1] == 'eccentricity'
    assert measures.CATALOGUE['clustering'] == 'nx.clustering(G)' and 'clustering' not in measures.OPT_IN
    assert 'clustering' in measures.available_measures(False, False)
    assert 'clustering' not in measures.available_measures(True, False)
    why = measures._unavailable('clustering', True, False)
    assert 'nx.clustering' in why and 'clustering(G)' in why
    assert 'multigraph' in measures._unavailable('clustering', False, True)
    import graphrole_amd
    assert graphrole_amd.clustering is measures.clustering
    assert graphrole_amd.average_clustering is measures.average_clustering


# ---------------------------------------------------------------------------------------------------------- ABI
_C_TYPES = {'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'size_t': ctypes.c_size_t, 'double': ctypes.c_double}


def _declared_arguments(header, name):
    text = re.search(r'\b' + name + r'\s*\(([^)]*)\)\s*;', header).group(1)
    out = []
    for arg in text.split(','):
        arg = ' '.join(arg.split())
        out.append(ctypes.c_void_p if '*' in arg else _C_TYPES[arg.replace('const ', '').rsplit(' ', 1)[0]])
    return out


def test_header_declaration_matches_the_ctypes_signature():
    from graphrole_amd import _lib, kernels
    header = open(os.path.join(ROOT, 'include', 'grx.h')).read()
    for name, restype in (('grx_clustering', ctypes.c_int), ('grx_clustering_workspace_bytes', ctypes.c_size_t)):
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[name] == (restype, _declared_arguments(header, name))
    assert len(_lib._SIGNATURES['grx_clustering'][1]) == 14
    assert _lib._SIGNATURES['grx_clustering'][1][5] is ctypes.c_double      # max_weight travels by value
    assert 'A NEGATIVE value marks a direction that is absent' in header
    assert callable(kernels.clustering)
    source = open(os.path.join(ROOT, 'graphrole_amd', 'csrc', 'grx_clustering.hip')).read()
    shared = open(os.path.join(ROOT, 'graphrole_amd', 'csrc', 'grx_rowjoin.h')).read()
    assert '#include "grx_rowjoin.h"' in source and 'fp contract(off)' in shared.split('#pragma once')[0]
    for constant in ('RJ_BLOCK', 'RJ_ROW_MAX_WG', 'RJ_ARC_MAX_WG'):     # the copies the GPU test sizes its graphs by
        assert int(re.search(r'constexpr int ' + constant + r' = (\d+);', shared).group(1)) == getattr(kernels, constant)
    assert '#pragma clang fp contract(off)' in source
    makefile = open(os.path.join(ROOT, 'graphrole_amd', 'csrc', 'Makefile')).read()
    assert 'grx_rowjoin.h' in re.search(r'%\.o: %\.hip (.*)', makefile).group(1)      # a dependency of every object
    assert 'grx_clustering.hip' in makefile and 'grx_clustering.o: FILEFLAGS := -ffp-contract=off' in makefile


def test_argument_validation_needs_no_device():
    """GRX_REQUIRE runs before any HIP call: n range, no output, weights in one direction only, max_weight, null
    pointers, lanes, hub list, a workspace below what the row array alone needs.  n = 0 is an empty result."""
    from graphrole_amd import _lib
    lib = _lib.load()
    size = lib.grx_clustering_workspace_bytes
    assert size(10, 0) >= 8 * 10                                # the denominators
    assert 8 * 10 + 20 * 1000 <= size(10, 1000) <= 8 * 10 + 20 * 1000 + 4 * 256     # + s, the term and the row per arc
    assert size(0, 0) > 0 and size(10, 1001) >= size(10, 1000)
    need = size(10, 0)
    p = ctypes.c_void_p(4096)                                   # never dereferenced: every call fails validation

    def call(n=10, row_ptr=p, col=p, fwd=None, bwd=None, max_weight=1.0, hubs=None, n_hubs=0, lanes=8, out=p, tri=None,
             ws=p, ws_bytes=need):
        return lib.grx_clustering(n, row_ptr, col, fwd, bwd, max_weight, hubs, n_hubs, lanes, out, tri, ws, ws_bytes,
                                  None)

    for bad in (dict(n=-1), dict(n=1 << 31), dict(out=None), dict(row_ptr=None), dict(col=None), dict(ws=None),
                dict(bwd=p), dict(fwd=p, max_weight=0.0), dict(fwd=p, max_weight=-2.0),
                dict(fwd=p, max_weight=float('inf')), dict(fwd=p, bwd=p, max_weight=float('nan')),
                dict(lanes=0), dict(lanes=12), dict(lanes=64), dict(n_hubs=3), dict(n_hubs=-1), dict(n_hubs=11, hubs=p),
                dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert call(**bad) == -1, bad
        assert b'grx_clustering' in lib.grx_last_error()
    assert call(fwd=p, max_weight=0.0) == -1 and b'max_weight' in lib.grx_last_error()
    assert call(n=0, row_ptr=None, col=None, ws=None, ws_bytes=0) == 0
    assert call(n=0, out=None) == -1                            # the output is required even then
