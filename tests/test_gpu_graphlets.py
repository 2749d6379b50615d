"""
Graphlet degree vectors on the MI355X: graphrole_amd.graphlet_degree_vectors equal (integers: compared with ==) to the
brute-force enumeration of tests/graphlet_oracle.py on the small graphs -- karate (every one of the 15 orbits occurs),
G(30, 0.3), every graph on five labelled nodes in one call (every orbit in every overlap pattern), the empty graph, one
edge, K3, K4, K5 -- and to the oracle's restatement of the formulas on the graphs brute force cannot reach: hub rows
(BA 2000), a wheel whose hub row is longer than 32 x 32, a book (one edge of support 1 500), a 40-clique behind a tail
(91 390 4-cliques), a grid, a tree, K(60, 60) and a graph with isolated nodes; kernels.graphlet_orbits on the adapter's
CSR against the oracle on the same arrays (orbits, non-induced counts, triangles per arc) for every lane width; the same
bytes in a second run and for a relabelled copy; the refusals; and the karate sense-making run with the 15 columns.
"""
import functools
from math import comb

import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import graphlet_oracle as go
from tests.test_gpu_truss import _book, _clique_with_tail, _disconnected, _five_node_union

pytestmark = pytest.mark.gpu

COLUMNS = [f'orbit_{k}' for k in range(15)]

BRUTE = {
    'karate': nx.karate_club_graph,
    'strings': lambda: nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
    'gnp30': lambda: nx.gnp_random_graph(30, 0.3, seed=7),
    'five_nodes': _five_node_union,
    'empty5': lambda: nx.empty_graph(5),
    'n2': lambda: nx.path_graph(2),
    'k3': lambda: nx.complete_graph(3),
    'k4': lambda: nx.complete_graph(4),
    'k5': lambda: nx.complete_graph(5),
}
FORMULAS = {
    'ba2000': lambda: nx.barabasi_albert_graph(2000, 5, seed=3),
    'wheel': lambda: nx.wheel_graph(1501),
    'book': _book,
    'clique_tail': _clique_with_tail,
    'grid40': lambda: nx.grid_2d_graph(40, 40),
    'tree': lambda: nx.random_labeled_tree(500, seed=11),
    'k60_60': lambda: nx.complete_bipartite_graph(60, 60),
    'disconnected': _disconnected,
}
GRAPHS = {**BRUTE, **FORMULAS}


@functools.lru_cache(maxsize=None)
def _graph(key):
    return GRAPHS[key]()


@functools.lru_cache(maxsize=None)
def _want(key):
    """{node: [o0 .. o14]}: by enumeration where that is affordable, else by the oracle's formulas; computed once per
    graph and never changed."""
    return go.brute_orbits(_graph(key)) if key in BRUTE else go.graph_orbits(_graph(key))


@functools.lru_cache(maxsize=None)
def _frame(key):
    from graphrole_amd import graphlet_degree_vectors
    return graphlet_degree_vectors(_graph(key))


def _column_sums(key):
    return np.array(list(_want(key).values()), dtype=np.int64).reshape(-1, 15).sum(axis=0)


@pytest.mark.parametrize('key', list(GRAPHS))
def test_matches_the_oracle(key):
    G = _graph(key)
    frame = _frame(key)
    assert isinstance(frame, pd.DataFrame) and list(frame.columns) == COLUMNS
    assert all(dt == np.int64 for dt in frame.dtypes)
    order = sorted(G)
    assert list(frame.index) == order and frame.shape == (len(order), 15)
    want = _want(key)
    assert frame.to_numpy().tolist() == [want[v] for v in order]
    s = _column_sums(key)
    assert frame.attrs['graphlets'] == dict(edge=s[0] // 2, path3=s[2], triangle=s[3] // 3, path4=s[4] // 2, star4=s[7],
                                            cycle4=s[8] // 4, paw=s[9], diamond=s[13] // 2, clique4=s[14] // 4)


def test_closed_forms():
    book = _frame('book')
    assert book.loc[0, 'orbit_13'] == book.loc[1, 'orbit_13'] == comb(1500, 2)
    assert set(book.loc[2:, 'orbit_12']) == {1499} and set(book.loc[2:, 'orbit_3']) == {1}
    clique = _frame('clique_tail')
    assert set(clique.loc[:39, 'orbit_14']) == {comb(39, 3)} and not clique.loc[40:, 'orbit_14'].any()
    wheel = _frame('wheel')
    # the independent triples of the rim: all, less those with one adjacent pair, less the paths on three rim nodes
    assert wheel.loc[0, 'orbit_3'] == 1500 and wheel.loc[0, 'orbit_7'] == comb(1500, 3) - 1500 * 1496 - 1500
    k5 = _frame('k5')
    assert k5.to_numpy().tolist() == [[4, 0, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4]] * 5
    assert not _frame('empty5').to_numpy().any()


def test_the_graph_kinds_are_what_they_are_here_for():
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    assert np.all(_column_sums('karate') > 0)                   # every orbit occurs
    G = _graph('ba2000')
    assert max(d for _, d in G.degree()) == 215 and sum(nx.triangles(G).values()) // 3 == 1423
    assert _column_sums('ba2000')[14] // 4 == 147
    assert 147 == sum(1 for c in nx.enumerate_all_cliques(G) if len(c) == 4)
    for key in ('ba2000', 'wheel', 'book'):
        assert NetworkxInterface(_graph(key))._structure_csrs()[0].n_hubs > 0, key
    assert max(d for _, d in _graph('wheel').degree()) == 1500 > 32 * 32
    assert len(set(_graph('book')[0]) & set(_graph('book')[1])) == 1500
    G = _graph('five_nodes')
    assert G.number_of_nodes() == 5120 and np.all(_column_sums('five_nodes') > 0)
    assert _column_sums('clique_tail')[14] // 4 == comb(40, 4) == 91390
    zero = {key: set(np.nonzero(_column_sums(key) == 0)[0].tolist()) for key in ('grid40', 'tree', 'k60_60')}
    assert zero['grid40'] == {3, 9, 10, 11, 12, 13, 14}         # only 0, 1, 2, 4, 5, 6, 7, 8
    assert zero['tree'] == {3, 8, 9, 10, 11, 12, 13, 14}
    assert zero['k60_60'] == {3, 4, 5, 9, 10, 11, 12, 13, 14}   # a path on 4 nodes of K(a, b) closes to a 4-cycle
    want = _want('disconnected')
    assert want[1000] == [0] * 15 and want[1001] == [0] * 15


def _kernel_run(csr, **kwargs):
    from graphrole_amd import kernels as K
    orbits, non, tri = K.graphlet_orbits(csr, want_noninduced=True, want_arc_triangles=True, **kwargs)
    return K.to_host(orbits).copy(), K.to_host(non).copy(), K.to_host(tri)[:csr.nnz].copy()


@pytest.mark.parametrize('key', ['ba2000', 'book', 'clique_tail', 'five_nodes'])
def test_kernel_equals_oracle_on_the_same_csr(key):
    from graphrole_amd import kernels as K
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    csr = NetworkxInterface(_graph(key))._structure_csrs()[0]
    row_ptr = K.to_host(csr.row_ptr).astype(np.int64)
    col = K.to_host(csr.col)[:csr.nnz].astype(np.int64)
    want = go.orbits(row_ptr, col)
    orbits, non, tri = _kernel_run(csr)
    assert orbits.dtype == np.int64 and non.dtype == np.int64 and tri.dtype == np.int32
    assert orbits.shape == (15, csr.n) and non.shape == (15, csr.n)
    assert np.array_equal(tri, want.arc_triangles)
    assert np.array_equal(non, want.noninduced)
    assert np.array_equal(orbits, want.orbits)
    # both arcs of every edge hold the same t
    rows = np.repeat(np.arange(csr.n, dtype=np.int64), np.diff(row_ptr))
    reverse = np.searchsorted(rows * csr.n + col, col * csr.n + rows)
    assert np.array_equal(tri[reverse], tri)
    plain = K.graphlet_orbits(csr)
    assert plain[1] is None and plain[2] is None and K.to_host(plain[0]).tobytes() == orbits.tobytes()
    for lanes in (4, 8, 16, 32):
        orbits2, non2, tri2 = _kernel_run(csr, lanes=lanes)
        assert orbits2.tobytes() == orbits.tobytes() and non2.tobytes() == non.tobytes(), lanes
        assert tri2.tobytes() == tri.tobytes(), lanes


def test_kernel_on_a_csr_without_arcs_zeroes_the_outputs():
    from graphrole_amd import kernels as K
    csr = K.DeviceCSR(np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32))
    orbits, non, tri = K.graphlet_orbits(csr, want_noninduced=True, want_arc_triangles=True)
    assert K.to_host(orbits).tolist() == [[0] * 5] * 15 and K.to_host(non).tolist() == [[0] * 5] * 15


def test_kernel_refuses_an_orientation_that_is_not_one_arc_per_edge():
    from graphrole_amd import _lib, kernels as K
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    csr = NetworkxInterface(_graph('karate'))._structure_csrs()[0]
    csr._oriented = csr                                         # both arcs of every edge: o_row_ptr[n] = nnz
    with pytest.raises(_lib.GrxInvalid, match=r'grx_graphlet_orbits: o_row_ptr\[n\] = 156'):
        K.graphlet_orbits(csr)


def test_relabelled_copy_and_second_run_give_the_same_bytes():
    from graphrole_amd import graphlet_degree_vectors
    G = _graph('ba2000')
    a, b = _frame('ba2000'), graphlet_degree_vectors(G)
    assert list(a.index) == list(b.index) and a.to_numpy().tobytes() == b.to_numpy().tobytes()
    shuffled = np.random.default_rng(5).permutation(2000)
    H = nx.relabel_nodes(G, {v: int(shuffled[v]) for v in G})   # other ids: other rows, orientation, hub blocks
    c = graphlet_degree_vectors(H)
    back = c.loc[[int(shuffled[v]) for v in a.index]]
    assert back.to_numpy().tobytes() == a.to_numpy().tobytes()
    assert c.attrs == a.attrs


def test_refusals_reach_no_device_entry_point(monkeypatch):
    from graphrole_amd import graphlet_counts, graphlet_degree_vectors, kernels as K
    from graphrole_amd.graph.interface.networkx import NetworkxInterface

    def no_device(*args, **kwargs):
        raise AssertionError('device work for a refused graph')

    monkeypatch.setattr(K, 'graphlet_orbits', no_device)
    monkeypatch.setattr(NetworkxInterface, '_device_graph', no_device)
    D = nx.gnm_random_graph(30, 90, seed=2, directed=True)
    L = nx.karate_club_graph()
    L.add_edge(3, 3)
    M = nx.MultiGraph([(0, 1), (0, 1), (1, 2)])
    for fn in (graphlet_degree_vectors, graphlet_counts):
        for G, word in ((D, 'to_undirected'), (L, 'selfloop_edges'), (M, 'multigraph')):
            with pytest.raises(NotImplementedError, match=word):
                fn(G)
        with pytest.raises(TypeError, match='supported libraries'):
            fn({'not': 'a graph'})


def test_graphlet_counts_and_nodes_argument():
    from graphrole_amd import graphlet_counts, graphlet_degree_vectors
    G = _graph('karate')
    counts = graphlet_counts(G)
    assert counts.dtype == np.int64 and counts.to_dict() == _frame('karate').attrs['graphlets']
    assert counts['edge'] == 78 and counts['triangle'] == 45
    assert counts['clique4'] == sum(1 for c in nx.enumerate_all_cliques(G) if len(c) == 4)
    one = graphlet_degree_vectors(G, 33)
    assert isinstance(one, pd.Series) and one.tolist() == _want('karate')[33]
    some = graphlet_degree_vectors(G, [33, 0, 99])
    assert list(some.index) == [0, 33] and some.to_numpy().tolist() == [_want('karate')[0], _want('karate')[33]]


def test_karate_end_to_end_sense_making():
    from graphrole_amd import RecursiveFeatureExtractor, RoleExtractor, graphlet_degree_vectors, node_measures
    G = nx.karate_club_graph()
    features = RecursiveFeatureExtractor(G).extract_features()
    np.random.seed(0)
    role_extractor = RoleExtractor(n_roles=3)
    role_extractor.extract_role_factors(features)
    M = node_measures(G, ['degree']).join(graphlet_degree_vectors(G))
    assert list(M.columns) == ['degree'] + COLUMNS and (M['degree'] == M['orbit_0']).all()
    E = role_extractor.sense_making(M)
    assert E.shape == (3, 16) and list(E.columns) == list(M.columns)
    assert np.all(E.to_numpy() >= 0)
