"""
Closeness and harmonic centrality on the MI355X: graphrole_amd.closeness_centrality bit-equal to
nx.closeness_centrality computed here, and harmonic_centrality bit-equal to the exact sum of tests/closeness_oracle.py
(and within 1e-12 of nx.harmonic_centrality), on every graph kind, hub rows included; the same bits for every source
width W, source order and run; BA 5 000 against scipy's BFS; 1 M nodes against the numpy restatement; and the karate
sense-making run with both columns.
"""
import random

import networkx as nx
import numpy as np
import pytest

from tests import closeness_oracle as co

pytestmark = pytest.mark.gpu


def _directed_loops_isolated():
    G = nx.gnm_random_graph(300, 1200, seed=7, directed=True)
    G.add_edges_from([(3, 3), (10, 10)])
    G.add_nodes_from([900, 901])
    return G


def _directed_hubs():
    """A random digraph with one in-hub (1500 arcs into node 0) and another out-hub (1500 arcs out of node 1): the
    transposed CSR has its own hub list."""
    G = nx.gnm_random_graph(2000, 8000, seed=12, directed=True)
    G.add_edges_from((v, 0) for v in range(2, 1502))
    G.add_edges_from((1, v) for v in range(500, 2000))
    return G


def _multigraph():
    return nx.MultiGraph([(0, 1), (0, 1), (1, 2), (2, 0), (2, 3), (3, 3), (3, 4), (4, 5), (5, 3), (5, 6), (5, 6)])


def _disconnected():
    G = nx.disjoint_union(nx.barabasi_albert_graph(200, 2, seed=1), nx.cycle_graph(9))
    G.add_nodes_from([1000, 1001])
    return G


GRAPHS = {
    'karate': nx.karate_club_graph,
    'er300': lambda: nx.gnm_random_graph(300, 1200, seed=1),
    'ba300': lambda: nx.barabasi_albert_graph(300, 3, seed=2),
    'ba2000': lambda: nx.barabasi_albert_graph(2000, 5, seed=3),
    'star': lambda: nx.star_graph(1500),
    'directed_loops_isolated': _directed_loops_isolated,
    'directed_hubs': _directed_hubs,
    'multigraph': _multigraph,
    'multidigraph': lambda: nx.MultiDiGraph([(0, 1), (0, 1), (1, 2), (2, 0), (2, 3), (3, 1), (4, 4)]),
    'disconnected': _disconnected,
    'strings': lambda: nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
    'path600': lambda: nx.path_graph(600),
    'n1': lambda: nx.empty_graph(1),
    'n2': lambda: nx.path_graph(2),
    'n3': lambda: nx.path_graph(3),
}


def _bits(series, want: dict):
    assert list(series.index) == sorted(want)
    assert series.dtype == np.float64
    expected = np.array([want[v] for v in series.index], dtype=np.float64)
    assert series.to_numpy().tobytes() == expected.tobytes(), np.nonzero(series.to_numpy() != expected)


def _close(series, want: dict):
    assert list(series.index) == sorted(want)
    np.testing.assert_allclose(series.to_numpy(), [want[v] for v in series.index], rtol=co.HARMONIC_RTOL, atol=0)


def test_hub_graphs_have_hub_rows():
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    for key in ('star', 'ba2000'):
        out = NetworkxInterface(GRAPHS[key]())._device_graph()[1]
        assert out.n_hubs > 0, key
    _, out, tr = NetworkxInterface(_directed_hubs())._device_graph()
    assert out.n_hubs > 0 and tr.n_hubs > 0


@pytest.mark.parametrize('key', list(GRAPHS))
def test_matches_networkx(key):
    from graphrole_amd import closeness_centrality, harmonic_centrality
    G = GRAPHS[key]()
    for wf in (True, False):
        _bits(closeness_centrality(G, wf_improved=wf), nx.closeness_centrality(G, wf_improved=wf))
    got = harmonic_centrality(G)
    _bits(got, co.harmonic(G))
    _close(got, nx.harmonic_centrality(G))


@pytest.mark.parametrize('directed', [False, True])
def test_igraph_with_loops_and_parallel_edges(directed):
    from graphrole_amd import closeness_centrality, harmonic_centrality
    from tests.test_igraph_adapter_cpu import _pair, _random_multigraph
    edges = _random_multigraph(np.random.default_rng(5 + directed), 400, 1600, directed, True, True)
    ig, G = _pair(400, edges, directed)
    _bits(closeness_centrality(ig), nx.closeness_centrality(G))
    _bits(harmonic_centrality(ig), co.harmonic(G))


def test_csr_input_equals_networkx_input():
    from graphrole_amd import closeness_centrality, harmonic_centrality
    from graphrole_amd.graph.csr import CSRGraph
    G = nx.barabasi_albert_graph(2000, 5, seed=3)
    src, dst = np.array(list(G.edges)).T
    g = CSRGraph(G.number_of_nodes(), src, dst)
    assert closeness_centrality(g).to_numpy().tobytes() == closeness_centrality(G).to_numpy().tobytes()
    assert harmonic_centrality(g).to_numpy().tobytes() == harmonic_centrality(G).to_numpy().tobytes()


def test_closeness_of_one_node():
    from graphrole_amd import closeness_centrality
    star = GRAPHS['star']()
    D = _directed_hubs()
    D.add_node(5000)                                             # isolated
    D.add_edge(7, 4000)                                          # 4000: a sink (in-arc only)
    cases = [(star, 0), (star, 17), (D, 0), (D, 1), (D, 4000), (D, 5000), (_directed_loops_isolated(), 900)]
    for G, u in cases:
        for wf in (True, False):
            got = closeness_centrality(G, u=u, wf_improved=wf)
            assert isinstance(got, float)
            assert got == nx.closeness_centrality(G, u=u, wf_improved=wf), (u, wf)


def test_harmonic_sources_and_nbunch():
    from graphrole_amd import harmonic_centrality
    G = _directed_hubs()
    rng = random.Random(4)
    sources = rng.sample(list(G), 300) + [0, 1, 0]               # duplicates count once
    nbunch = rng.sample(list(G), 40) + [-5]                      # smaller than sources: networkx transposes
    for nb, src in ((None, sources), (nbunch, None), (nbunch, sources), (list(G)[:500], list(G)[:100])):
        got = harmonic_centrality(G, nbunch=nb, sources=src)
        ref = nx.harmonic_centrality(G, nbunch=nb, sources=src)
        exact = co.harmonic(G, src)
        _bits(got, {v: exact[v] for v in ref})
        _close(got, ref)


def _words(G, words, order_seed=None):
    """kernels.distance_sums over every node with an explicit W, optionally in a shuffled source order."""
    from graphrole_amd import kernels as K
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    g = NetworkxInterface(G)
    host = g._device_graph()[0]
    s_out, s_in = g._structure_csrs()
    sources = np.arange(host.n)
    if order_seed is not None:
        sources = np.random.default_rng(order_seed).permutation(sources)
    reach, dsum, harm = K.distance_sums(s_in if G.is_directed() else s_out, sources, words=words)
    return tuple(K.to_host(t)[:host.n].tobytes() for t in (reach, dsum, harm))


@pytest.mark.parametrize('key', ['ba2000', 'directed_hubs', 'star', 'disconnected'])
def test_same_bits_for_every_width_order_and_run(key):
    G = GRAPHS[key]()
    ref = _words(G, 0)
    for words in (1, 4, 16, 0):
        assert _words(G, words) == ref, words
    assert _words(G, 0, order_seed=3) == ref
    assert _words(G, 4, order_seed=5) == ref


def test_ba5000_exact_against_scipy():
    from scipy.sparse.csgraph import shortest_path
    from graphrole_amd import closeness_centrality, harmonic_centrality
    G = nx.barabasi_albert_graph(5000, 5, seed=6)
    n = G.number_of_nodes()
    A = nx.to_scipy_sparse_array(G, nodelist=range(n), format='csr')
    reach = np.zeros(n, dtype=np.int64)
    dsum = np.zeros(n, dtype=np.int64)
    for c0 in range(0, n, 500):
        D = shortest_path(A, directed=False, unweighted=True, indices=np.arange(c0, min(c0 + 500, n)))
        hit = np.isfinite(D) & (D > 0)
        reach += hit.sum(axis=0)
        dsum += np.where(hit, D, 0).sum(axis=0).astype(np.int64)
    want = dict(zip(range(n), co.closeness_from_sums(reach, dsum, n)))
    _bits(closeness_centrality(G), want)
    _close(harmonic_centrality(G), nx.harmonic_centrality(G))


def test_fullsize_ba():
    from graphrole_amd import closeness_centrality, kernels as K, synth
    from graphrole_amd.measures import _adapter
    g = synth.ba_graph(1_000_000, 10, seed=0)
    graph = _adapter(g)
    host = graph._device_graph()[0]
    s_out, _ = graph._structure_csrs()
    inv = np.asarray(host.inv)
    rng = np.random.default_rng(0)
    rows = rng.choice(g.n, size=600, replace=False)              # label rows
    targets = np.sort(rng.choice(g.n, size=2000, replace=False))
    sym = (np.asarray(g.row_ptr, dtype=np.int64), np.asarray(g.col, dtype=np.int64))   # undirected: its own transpose
    r1, d1, h1 = co.distance_sums(*sym, rows[:512], in_adjacency=sym, targets=targets)
    r2, d2, h2 = co.distance_sums(*sym, rows[512:], in_adjacency=sym, targets=targets)
    wants = {512: (r1, d1, h1), 600: (r1 + r2, d1 + d2, [a + b for a, b in zip(h1, h2)])}   # the sums add up
    for count, (w_reach, w_dsum, w_harm) in wants.items():     # 600: one full batch of 512 and a partial one
        reach, dsum, harm = (host.to_label_order(K.to_host(t)[:g.n]) for t in
                             K.distance_sums(s_out, inv[rows[:count]]))
        assert reach.sum() > 0.9 * count * g.n                 # one component: nearly every node reached
        assert np.array_equal(reach, w_reach), count
        assert np.array_equal(dsum, w_dsum), count
        exact = np.array([co.harm_to_float(w_harm[t]) for t in targets])
        assert harm[targets].tobytes() == exact.tobytes(), count
    for u in (0, 12345, 999_999):
        D = co.bfs_levels(*sym, u)
        r, t = int((D > 0).sum()), int(D[D > 0].sum())
        assert closeness_centrality(g, u=u) == co.closeness_from_sums([r], [t], g.n)[0]


def test_karate_end_to_end_sense_making():
    from graphrole_amd import (RecursiveFeatureExtractor, RoleExtractor, closeness_centrality, harmonic_centrality,
                               node_measures)
    G = nx.karate_club_graph()
    features = RecursiveFeatureExtractor(G).extract_features()
    np.random.seed(0)
    role_extractor = RoleExtractor(n_roles=3)
    role_extractor.extract_role_factors(features)
    M = node_measures(G, ['degree', 'pagerank', 'closeness_centrality', 'harmonic_centrality'])
    assert list(M.columns) == ['degree', 'pagerank', 'closeness_centrality', 'harmonic_centrality']
    assert M['closeness_centrality'].to_numpy().tobytes() == closeness_centrality(G).to_numpy().tobytes()
    assert M['harmonic_centrality'].to_numpy().tobytes() == harmonic_centrality(G).to_numpy().tobytes()
    _bits(M['closeness_centrality'], nx.closeness_centrality(G))
    E = role_extractor.sense_making(M)
    assert list(E.columns) == list(M.columns)
    assert np.all(E.to_numpy() >= 0)
    assert E['closeness_centrality'].sum() > 0 and E['harmonic_centrality'].sum() > 0
