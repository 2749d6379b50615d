"""
Betweenness centrality on the MI355X: graphrole_amd.betweenness_centrality against nx.betweenness_centrality computed
here, within tests/betweenness_oracle.py's one tolerance, on every graph kind and option; the same bits for every batch
size and run to run; sampled sources that follow networkx's; 1 M nodes against the numpy restatement; and the karate
sense-making run with a betweenness column.
"""
import random

import networkx as nx
import numpy as np
import pytest

from tests import betweenness_oracle as bo

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
    'multidigraph': lambda: nx.MultiDiGraph([(0, 1), (0, 1), (1, 2), (2, 0), (2, 3), (3, 1)]),
    'disconnected': _disconnected,
    'strings': lambda: nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
    'path600': lambda: nx.path_graph(600),
    'n1': lambda: nx.empty_graph(1),
    'n2': lambda: nx.path_graph(2),
    'n3': lambda: nx.path_graph(3),
}

OPTIONS = [
    dict(normalized=False),
    dict(endpoints=True),
    dict(normalized=False, endpoints=True),
    dict(k=40, seed=3),
    dict(k=40, seed=random.Random(11)),
]


def _fresh(opts):
    opts = dict(opts)
    if isinstance(opts.get('seed'), random.Random):
        opts['seed'] = random.Random(11)
    return opts


def _check(series, want: dict):
    assert list(series.index) == sorted(want)
    assert series.dtype == np.float64
    np.testing.assert_allclose(series.to_numpy(), [want[v] for v in series.index], rtol=bo.RTOL, atol=0)


def test_hub_graphs_have_hub_rows():
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    for key in ('star', 'ba2000'):
        out = NetworkxInterface(GRAPHS[key]())._device_graph()[1]
        assert out.n_hubs > 0, key
    host, out, tr = NetworkxInterface(_directed_hubs())._device_graph()
    hub_out = set(out.hub_rows.cpu().tolist())
    hub_in = set(tr.hub_rows.cpu().tolist())
    row_of = {v: i for i, v in enumerate(sorted(_directed_hubs()))}
    assert np.asarray(host.inv)[row_of[1]] in hub_out and np.asarray(host.inv)[row_of[0]] in hub_in
    assert hub_out != hub_in


@pytest.mark.parametrize('directed', [False, True])
def test_igraph_with_loops_and_parallel_edges(directed):
    from graphrole_amd import betweenness_centrality
    from tests.test_igraph_adapter_cpu import _pair, _random_multigraph
    edges = _random_multigraph(np.random.default_rng(5 + directed), 400, 1600, directed, True, True)
    ig, G = _pair(400, edges, directed)
    _check(betweenness_centrality(ig), nx.betweenness_centrality(G))
    _check(betweenness_centrality(ig, k=50, seed=2, endpoints=True),
           nx.betweenness_centrality(G, k=50, seed=2, endpoints=True))


@pytest.mark.parametrize('key', list(GRAPHS))
def test_matches_networkx(key):
    from graphrole_amd import betweenness_centrality
    G = GRAPHS[key]()
    _check(betweenness_centrality(G), nx.betweenness_centrality(G))


@pytest.mark.parametrize('opts', OPTIONS, ids=['raw', 'endpoints', 'raw_endpoints', 'k_int', 'k_random'])
@pytest.mark.parametrize('key', ['ba2000', 'directed_loops_isolated', 'directed_hubs', 'disconnected', 'multigraph'])
def test_options_match_networkx(key, opts):
    from graphrole_amd import betweenness_centrality
    G = GRAPHS[key]()
    if opts.get('k', 0) > G.number_of_nodes():
        opts = dict(opts, k=G.number_of_nodes())
    _check(betweenness_centrality(G, **_fresh(opts)), nx.betweenness_centrality(G, **_fresh(opts)))


def test_csr_input_equals_networkx_input():
    from graphrole_amd import betweenness_centrality
    from graphrole_amd.graph.csr import CSRGraph
    G = nx.barabasi_albert_graph(2000, 5, seed=3)
    src, dst = np.array(list(G.edges)).T
    a = betweenness_centrality(G)
    b = betweenness_centrality(CSRGraph(G.number_of_nodes(), src, dst))
    assert a.to_numpy().tobytes() == b.to_numpy().tobytes()


def _batched(G, batch, **kw):
    """node_measures' betweenness column with an explicit batch size (graph rows in internal order)."""
    from graphrole_amd import kernels as K
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    from graphrole_amd.measures import _betweenness_sources, _rescale_factor
    g = NetworkxInterface(G)
    host, out, tr = g._device_graph()
    k = kw.get('k')
    sources = np.asarray(host.inv)[_betweenness_sources(g, k, kw.get('seed'))]
    scale = _rescale_factor(host.n, True, G.is_directed(), k, False)
    return K.to_host(K.betweenness(out, tr, sources, False, scale, batch=batch))


@pytest.mark.parametrize('key', ['ba2000', 'directed_loops_isolated', 'directed_hubs', 'star'])
def test_same_bits_for_every_batch_and_run(key):
    G = GRAPHS[key]()
    ref = _batched(G, 0)
    for batch in (64, 128, 0):
        assert _batched(G, batch).tobytes() == ref.tobytes(), batch
    sampled = _batched(G, 0, k=70, seed=5)                       # a partial last batch of 64
    assert _batched(G, 64, k=70, seed=5).tobytes() == sampled.tobytes()


def _hub_graph(directed):
    """300 nodes: a sparse random graph and a star centre whose row is a hub row (node 0 -> 1 .. 250; in the digraph
    also 40 .. 289 -> 299, so that the in-adjacency has a hub row of its own)."""
    G = nx.gnm_random_graph(300, 900, seed=21, directed=directed)
    G.add_edges_from((0, v) for v in range(1, 251))
    if directed:
        G.add_edges_from((v, 299) for v in range(40, 290))
    return G


@pytest.mark.parametrize('directed', [False, True], ids=['undirected', 'directed'])
def test_same_bits_with_endpoints_a_hub_row_and_a_repeated_source(directed):
    """The accumulation every batch width shares: `endpoints`, 70 sources (64 + 6 lanes at width 64, one partial batch at
    the wider ones), one node the source of two lanes, hub rows in both passes."""
    from networkx.algorithms.centrality import betweenness as nxb
    from graphrole_amd import kernels as K
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    G = _hub_graph(directed)
    host, out, tr = NetworkxInterface(G)._device_graph()
    assert out.n_hubs > 0 and (tr.n_hubs > 0 if directed else tr is None)
    labels = sorted(G)
    picks = np.random.default_rng(4).permutation(len(labels))[:69]
    picks = np.append(picks, picks[0])                           # 70: shuffled, a repeat
    want = dict.fromkeys(G, 0.0)
    for p in picks:                                              # networkx's own loops over this source list
        S, P, sigma, _ = nxb._single_source_shortest_path_basic(G, labels[p])
        want, _ = nxb._accumulate_endpoints(want, S, P, sigma, labels[p])
    inv = np.asarray(host.inv)
    runs = [K.to_host(K.betweenness(out, tr, inv[picks], True, 0.25, batch=batch))[:host.n]
            for batch in (64, 128, 192, 256, 0, 64)]
    for got in runs[1:]:                                         # every width, and width 64 a second time
        assert got.tobytes() == runs[0].tobytes()
    np.testing.assert_allclose(runs[0][inv], [0.25 * want[v] for v in labels], rtol=bo.RTOL, atol=0)


def test_sampled_sources_follow_networkx():
    from graphrole_amd import betweenness_centrality, kernels
    G = nx.relabel_nodes(nx.barabasi_albert_graph(1000, 3, seed=9), lambda v: f'v{v:04d}')
    seen = []
    original = kernels.betweenness

    def spy(csr_out, csr_in, sources, endpoints, scale, batch=0):
        seen.append(np.asarray(sources).copy())
        return original(csr_out, csr_in, sources, endpoints, scale, batch)

    kernels.betweenness = spy
    try:
        got = betweenness_centrality(G, k=100, seed=21)
    finally:
        kernels.betweenness = original
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    host = NetworkxInterface(G)._device_graph()[0]
    row_of = {v: i for i, v in enumerate(sorted(G))}
    expected = random.Random(21).sample(list(G.nodes()), 100)
    assert np.array_equal(seen[0], np.asarray(host.inv)[[row_of[v] for v in expected]])
    _check(got, nx.betweenness_centrality(G, k=100, seed=21))


def test_node_measures_with_pagerank():
    from graphrole_amd import node_measures
    G = nx.barabasi_albert_graph(2000, 5, seed=3)
    M = node_measures(G, ['pagerank', 'betweenness_centrality'], k=200, seed=4)
    assert list(M.columns) == ['pagerank', 'betweenness_centrality']
    _check(M['betweenness_centrality'], nx.betweenness_centrality(G, k=200, seed=4))
    pr = nx.pagerank(G)
    np.testing.assert_allclose(M['pagerank'].to_numpy(), [pr[v] for v in M.index], rtol=1e-12, atol=0)


def test_fullsize_ba_sampled():
    from graphrole_amd import betweenness_centrality, synth
    g = synth.ba_graph(1_000_000, 10, seed=0)
    got = betweenness_centrality(g, k=16, seed=0)
    sources = random.Random(0).sample(list(range(g.n)), 16)
    want = bo.betweenness_arrays(g.row_ptr, g.col, sources, False, True, False, 16)
    assert np.count_nonzero(want) > 100_000
    np.testing.assert_allclose(got.to_numpy(), want, rtol=bo.RTOL, atol=0)


def test_karate_end_to_end_sense_making():
    from graphrole_amd import RecursiveFeatureExtractor, RoleExtractor, betweenness_centrality, node_measures
    G = nx.karate_club_graph()
    features = RecursiveFeatureExtractor(G).extract_features()
    np.random.seed(0)
    role_extractor = RoleExtractor(n_roles=3)
    role_extractor.extract_role_factors(features)
    M = node_measures(G)
    M['betweenness_centrality'] = betweenness_centrality(G)
    E = role_extractor.sense_making(M)
    assert list(E.columns) == list(M.columns)
    assert np.all(E.to_numpy() >= 0)
    assert E['betweenness_centrality'].sum() > 0
    both = node_measures(G, ['degree', 'betweenness_centrality'])
    assert both['betweenness_centrality'].to_numpy().tobytes() == M['betweenness_centrality'].to_numpy().tobytes()
