"""
-m "not gpu": betweenness centrality without a device.  tests/betweenness_oracle.py against
nx.betweenness_centrality on every graph kind and option, then the Python layer of
graphrole_amd.betweenness_centrality / node_measures over a CPU double of kernels.betweenness (the oracle on the
double's CSR arrays): the sources passed down and their order, the scale, the argument errors, and the catalogue
left as it was.  The device numbers are pinned in tests/test_gpu_betweenness.py.
"""
import random
import types

import networkx as nx
import numpy as np
import pytest

from tests import betweenness_oracle as bo
from tests import fake_kernels


def _directed_loops_isolated():
    G = nx.gnm_random_graph(120, 400, seed=7, directed=True)
    G.add_edges_from([(3, 3), (10, 10)])
    G.add_nodes_from([500, 501])
    return G


def _multigraph():
    G = nx.MultiGraph([(0, 1), (0, 1), (1, 2), (2, 0), (2, 3), (3, 3), (3, 4), (4, 5), (5, 3), (5, 6), (5, 6)])
    return G


def _disconnected():
    G = nx.disjoint_union(nx.barabasi_albert_graph(60, 2, seed=1), nx.cycle_graph(9))
    G.add_nodes_from([1000, 1001])
    return G


GRAPHS = {
    'karate': nx.karate_club_graph,
    'er300': lambda: nx.gnm_random_graph(300, 1200, seed=1),
    'ba300': lambda: nx.barabasi_albert_graph(300, 3, seed=2),
    'directed_loops_isolated': _directed_loops_isolated,
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
    dict(),
    dict(normalized=False),
    dict(endpoints=True),
    dict(normalized=False, endpoints=True),
    dict(k=7, seed=3),
    dict(k=7, seed=random.Random(11)),
    dict(k=5, seed=4, endpoints=True, normalized=False),
]


def _close(got: dict, want: dict):
    keys = list(want)
    assert set(got) == set(keys)
    np.testing.assert_allclose([got[v] for v in keys], [want[v] for v in keys], rtol=bo.RTOL, atol=0)


def _fresh(opts):
    opts = dict(opts)
    if isinstance(opts.get('seed'), random.Random):                # the same stream for both sides
        opts['seed'] = random.Random(11)
    return opts


@pytest.mark.parametrize('key', list(GRAPHS))
def test_oracle_matches_networkx(key):
    G = GRAPHS[key]()
    _close(bo.betweenness(G), nx.betweenness_centrality(G))


@pytest.mark.parametrize('opts', OPTIONS, ids=[str(i) for i in range(len(OPTIONS))])
@pytest.mark.parametrize('key', ['karate', 'directed_loops_isolated', 'disconnected', 'n2'])
def test_oracle_options_match_networkx(key, opts):
    G = GRAPHS[key]()
    if opts.get('k', 0) > G.number_of_nodes():
        opts = dict(opts, k=G.number_of_nodes())
    _close(bo.betweenness(G, **_fresh(opts)), nx.betweenness_centrality(G, **_fresh(opts)))


# ------------------------------------------------------------------------------------------ Python layer, CPU double
@pytest.fixture
def cpu_backend():
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.calls = []

    def betweenness(csr_out, csr_in, sources, endpoints, scale, batch=0):
        sources = np.asarray(sources, dtype=np.int64)
        double.calls.append(dict(sources=sources.copy(), endpoints=endpoints, scale=scale, directed=csr_in is not None))
        # directed, not normalized: _rescale leaves the sums alone; the kernel's scale is applied below
        bc = bo.betweenness_arrays(csr_out.row_ptr, csr_out.col, sources, True, normalized=False, endpoints=endpoints)
        import torch
        return torch.from_numpy(bc * scale)

    double.betweenness = betweenness
    backend.use(double)
    yield double
    backend.use(None)


def _internal_ids(G, nodes):
    """Internal (degree-descending) row ids of `nodes`, as the adapter maps them."""
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    from graphrole_amd.graph.csr import InternalGraph
    labels = sorted(G.nodes)
    row_of = {v: i for i, v in enumerate(labels)}
    host = InternalGraph(NetworkxInterface(G).to_csr())
    return host.inv[[row_of[v] for v in nodes]]


def test_sources_and_order_all_nodes(cpu_backend):
    from graphrole_amd import betweenness_centrality
    G = nx.gnm_random_graph(50, 150, seed=3)
    H = nx.Graph()
    H.add_nodes_from(random.Random(0).sample(list(G), 50))       # graph order differs from label order
    H.add_edges_from(G.edges)
    bc = betweenness_centrality(H)
    call = cpu_backend.calls[-1]
    assert np.array_equal(call['sources'], _internal_ids(H, list(H)))
    assert call['scale'] == 1 / (49 * 48)
    assert list(bc.index) == sorted(H.nodes) and bc.dtype == np.float64 and bc.name == 'betweenness_centrality'
    ref = nx.betweenness_centrality(H)
    np.testing.assert_allclose(bc.to_numpy(), [ref[v] for v in bc.index], rtol=bo.RTOL, atol=0)


@pytest.mark.parametrize('seed_kind', ['int', 'random', 'global'])
def test_sampled_sources_follow_networkx(cpu_backend, seed_kind):
    from graphrole_amd import betweenness_centrality
    G = nx.relabel_nodes(nx.barabasi_albert_graph(80, 2, seed=5), lambda v: f'v{v}')
    if seed_kind == 'int':
        ours, theirs = 17, 17
    elif seed_kind == 'random':
        ours, theirs = random.Random(17), random.Random(17)
    else:
        ours = theirs = None
        random.seed(17)
    bc = betweenness_centrality(G, k=9, seed=ours)
    if seed_kind == 'global':
        random.seed(17)
    rng = random.Random(theirs) if seed_kind == 'int' else (theirs if seed_kind == 'random' else random._inst)
    expected = rng.sample(list(G.nodes()), 9)
    call = cpu_backend.calls[-1]
    assert np.array_equal(call['sources'], _internal_ids(G, expected))
    assert call['scale'] == 1 / (79 * 78) * 80 / 9
    if seed_kind == 'global':
        random.seed(17)
    ref = nx.betweenness_centrality(G, k=9, seed=17 if seed_kind == 'int' else
                                    (random.Random(17) if seed_kind == 'random' else None))
    np.testing.assert_allclose(bc.to_numpy(), [ref[v] for v in bc.index], rtol=bo.RTOL, atol=0)


@pytest.mark.parametrize('n,directed,normalized,endpoints,k', [
    (30, False, True, False, None), (30, True, True, False, None), (30, False, False, False, None),
    (30, True, False, False, None), (30, False, True, True, None), (30, True, False, True, 4),
    (2, False, True, False, None), (1, False, True, True, None), (2, False, True, True, None),
    (30, False, True, False, 6),
])
def test_scale_is_rescale(cpu_backend, n, directed, normalized, endpoints, k):
    from graphrole_amd import betweenness_centrality
    G = nx.gnm_random_graph(n, 2 * n, seed=1, directed=directed)
    betweenness_centrality(G, k=k, normalized=normalized, endpoints=endpoints, seed=0)
    want = bo.rescale_factor(n, normalized, directed, k, endpoints)
    call = cpu_backend.calls[-1]
    assert call['scale'] == (1.0 if want is None else want)
    assert call['endpoints'] == endpoints and call['directed'] == directed


def test_argument_errors(cpu_backend):
    from graphrole_amd import betweenness_centrality, node_measures
    G = nx.karate_club_graph()
    with pytest.raises(NotImplementedError, match=r"nx.betweenness_centrality\(G, weight='weight'\)"):
        betweenness_centrality(G, weight='weight')
    for k in (0, 35, -1, 2.5):
        with pytest.raises(ValueError, match='k must be'):
            betweenness_centrality(G, k=k)
    with pytest.raises(TypeError, match='seed'):
        betweenness_centrality(G, k=3, seed=np.random.RandomState(0))
    with pytest.raises(ValueError, match='k must be'):
        node_measures(G, ['betweenness_centrality'], k=0)
    assert cpu_backend.calls == []


def test_catalogue_unchanged_and_opt_in(cpu_backend):
    from graphrole_amd import measures, node_measures
    assert measures.available_measures(False, False) == ['degree', 'weighted_degree', 'clustering', 'effective_size',
                                                         'pagerank', 'eigenvector']
    assert measures.available_measures(True, True) == ['degree', 'weighted_degree', 'in_degree', 'out_degree',
                                                       'pagerank']
    assert 'betweenness_centrality' in measures.CATALOGUE
    with pytest.raises(ValueError, match='catalogue'):
        node_measures(nx.karate_club_graph(), ['betweenness'])
    G = nx.karate_club_graph()
    M = node_measures(G, ['weighted_degree', 'betweenness_centrality'], k=10, seed=1, endpoints=True)
    assert list(M.columns) == ['weighted_degree', 'betweenness_centrality']
    ref = nx.betweenness_centrality(G, k=10, seed=1, endpoints=True)
    np.testing.assert_allclose(M['betweenness_centrality'].to_numpy(), [ref[v] for v in M.index], rtol=bo.RTOL,
                               atol=0)


def test_csr_and_multigraph_inputs(cpu_backend):
    from graphrole_amd import betweenness_centrality
    from graphrole_amd.graph.csr import CSRGraph
    G = nx.barabasi_albert_graph(60, 3, seed=8)
    src, dst = np.array(list(G.edges)).T
    a = betweenness_centrality(CSRGraph(60, src, dst))
    b = betweenness_centrality(G)
    np.testing.assert_allclose(a.to_numpy(), b.to_numpy(), rtol=bo.RTOL, atol=0)
    MG = _multigraph()
    ref = nx.betweenness_centrality(MG)
    got = betweenness_centrality(MG)
    np.testing.assert_allclose(got.to_numpy(), [ref[v] for v in got.index], rtol=bo.RTOL, atol=0)


@pytest.mark.parametrize('directed', [False, True])
def test_igraph_with_loops_and_parallel_edges(cpu_backend, directed):
    # the device graph of such an igraph graph is the neighbour multiset (one column per parallel edge, no transposed
    # CSR); betweenness must walk the distinct arcs, out and in, as networkx's G[v]
    from graphrole_amd import betweenness_centrality
    from tests.test_igraph_adapter_cpu import _pair, _random_multigraph
    edges = _random_multigraph(np.random.default_rng(3 + directed), 70, 260, directed, True, True)
    ig, G = _pair(70, edges, directed)
    got = betweenness_centrality(ig)
    call = cpu_backend.calls[-1]
    assert call['directed'] == directed
    ref = nx.betweenness_centrality(G)
    np.testing.assert_allclose(got.to_numpy(), [ref[v] for v in got.index], rtol=bo.RTOL, atol=0)


def test_directed_graph_without_in_adjacency_raises(cpu_backend, monkeypatch):
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    from graphrole_amd.measures import measures_of
    g = NetworkxInterface(nx.gnm_random_graph(30, 90, seed=2, directed=True))
    monkeypatch.setattr(NetworkxInterface, '_structure_csrs', lambda self: (self._device_graph()[1], None))
    with pytest.raises(NotImplementedError, match='in-adjacency'):
        measures_of(g, ['betweenness_centrality'])
    assert cpu_backend.calls == []
