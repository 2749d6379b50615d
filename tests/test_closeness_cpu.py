"""
-m "not gpu": closeness and harmonic centrality without a device.  tests/closeness_oracle.py against
nx.closeness_centrality (bit for bit) and nx.harmonic_centrality (the correctly rounded sum: bit-equal to math.fsum
of networkx's own distances) on every graph kind, then the Python layer of graphrole_amd.closeness_centrality /
harmonic_centrality / node_measures over a CPU double of kernels.distance_sums (the oracle on the double's CSR
arrays): the sources and the adjacency passed down, the argument errors, and the catalogue left as it was.  The device
numbers are pinned in tests/test_gpu_closeness.py.
"""
import types

import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import closeness_oracle as co
from tests import fake_kernels


def _directed_loops_isolated():
    G = nx.gnm_random_graph(120, 400, seed=7, directed=True)
    G.add_edges_from([(3, 3), (10, 10)])
    G.add_nodes_from([500, 501])
    return G


def _multigraph():
    return nx.MultiGraph([(0, 1), (0, 1), (1, 2), (2, 0), (2, 3), (3, 3), (3, 4), (4, 5), (5, 3), (5, 6), (5, 6)])


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
    'multidigraph': lambda: nx.MultiDiGraph([(0, 1), (0, 1), (1, 2), (2, 0), (2, 3), (3, 1), (4, 4)]),
    'disconnected': _disconnected,
    'strings': lambda: nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
    'path600': lambda: nx.path_graph(600),
    'n1': lambda: nx.empty_graph(1),
    'n2': lambda: nx.path_graph(2),
    'n3': lambda: nx.path_graph(3),
}


def _bits(got: dict, want: dict):
    keys = list(want)
    assert set(got) == set(keys)
    a = np.array([got[v] for v in keys], dtype=np.float64)
    b = np.array([want[v] for v in keys], dtype=np.float64)
    assert a.tobytes() == b.tobytes(), np.nonzero(a != b)


def _close(got: dict, want: dict):
    keys = list(want)
    assert set(got) == set(keys)
    np.testing.assert_allclose([got[v] for v in keys], [want[v] for v in keys], rtol=co.HARMONIC_RTOL, atol=0)


@pytest.mark.parametrize('wf_improved', [True, False])
@pytest.mark.parametrize('key', list(GRAPHS))
def test_oracle_closeness_is_networkx_bit_for_bit(key, wf_improved):
    G = GRAPHS[key]()
    _bits(co.closeness(G, wf_improved), nx.closeness_centrality(G, wf_improved=wf_improved))


@pytest.mark.parametrize('key', list(GRAPHS))
def test_oracle_harmonic_is_the_correctly_rounded_sum(key):
    G = GRAPHS[key]()
    got = co.harmonic(G)
    _bits(got, co.harmonic_fsum(G))
    _close(got, nx.harmonic_centrality(G))


@pytest.mark.parametrize('key', ['karate', 'directed_loops_isolated', 'multidigraph', 'disconnected'])
def test_oracle_closeness_of_one_node(key):
    G = GRAPHS[key]()
    for u in list(G)[:5] + list(G)[-2:]:
        for wf in (True, False):
            assert co.closeness_of(G, u, wf) == nx.closeness_centrality(G, u, wf_improved=wf)


def test_oracle_harmonic_with_sources():
    G = _directed_loops_isolated()
    sources = [5, 3, 3, 77, 500, 9999]
    _bits(co.harmonic(G, sources), co.harmonic_fsum(G, sources))
    _close(co.harmonic(G, sources), nx.harmonic_centrality(G, sources=sources))


def test_exact_fixed_point_terms():
    # fl(1 / d) * 2^84 is a whole number for every d < 2^31, and the largest possible sum fits 115 bits
    for d in (1, 2, 3, 7, 10, 1000, 65537, 2 ** 31 - 1):
        assert co.q(d) == int(co.q(d))
        assert co.harm_to_float(co.q(d)) == 1.0 / d
    assert ((2 ** 31 - 1) * co.q(1)).bit_length() <= 115         # at most 2^31 - 1 sources


# ------------------------------------------------------------------------------------------ Python layer, CPU double
@pytest.fixture
def cpu_backend():
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.calls = []

    def distance_sums(csr_pull, sources, words=0):
        import torch
        sources = np.asarray(sources, dtype=np.int64)
        double.calls.append(dict(sources=sources.copy(), csr=csr_pull, words=words))
        # the BFS pulls over csr_pull: it walks the arcs of csr_pull's transpose from each source
        t_ptr, t_col = co.transpose(csr_pull.row_ptr, csr_pull.col)
        reach, dsum, harm = co.distance_sums(t_ptr, t_col, sources,
                                             in_adjacency=(csr_pull.row_ptr, csr_pull.col.astype(np.int64)))
        return (torch.from_numpy(reach), torch.from_numpy(dsum),
                torch.from_numpy(np.array([co.harm_to_float(h) for h in harm], dtype=np.float64)))

    double.distance_sums = distance_sums
    backend.use(double)
    yield double
    backend.use(None)


def _internal_ids(G, nodes):
    """Internal (degree-descending) row ids of `nodes`, as the adapter maps them."""
    from graphrole_amd.graph.csr import InternalGraph
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    labels = sorted(G.nodes)
    row_of = {v: i for i, v in enumerate(labels)}
    host = InternalGraph(NetworkxInterface(G).to_csr())
    return host.inv[[row_of[v] for v in nodes]]


def _series_bits(series: pd.Series, want: dict, name: str):
    assert series.name == name and series.dtype == np.float64
    assert list(series.index) == sorted(want)
    assert series.to_numpy().tobytes() == np.array([want[v] for v in series.index], dtype=np.float64).tobytes()


def _series_close(series: pd.Series, want: dict):
    assert list(series.index) == sorted(want)
    np.testing.assert_allclose(series.to_numpy(), [want[v] for v in series.index], rtol=co.HARMONIC_RTOL, atol=0)


@pytest.mark.parametrize('key', ['karate', 'directed_loops_isolated', 'multigraph', 'multidigraph', 'strings', 'n1'])
@pytest.mark.parametrize('wf_improved', [True, False])
def test_closeness_all_nodes(cpu_backend, key, wf_improved):
    from graphrole_amd import closeness_centrality
    G = GRAPHS[key]()
    got = closeness_centrality(G, wf_improved=wf_improved)
    _series_bits(got, nx.closeness_centrality(G, wf_improved=wf_improved), 'closeness_centrality')
    (call,) = cpu_backend.calls
    assert sorted(call['sources'].tolist()) == list(range(G.number_of_nodes()))
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    _, out, tr = NetworkxInterface(G)._device_graph()
    pulled = tr if G.is_directed() else out                     # walking out-arcs = pulling over the in-adjacency
    assert np.array_equal(call['csr'].row_ptr, pulled.row_ptr) and np.array_equal(call['csr'].col, pulled.col)


@pytest.mark.parametrize('key', ['karate', 'directed_loops_isolated', 'multidigraph', 'disconnected'])
def test_closeness_of_one_node(cpu_backend, key):
    from graphrole_amd import closeness_centrality
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    G = GRAPHS[key]()
    _, out, _ = NetworkxInterface(G)._device_graph()
    for u in (list(G)[0], list(G)[-1], max(G, key=G.degree)):
        for wf in (True, False):
            got = closeness_centrality(G, u=u, wf_improved=wf)
            assert isinstance(got, float)
            assert got == nx.closeness_centrality(G, u=u, wf_improved=wf)
            call = cpu_backend.calls[-1]
            assert np.array_equal(call['sources'], _internal_ids(G, [u]))
            # reversed arcs: pulled over the out-adjacency
            assert np.array_equal(call['csr'].row_ptr, out.row_ptr) and np.array_equal(call['csr'].col, out.col)


def test_harmonic_all_nodes(cpu_backend):
    from graphrole_amd import harmonic_centrality
    G = _directed_loops_isolated()
    got = harmonic_centrality(G)
    _series_bits(got, co.harmonic(G), 'harmonic_centrality')
    _series_close(got, nx.harmonic_centrality(G))
    (call,) = cpu_backend.calls
    assert sorted(call['sources'].tolist()) == list(range(G.number_of_nodes()))


@pytest.mark.parametrize('nbunch,sources', [
    ([0, 5, 7, 500], None),                                     # nbunch smaller: networkx transposes, here it does not
    (None, [3, 3, 40, 41, 500, 12345]),                         # duplicates and a non-member
    ([1, 2, 3, 'x'], [9, 8, 7, 6, 5, 4, 3, 2, 1, 0]),
    (7, [7, 8, 9]),                                             # a single node as nbunch
    ([], [1, 2]),
])
def test_harmonic_sources_and_nbunch(cpu_backend, nbunch, sources):
    from graphrole_amd import harmonic_centrality
    G = _directed_loops_isolated()
    got = harmonic_centrality(G, nbunch=nbunch, sources=sources)
    want_all = co.harmonic(G, sources)
    ref = nx.harmonic_centrality(G, nbunch=nbunch, sources=sources)
    want = {v: want_all[v] for v in ref}
    assert got.name == 'harmonic_centrality' and got.dtype == np.float64
    assert list(got.index) == sorted(ref)
    assert got.to_numpy().tobytes() == np.array([want[v] for v in got.index], dtype=np.float64).tobytes()
    _series_close(got, ref)
    (call,) = cpu_backend.calls
    expected = set(G) if sources is None else {v for v in sources if v in G}
    assert sorted(call['sources'].tolist()) == sorted(_internal_ids(G, sorted(expected)).tolist())
    assert len(call['sources']) == len(expected)                # duplicates count once
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    _, _, tr = NetworkxInterface(G)._device_graph()
    assert np.array_equal(call['csr'].row_ptr, tr.row_ptr)      # always from `sources`, along the out-arcs


def test_argument_errors(cpu_backend):
    from graphrole_amd import closeness_centrality, harmonic_centrality
    G = nx.karate_club_graph()
    with pytest.raises(NotImplementedError, match=r"nx.closeness_centrality\(G, distance='weight'\)"):
        closeness_centrality(G, distance='weight')
    with pytest.raises(NotImplementedError, match=r"nx.closeness_centrality\(G, distance='weight'\)"):
        closeness_centrality(G, u=0, distance='weight')
    with pytest.raises(NotImplementedError, match=r"nx.harmonic_centrality\(G, distance='w'\)"):
        harmonic_centrality(G, distance='w')
    with pytest.raises(nx.NodeNotFound):
        closeness_centrality(G, u=34)
    with pytest.raises(nx.NodeNotFound):
        closeness_centrality(nx.relabel_nodes(G, str), u=3)
    with pytest.raises(nx.NetworkXError):
        harmonic_centrality(G, nbunch=3.5)
    assert cpu_backend.calls == []


@pytest.mark.parametrize('which', ['closeness', 'harmonic', 'node_measures'])
def test_directed_graph_without_in_adjacency_raises(cpu_backend, monkeypatch, which):
    from graphrole_amd import closeness_centrality, harmonic_centrality, node_measures
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    G = nx.gnm_random_graph(30, 90, seed=2, directed=True)
    monkeypatch.setattr(NetworkxInterface, '_structure_csrs', lambda self: (self._device_graph()[1], None))
    call = {'closeness': lambda: closeness_centrality(G), 'harmonic': lambda: harmonic_centrality(G),
            'node_measures': lambda: node_measures(G, ['harmonic_centrality'])}[which]
    with pytest.raises(NotImplementedError, match='in-adjacency'):
        call()
    assert cpu_backend.calls == []
    # closeness of one node walks the reversed arcs: the out-adjacency is enough
    assert closeness_centrality(G, u=3) == nx.closeness_centrality(G, u=3)


def test_catalogue_opt_in_and_one_pass(cpu_backend):
    from graphrole_amd import measures, node_measures
    assert measures.available_measures(False, False) == ['degree', 'weighted_degree', 'clustering', 'effective_size',
                                                         'pagerank', 'eigenvector']
    assert measures.available_measures(True, True) == ['degree', 'weighted_degree', 'in_degree', 'out_degree',
                                                       'pagerank']
    for name in ('closeness_centrality', 'harmonic_centrality'):
        assert name in measures.CATALOGUE and name in measures.OPT_IN
    G = _directed_loops_isolated()
    M = node_measures(G, ['weighted_degree', 'closeness_centrality', 'harmonic_centrality'], wf_improved=False)
    assert len(cpu_backend.calls) == 1                          # both columns from one pass
    assert list(M.columns) == ['weighted_degree', 'closeness_centrality', 'harmonic_centrality']
    _series_bits(M['closeness_centrality'], nx.closeness_centrality(G, wf_improved=False), 'closeness_centrality')
    _series_bits(M['harmonic_centrality'], co.harmonic(G), 'harmonic_centrality')
    node_measures(G, ['harmonic_centrality'])
    assert len(cpu_backend.calls) == 2
    assert 'closeness_centrality' not in node_measures(G, ['weighted_degree', 'harmonic_centrality']).columns


def test_csr_and_igraph_inputs(cpu_backend):
    from graphrole_amd import closeness_centrality, harmonic_centrality
    from graphrole_amd.graph.csr import CSRGraph
    from tests.test_igraph_adapter_cpu import _pair, _random_multigraph
    G = nx.barabasi_albert_graph(60, 3, seed=8)
    src, dst = np.array(list(G.edges)).T
    a = closeness_centrality(CSRGraph(60, src, dst))
    assert a.to_numpy().tobytes() == closeness_centrality(G).to_numpy().tobytes()
    for directed in (False, True):
        edges = _random_multigraph(np.random.default_rng(3 + directed), 70, 260, directed, True, True)
        ig, H = _pair(70, edges, directed)
        _series_bits(closeness_centrality(ig), nx.closeness_centrality(H), 'closeness_centrality')
        _series_bits(harmonic_centrality(ig), co.harmonic(H), 'harmonic_centrality')
