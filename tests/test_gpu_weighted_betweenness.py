"""
Betweenness centrality over shortest paths by weight on the MI355X: kernels.weighted_betweenness against
tests/weighted_betweenness_oracle.py within 1e-12 (atol 0: exact zeros stay exact) at every batch width, with a source
list that does not fill a batch, repeats a node and is shuffled -- the same bc bytes for every width and run, the
oracle's relaxation rounds and DAG depth --; weighted_betweenness_centrality against nx.betweenness_centrality(G,
weight='weight'); unit weights against the unweighted kernel; and the karate sense-making run with the weighted column.
The shapes are the smallest at which each mechanism runs: hub rows of both passes, a DAG 599 levels deep (dozens of
read-backs of the forward loop, 599 backward launches), a DAG deeper than the BFS, lightest paths of equal weight and
different length, unreached cells, n = 1, 2, 3.
"""
import copy
import functools

import networkx as nx
import numpy as np
import pytest

from tests import sssp_oracle as so
from tests import weighted_betweenness_oracle as wo

pytestmark = pytest.mark.gpu

HUB_FACTOR = 32                                                 # GRX_HUB_FACTOR


def _er_loops_isolated(directed):
    G = nx.gnm_random_graph(300, 1500 if directed else 1200, seed=7, directed=directed)
    G.add_edges_from([(3, 3), (10, 10)])
    G.add_nodes_from([900, 901])
    return wo.with_weights(G, 'ints', seed=1)


def _directed_hubs():
    """One in-hub (300 arcs into node 0) and one out-hub (300 arcs out of node 1): hub rows in both CSRs (4 lanes per
    row at this density: rows above 128 arcs).  The graph of tests/test_gpu_weighted_distances.py with integer
    weights."""
    G = nx.gnm_random_graph(600, 2400, seed=12, directed=True)
    G.add_edges_from((v, 0) for v in range(2, 302))
    G.add_edges_from((1, v) for v in range(300, 600))
    return wo.with_weights(G, 'ints', seed=2)


def _disconnected():
    G = nx.disjoint_union(nx.barabasi_albert_graph(200, 2, seed=1), nx.cycle_graph(9))
    G.add_nodes_from([1000, 1001])
    return wo.with_weights(G, 'ints', seed=3)


GRAPHS = {
    'karate': nx.karate_club_graph,                              # its own integer weights
    'er300': lambda: _er_loops_isolated(False),
    'directed_er300': lambda: _er_loops_isolated(True),
    'ba300_dyadic': lambda: wo.with_weights(nx.barabasi_albert_graph(300, 3, seed=2), 'dyadic', seed=4),
    'star': lambda: wo.with_weights(nx.star_graph(1500), 'ints', seed=5),
    'directed_hubs': _directed_hubs,
    'path600': lambda: wo.with_weights(nx.path_graph(600), 'ints', seed=6),
    'detour': so.detour_graph,
    'uneven_ties': wo.uneven_ties_graph,
    'disconnected': _disconnected,
    'n1': lambda: nx.empty_graph(1),
    'n2': lambda: wo.with_weights(nx.path_graph(2), 'uniform', seed=7),
    'n3': lambda: wo.with_weights(nx.path_graph(3), 'ints', seed=8),
}


def _host_arrays(K, csr):
    return (K.to_host(csr.row_ptr).astype(np.int64), K.to_host(csr.col).astype(np.int64)[:csr.nnz],
            np.ones(csr.nnz) if csr.w is None else K.to_host(csr.w)[:csr.nnz])


@functools.lru_cache(maxsize=None)
def _case(key):
    """(G, adapter, out CSR, in CSR or None, 70 sources as internal rows): built once per graph."""
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    G = GRAPHS[key]()
    graph = NetworkxInterface(G)
    host, out, tr = graph._device_graph()
    rng = np.random.default_rng(9)
    sources = rng.permutation(np.arange(host.n) if host.n >= 69 else np.repeat(np.arange(host.n), 69))[:69]
    sources = np.append(sources, sources[0])                    # 70: shuffled, a repeat, no multiple of 16
    return G, graph, out, (tr if G.is_directed() else None), sources


@functools.lru_cache(maxsize=None)
def _terms(key):
    """The oracle's passes of the 70 sources on the kernel's own CSR arrays, hub rows as the kernel sums them: computed
    once per graph, shared by every width and both `endpoints`."""
    from graphrole_amd import kernels as K
    _, _, out, tr, sources = _case(key)
    o = _host_arrays(K, out)
    i = o if tr is None else _host_arrays(K, tr)
    terms, levels, _ = wo.source_terms(o, i, sources, HUB_FACTOR * out.lanes_per_row,
                                       HUB_FACTOR * (out if tr is None else tr).lanes_per_row)
    return i, terms, levels


@functools.lru_cache(maxsize=None)
def _rounds(key, batch):
    return wo.relaxation_rounds(_terms(key)[0], _case(key)[4], batch)


def _run(key, batch, endpoints, scale):
    from graphrole_amd import kernels as K
    _, _, out, tr, sources = _case(key)
    bc, rounds, levels = K.weighted_betweenness(out, tr, sources, endpoints, scale, batch)
    return K.to_host(bc)[:out.n], rounds, levels


def test_hub_graphs_have_hub_rows():
    assert _case('star')[2].n_hubs > 0
    _, _, out, tr, _ = _case('directed_hubs')
    assert out.n_hubs > 0 and tr.n_hubs > 0


@pytest.mark.parametrize('endpoints', [False, True])
@pytest.mark.parametrize('key', list(GRAPHS))
def test_kernel_is_the_oracle_at_every_width(key, endpoints):
    _, terms, levels = _terms(key)
    n = _case(key)[2].n
    want = wo.accumulate(terms, n, endpoints, 0.25)
    first = None
    for batch in (16, 32, 64, 0):
        got, rounds, deepest = _run(key, batch, endpoints, 0.25)
        assert got.dtype == np.float64
        np.testing.assert_allclose(got, want, rtol=wo.RTOL, atol=0, err_msg=str(batch))
        assert rounds == _rounds(key, so.batch_width(batch, 70)) and deepest == levels, batch
        first = first or got.tobytes()
        assert got.tobytes() == first, batch                    # the same bits across the widths
    again, _, _ = _run(key, 0, endpoints, 0.25)
    assert again.tobytes() == first                             # and across two runs


def test_path_is_599_levels_deep():
    from graphrole_amd import kernels as K
    _, graph, out, _, _ = _case('path600')
    end = np.asarray(graph._device_graph()[0].inv)[[0]]          # the internal row of node 0, one end of the path
    _, rounds, levels = K.weighted_betweenness(out, None, end, False, 1.0, 16)
    assert levels == 599 and rounds == 600


def test_detour_is_deeper_than_its_bfs_and_uneven_ties_wait():
    from graphrole_amd import weighted_betweenness_centrality
    bc = weighted_betweenness_centrality(so.detour_graph(), normalized=False)
    assert bc.attrs['levels'] == 4 and bc.attrs['rounds'] == 5  # the BFS from node 0 is 2 levels deep
    assert bc.tolist() == [0.0, 3.0, 4.0, 3.0, 0.0]
    G = wo.uneven_ties_graph()
    got = weighted_betweenness_centrality(G, normalized=False)
    want = nx.betweenness_centrality(G, weight='weight', normalized=False)
    np.testing.assert_allclose(got.to_numpy(), [want[v] for v in got.index], rtol=wo.RTOL, atol=0)
    assert got[2] > 0                                           # node 2 carries one of the two lightest paths 0 .. 1


@functools.lru_cache(maxsize=None)
def _networkx(key, normalized):
    G = GRAPHS[key]()
    if key == 'star':                                           # all sources: 11 s of networkx; 70 sampled ones: 0.6 s
        return nx.betweenness_centrality(G, k=70, seed=3, weight='weight', normalized=normalized)
    return nx.betweenness_centrality(G, weight='weight', normalized=normalized)


@pytest.mark.parametrize('normalized', [True, False])
@pytest.mark.parametrize('key', list(GRAPHS))
def test_public_function_against_networkx(key, normalized):
    from graphrole_amd import weighted_betweenness_centrality
    G = GRAPHS[key]()
    opts = dict(k=70, seed=3) if key == 'star' else {}
    got = weighted_betweenness_centrality(G, normalized=normalized, **opts)
    want = _networkx(key, normalized)
    assert got.dtype == np.float64 and list(got.index) == sorted(G) and got.name == 'betweenness_centrality'
    np.testing.assert_allclose(got.to_numpy(), [want[v] for v in got.index], rtol=wo.RTOL, atol=0)
    assert got.attrs['levels'] >= (1 if G.number_of_edges() else 0) and got.attrs['rounds'] >= 1


@pytest.mark.parametrize('key', ['er300', 'directed_hubs', 'star', 'disconnected', 'path600'])
def test_unit_weights_equal_the_unweighted_kernel(key):
    from graphrole_amd import kernels as K
    G, graph, out, tr, sources = _case(key)
    host = graph._device_graph()[0]
    unit_out = copy.copy(out)
    unit_out.w = None
    unit_in = None
    if tr is not None:
        unit_in = copy.copy(tr)
        unit_in.w = None
    bc, _, levels = K.weighted_betweenness(unit_out, unit_in, sources, True, 0.5)
    plain = K.betweenness(out, tr, sources, True, 0.5)
    np.testing.assert_allclose(K.to_host(bc)[:out.n], K.to_host(plain)[:out.n], rtol=wo.RTOL, atol=0)
    labels = sorted(G)
    bfs = max(max(nx.single_source_shortest_path_length(G, labels[r]).values())
              for r in np.asarray(host.perm)[sources])
    assert levels == bfs


def test_weights_matter_on_karate():
    from graphrole_amd import betweenness_centrality, weighted_betweenness_centrality
    G = nx.karate_club_graph()
    assert not np.allclose(weighted_betweenness_centrality(G).to_numpy(), betweenness_centrality(G).to_numpy())


def test_karate_end_to_end_sense_making():
    from graphrole_amd import RecursiveFeatureExtractor, RoleExtractor, node_measures
    G = nx.karate_club_graph()
    features = RecursiveFeatureExtractor(G).extract_features()
    np.random.seed(0)
    role_extractor = RoleExtractor(n_roles=3)
    role_extractor.extract_role_factors(features)
    names = ['degree', 'betweenness_centrality']
    M = node_measures(G, names, betweenness_weight='weight')
    assert list(M.columns) == names and M.attrs['weighted_betweenness']['levels'] >= 2
    want = nx.betweenness_centrality(G, weight='weight')
    np.testing.assert_allclose(M['betweenness_centrality'].to_numpy(), [want[v] for v in M.index], rtol=wo.RTOL, atol=0)
    E = role_extractor.sense_making(M)
    assert list(E.columns) == names and np.all(E.to_numpy() >= 0)
    assert E['betweenness_centrality'].sum() > 0
