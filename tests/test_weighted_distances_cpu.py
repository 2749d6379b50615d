"""
-m "not gpu": shortest-path distances by weight without a device.  tests/sssp_oracle.py (the numpy restatement of
grx_weighted_distances: Jacobi Bellman-Ford from +inf, then the sums in source order) against networkx's Dijkstra bit
for bit, and closeness, harmonic centrality and eccentricity formed from it against nx.*(..., distance / weight =
'weight'); then the Python layer -- node_measures(distance='weight') and dijkstra_path_lengths -- over a CPU double of
kernels.weighted_distances (the oracle on the double's CSR arrays): one call for the three columns, the in-adjacency
for a directed graph, the refusals, and the unweighted table left as it was; then the C ABI's argument checks.  The
device numbers are pinned in tests/test_gpu_weighted_distances.py.
"""
import ctypes
import os
import types

import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import fake_kernels
from tests import sssp_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _directed_er():
    return nx.gnm_random_graph(300, 1500, seed=3, directed=True)


SHAPES = {
    'er300': lambda: nx.gnm_random_graph(300, 1200, seed=1),
    'directed_er300': _directed_er,
    'ba300': lambda: nx.barabasi_albert_graph(300, 3, seed=2),
    'path300': lambda: nx.path_graph(300),
}


def _graph(shape, kind):
    return so.with_weights(SHAPES[shape](), kind, seed=11)


def _bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.tobytes() == b.tobytes(), np.nonzero(a != b)


def _values(result: dict, labels):
    return np.array([result[v] for v in labels], dtype=np.float64)


# ------------------------------------------------------------------------------------------ oracle against networkx
@pytest.mark.parametrize('kind', ['uniform', 'ints', 'mixed'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_oracle_distances_are_networkx_bit_for_bit(shape, kind):
    G = _graph(shape, kind)
    labels, row_ptr, col, w = so.pulled_csr(G)
    sources = np.random.default_rng(5).choice(len(labels), size=40, replace=False)
    *_, dist, rounds = so.weighted_distances(row_ptr, col, w, sources, batch=16)
    _bits(dist, so.networkx_matrix(G, [labels[s] for s in sources]))
    assert rounds >= 3                                          # three batches, at least one round each
    *_, dist64, _ = so.weighted_distances(row_ptr, col, w, sources, batch=64)
    _bits(dist64, dist)                                         # the fixed point does not depend on the batch


@pytest.mark.parametrize('kind', ['uniform', 'ints', 'mixed'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_oracle_measures_against_networkx(shape, kind):
    G = _graph(shape, kind)
    labels, row_ptr, col, w = so.pulled_csr(G)
    n = len(labels)
    reach, dsum, harmonic, far, source_ecc, dist, _ = so.weighted_distances(row_ptr, col, w, np.arange(n))
    for wf in (True, False):
        want = _values(nx.closeness_centrality(G, distance='weight', wf_improved=wf), labels)
        got = so.closeness(reach, dsum, n, wf)
        if kind == 'ints':
            _bits(got, want)                                    # integer path lengths: every sum is exact
        else:
            np.testing.assert_allclose(got, want, rtol=so.RTOL, atol=0)
    np.testing.assert_allclose(harmonic, _values(nx.harmonic_centrality(G, distance='weight'), labels),
                               rtol=so.RTOL, atol=0)
    if kind == 'mixed':
        zero_pairs = int(((dist == 0) & ~np.eye(n, dtype=bool)).sum())
        assert zero_pairs > 0 and np.all(np.isfinite(harmonic))   # pairs at distance 0 are skipped, not divided by
    try:
        want = nx.eccentricity(G, weight='weight')
    except nx.NetworkXError:
        assert np.any(reach != n - 1)
    else:
        assert np.all(reach == n - 1)
        _bits(source_ecc, _values(want, labels))


def test_oracle_detour_and_unit_weights():
    G = so.detour_graph()
    labels, row_ptr, col, w = so.pulled_csr(G)
    *_, dist, rounds = so.weighted_distances(row_ptr, col, w, [0])
    assert dist[0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and rounds == 5      # four hops beat the direct arc
    _, row_ptr, col, w = so.pulled_csr(G, weight=None)
    assert so.weighted_distances(row_ptr, col, w, [0])[5][0].tolist() == [0.0, 1.0, 2.0, 2.0, 1.0]


def test_oracle_invalid_and_repeated_sources():
    G = _graph('ba300', 'uniform')
    labels, row_ptr, col, w = so.pulled_csr(G)
    reach, dsum, _, _, ecc, dist, _ = so.weighted_distances(row_ptr, col, w, [7, -1, 7, 300])
    assert np.all(np.isinf(dist[1])) and np.all(np.isinf(dist[3])) and ecc[1] == ecc[3] == 0.0
    _bits(dist[0], dist[2])
    assert reach[7] == 0 and reach[8] == 2 and dsum[8] == dist[0][8] + dist[0][8]


# ------------------------------------------------------------------------------------------ Python layer, CPU double
@pytest.fixture
def cpu_backend():
    import torch
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.calls = []

    def weighted_distances(csr_pull, sources, batch=0, want_matrix=False):
        sources = np.asarray(sources, dtype=np.int64)
        double.calls.append(dict(sources=sources.copy(), csr=csr_pull, batch=batch, want_matrix=want_matrix))
        w = np.ones(len(csr_pull.col)) if csr_pull.w is None else csr_pull.w
        reach, dsum, harmonic, far, ecc, dist, rounds = so.weighted_distances(
            csr_pull.row_ptr, csr_pull.col.astype(np.int64), w, sources, batch)
        return (torch.from_numpy(reach), torch.from_numpy(dsum), torch.from_numpy(harmonic), torch.from_numpy(far),
                torch.from_numpy(ecc), torch.from_numpy(dist) if want_matrix else None, rounds)

    double.weighted_distances = weighted_distances
    backend.use(double)
    yield double
    backend.use(None)


def _column(series: pd.Series, want: dict, exact: bool):
    assert series.dtype == np.float64 and list(series.index) == sorted(want)
    if exact:
        _bits(series.to_numpy(), _values(want, series.index))
    else:
        np.testing.assert_allclose(series.to_numpy(), _values(want, series.index), rtol=so.RTOL, atol=0)


THREE = ['closeness_centrality', 'harmonic_centrality', 'eccentricity']


@pytest.mark.parametrize('directed', [False, True])
def test_three_columns_from_one_call(cpu_backend, directed):
    from graphrole_amd import node_measures
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    G = nx.gnm_random_graph(60, 600, seed=4, directed=directed)
    assert nx.is_strongly_connected(G) if directed else nx.is_connected(G)
    G = so.with_weights(G, 'ints', seed=2)
    M = node_measures(G, ['weighted_degree'] + THREE, distance='weight')
    assert list(M.columns) == ['weighted_degree'] + THREE
    (call,) = cpu_backend.calls
    assert sorted(call['sources'].tolist()) == list(range(60)) and not call['want_matrix']
    _, out, tr = NetworkxInterface(G)._device_graph()
    pulled = tr if directed else out                            # walking out-arcs = pulling over the in-adjacency
    assert np.array_equal(call['csr'].row_ptr, pulled.row_ptr) and np.array_equal(call['csr'].col, pulled.col)
    assert np.array_equal(call['csr'].w, pulled.w)
    _column(M['closeness_centrality'], nx.closeness_centrality(G, distance='weight'), exact=True)
    _column(M['harmonic_centrality'], nx.harmonic_centrality(G, distance='weight'), exact=False)
    _column(M['eccentricity'], nx.eccentricity(G, weight='weight'), exact=True)
    assert M['weighted_degree'].dtype == np.int64
    _column(node_measures(G, ['closeness_centrality'], distance='weight', wf_improved=False)['closeness_centrality'],
            nx.closeness_centrality(G, distance='weight', wf_improved=False), exact=True)


def test_float_weights_missing_weight_and_string_labels(cpu_backend):
    from graphrole_amd import node_measures
    G = so.with_weights(nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'), 'uniform', seed=8)
    del G['node-00']['node-01']['weight']                       # a missing weight counts 1
    M = node_measures(G, THREE, distance='weight')
    _column(M['closeness_centrality'], nx.closeness_centrality(G, distance='weight'), exact=False)
    _column(M['harmonic_centrality'], nx.harmonic_centrality(G, distance='weight'), exact=False)
    _column(M['eccentricity'], nx.eccentricity(G, weight='weight'), exact=True)


def test_distance_none_is_todays_table(cpu_backend):
    """Without `distance` the three columns come from the unweighted kernels as before, weights or not."""
    from graphrole_amd import node_measures
    from tests import closeness_oracle as co
    seen = []

    def distance_sums(csr_pull, sources, words=0):
        import torch
        seen.append(len(sources))
        t_ptr, t_col = co.transpose(csr_pull.row_ptr, csr_pull.col)
        reach, dsum, harm = co.distance_sums(t_ptr, t_col, np.asarray(sources, dtype=np.int64),
                                             in_adjacency=(csr_pull.row_ptr, csr_pull.col.astype(np.int64)))
        return (torch.from_numpy(reach), torch.from_numpy(dsum),
                torch.from_numpy(np.array([co.harm_to_float(h) for h in harm], dtype=np.float64)))

    cpu_backend.distance_sums = distance_sums
    G = so.with_weights(nx.karate_club_graph(), 'uniform', seed=1)
    M = node_measures(G, ['closeness_centrality', 'harmonic_centrality'])
    assert seen == [34] and cpu_backend.calls == []
    _column(M['closeness_centrality'], nx.closeness_centrality(G), exact=True)
    assert M.equals(node_measures(G, ['closeness_centrality', 'harmonic_centrality'], distance=None))
    # `distance` touches the three distance columns only
    assert node_measures(G, ['weighted_degree'], distance='weight').equals(node_measures(G, ['weighted_degree']))
    assert cpu_backend.calls == []


def test_unweighted_graph_by_weight_equals_hop_counts(cpu_backend):
    from graphrole_amd import node_measures
    G = nx.karate_club_graph()
    for u, v in G.edges():
        del G[u][v]['weight']
    M = node_measures(G, THREE, distance='weight')
    _column(M['closeness_centrality'], nx.closeness_centrality(G), exact=True)
    _column(M['eccentricity'], nx.eccentricity(G), exact=True)
    assert M['eccentricity'].dtype == np.float64                # float by weight, whatever the weights are


@pytest.mark.parametrize('directed', [False, True])
def test_eccentricity_of_a_disconnected_graph_raises_networkx_messages(cpu_backend, directed):
    from graphrole_amd import node_measures
    G = nx.path_graph(5, create_using=nx.DiGraph if directed else nx.Graph)
    if not directed:
        G.add_node(9)
    G = so.with_weights(G, 'uniform')
    message = ('Found infinite path length because the digraph is not strongly connected' if directed
               else 'Found infinite path length because the graph is not connected')
    with pytest.raises(nx.NetworkXError, match=message):
        nx.eccentricity(G, weight='weight')
    with pytest.raises(nx.NetworkXError, match=message):
        node_measures(G, ['eccentricity'], distance='weight')
    # the sums are defined all the same
    _column(node_measures(G, ['harmonic_centrality'], distance='weight')['harmonic_centrality'],
            nx.harmonic_centrality(G, distance='weight'), exact=False)


def test_refusals_before_any_device_work(cpu_backend):
    from graphrole_amd import dijkstra_path_lengths, node_measures
    from graphrole_amd.graph.csr import CSRGraph
    G = nx.karate_club_graph()
    for bad in (-1.0, float('nan'), float('inf')):
        H = G.copy()
        H[0][1]['weight'] = bad
        with pytest.raises(ValueError, match='finite and >= 0'):
            node_measures(H, ['closeness_centrality'], distance='weight')
        with pytest.raises(ValueError, match='finite and >= 0'):
            dijkstra_path_lengths(H)
        node_measures(H, ['weighted_degree'], distance='weight')         # no distance column: the weights are not looked at
    with pytest.raises(ValueError, match='finite and >= 0'):
        node_measures(CSRGraph(3, np.array([0, 1]), np.array([1, 2]), np.array([1.0, -2.0])), ['eccentricity'],
                      distance='weight')
    for multi in (nx.MultiGraph([(0, 1), (0, 1), (1, 2)]), nx.MultiDiGraph([(0, 1), (1, 0)])):
        with pytest.raises(NotImplementedError, match='parallel edges'):
            node_measures(multi, ['harmonic_centrality'], distance='weight')
        with pytest.raises(NotImplementedError, match='parallel edges'):
            dijkstra_path_lengths(multi)
    for bad in ('cost', 1, lambda u, v, d: 1):
        with pytest.raises(NotImplementedError, match="distance='weight'"):
            node_measures(G, ['closeness_centrality'], distance=bad)
    with pytest.raises(NotImplementedError):
        dijkstra_path_lengths(G, weight='cost')
    with pytest.raises(nx.NodeNotFound):
        dijkstra_path_lengths(G, sources=[0, 99])
    assert cpu_backend.calls == []


def test_igraph_parallel_edges_are_refused(cpu_backend):
    from graphrole_amd import node_measures
    from tests.test_igraph_adapter_cpu import _pair, _random_multigraph
    edges = _random_multigraph(np.random.default_rng(3), 40, 160, False, True, True)
    ig, _ = _pair(40, edges, False)
    with pytest.raises(NotImplementedError, match='parallel edges'):
        node_measures(ig, ['closeness_centrality'], distance='weight')
    assert cpu_backend.calls == []


def test_pinned_refusals_name_the_way_in(cpu_backend):
    from graphrole_amd import closeness_centrality, eccentricity, harmonic_centrality
    G = nx.karate_club_graph()
    for call, pattern in ((lambda: closeness_centrality(G, distance='weight'),
                           r"nx.closeness_centrality\(G, distance='weight'\).*node_measures\(G, \['closeness_centrality'\], "
                           r"distance='weight'\)"),
                          (lambda: harmonic_centrality(G, distance='w'),
                           r"nx.harmonic_centrality\(G, distance='w'\).*node_measures\(G, \['harmonic_centrality'\]"),
                          (lambda: eccentricity(G, weight='weight'),
                           r"nx.eccentricity\(G, weight='weight'\).*node_measures\(G, \['eccentricity'\]")):
        with pytest.raises(NotImplementedError, match=pattern) as info:
            call()
        assert 'use networkx' not in str(info.value)
    assert cpu_backend.calls == []


@pytest.mark.parametrize('directed', [False, True])
def test_dijkstra_path_lengths(cpu_backend, directed):
    from graphrole_amd import dijkstra_path_lengths
    G = nx.gnm_random_graph(50, 120, seed=6, directed=directed)
    G.add_nodes_from([70, 71])                                  # unreachable
    G = so.with_weights(G, 'mixed', seed=3)
    sources = [49, 0, 70, 0, 13]                                # given order, a repeat, an isolated node
    D = dijkstra_path_lengths(G, sources)
    assert D.shape == (5, 52) and list(D.index) == sources and list(D.columns) == sorted(G)
    assert all(dt == np.float64 for dt in D.dtypes)
    _bits(D.to_numpy(), so.networkx_matrix(G, sources))
    assert np.isinf(D.loc[70]).sum() == 51 and D.loc[70, 70] == 0.0
    (call,) = cpu_backend.calls
    assert call['want_matrix'] and len(call['sources']) == 5
    everything = dijkstra_path_lengths(G)
    assert list(everything.index) == sorted(G) == list(everything.columns)
    _bits(everything.to_numpy(), so.networkx_matrix(G, sorted(G)))
    assert everything.attrs['rounds'] >= 1
    hops = dijkstra_path_lengths(G, [0, 13], weight=None)
    _bits(hops.to_numpy(), so.networkx_matrix(G, [0, 13], weight=None))
    assert cpu_backend.calls[-1]['csr'].w is None


def test_dijkstra_path_lengths_refuses_a_result_above_2_gib(cpu_backend, monkeypatch):
    from graphrole_amd import dijkstra_path_lengths, measures
    monkeypatch.setattr(measures, '_PATH_LENGTHS_MAX_BYTES', 8 * 34 * 10)
    G = nx.karate_club_graph()
    assert dijkstra_path_lengths(G, list(range(10))).shape == (10, 34)
    with pytest.raises(ValueError, match='2 GiB'):
        dijkstra_path_lengths(G, list(range(11)))
    assert len(cpu_backend.calls) == 1


def test_public_names():
    import graphrole_amd
    from graphrole_amd import kernels, measures
    assert graphrole_amd.dijkstra_path_lengths is measures.dijkstra_path_lengths
    assert callable(kernels.weighted_distances)
    assert list(measures.CATALOGUE)[-1] == 'eccentricity' and len(measures.CATALOGUE) == 16


# ---------------------------------------------------------------------------------------------------------- ABI
def test_ctypes_signatures_and_header():
    from graphrole_amd import _lib
    assert len(_lib._SIGNATURES['grx_weighted_distances'][1]) == 21
    assert len(_lib._SIGNATURES['grx_weighted_distances_workspace_bytes'][1]) == 3
    header = open(os.path.join(ROOT, 'include', 'grx.h')).read()
    assert 'grx_weighted_distances(' in header and 'grx_weighted_distances_workspace_bytes(' in header
    assert 'finite and >= 0' in header                          # the contract on the weights is documented
    assert '#define GRX_VERSION 1100' in header


def test_argument_validation_needs_no_device():
    """GRX_REQUIRE runs before any HIP call: batch, n range, source count, ld_dist, workspace, null pointers."""
    from graphrole_amd import _lib
    lib = _lib.load()
    size = lib.grx_weighted_distances_workspace_bytes
    need = size(10, 16, 70)
    assert need >= 2 * 8 * 16 * 10 + 4 * 10
    assert size(10, 64, 70) >= 2 * 8 * 64 * 10 + 4 * 10 > size(10, 32, 70) > need
    assert size(10, 0, 70) == size(10, 64, 70)                  # no wider than the source list rounded up ...
    assert size(10, 0, 17) == size(10, 32, 17) and size(10, 0, 3) == need    # ... and never below 16
    assert size(1 << 22, 0, 1 << 22) == size(1 << 22, 32, 1)    # 64 lanes would need 4 GiB + the stamps
    p = ctypes.c_void_p(4096)                                   # never dereferenced: every call fails validation

    def call(n=10, row_ptr=p, col=p, w=None, hubs=None, n_hubs=0, lanes=8, sources=p, n_sources=70, batch=16,
             reach=p, dsum=p, harmonic=p, far=p, ecc=p, dist=None, ld_dist=0, rounds=None, ws=p, ws_bytes=need):
        return lib.grx_weighted_distances(n, row_ptr, col, w, hubs, n_hubs, lanes, sources, n_sources, batch, reach,
                                          dsum, harmonic, far, ecc, dist, ld_dist, rounds, ws, ws_bytes, None)

    for bad in (dict(batch=8), dict(batch=48), dict(batch=128), dict(batch=-16), dict(n=1 << 31), dict(n=0),
                dict(n_sources=-1), dict(dist=p, ld_dist=9), dict(dist=p, ld_dist=0), dict(ws_bytes=need - 1),
                dict(batch=64), dict(batch=0), dict(row_ptr=None), dict(col=None), dict(reach=None), dict(dsum=None),
                dict(harmonic=None), dict(far=None), dict(ecc=None), dict(sources=None), dict(ws=None),
                dict(lanes=0), dict(n_hubs=2), dict(n_hubs=-1)):
        assert call(**bad) == -1, bad
        assert b'grx_weighted_distances' in lib.grx_last_error(), bad
