"""
Shortest-path distances by weight on the MI355X: kernels.weighted_distances bit-equal to tests/sssp_oracle.py
(distances, per-target sums, source eccentricities and the number of rounds) for every batch width, with source lists
that do not fill a batch, repeat a node and are shuffled; the distance matrix bit-equal to networkx's Dijkstra; unit
weights equal to the bitset BFS kernels; node_measures(distance='weight') against nx.*(..., distance / weight =
'weight') -- eccentricity and integer-weight closeness bit for bit, the rest within 1e-12 --; and the karate
sense-making run with the three weighted columns.
"""
import functools

import networkx as nx
import numpy as np
import pytest

from tests import sssp_oracle as so

pytestmark = pytest.mark.gpu


def _er_loops_isolated(directed):
    G = nx.gnm_random_graph(300, 1500 if directed else 1200, seed=7, directed=directed)
    G.add_edges_from([(3, 3), (10, 10)])
    G.add_nodes_from([900, 901])
    return so.with_weights(G, 'uniform', seed=1)


def _directed_hubs():
    """One in-hub (300 arcs into node 0) and one out-hub (300 arcs out of node 1): hub rows in both CSRs (4 lanes per
    row at this density: rows above 128 arcs)."""
    G = nx.gnm_random_graph(600, 2400, seed=12, directed=True)
    G.add_edges_from((v, 0) for v in range(2, 302))
    G.add_edges_from((1, v) for v in range(300, 600))
    return so.with_weights(G, 'uniform', seed=2)


def _disconnected():
    G = nx.disjoint_union(nx.barabasi_albert_graph(200, 2, seed=1), nx.cycle_graph(9))
    G.add_nodes_from([1000, 1001])
    return so.with_weights(G, 'uniform', seed=3)


GRAPHS = {
    'karate': nx.karate_club_graph,                              # its own integer weights
    'er300': lambda: _er_loops_isolated(False),
    'directed_er300': lambda: _er_loops_isolated(True),
    'ba300_mixed': lambda: so.with_weights(nx.barabasi_albert_graph(300, 3, seed=2), 'mixed', seed=4),
    'star': lambda: so.with_weights(nx.star_graph(1500), 'uniform', seed=5),
    'directed_hubs': _directed_hubs,
    'path600': lambda: so.with_weights(nx.path_graph(600), 'uniform', seed=6),
    'detour': so.detour_graph,
    'disconnected': _disconnected,
    'n1': lambda: nx.empty_graph(1),
    'n2': lambda: so.with_weights(nx.path_graph(2), 'uniform', seed=7),
    'n3': lambda: so.with_weights(nx.path_graph(3), 'ints', seed=8),
}
INTEGER_WEIGHTS = ('karate', 'detour', 'n1', 'n3')


@functools.lru_cache(maxsize=None)
def _case(key):
    """(G, adapter, pulled device CSR, host arrays of that CSR, 70 sources as internal rows): built once per graph."""
    from graphrole_amd import kernels as K
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    G = GRAPHS[key]()
    graph = NetworkxInterface(G)
    host, out, tr = graph._device_graph()
    pull = tr if G.is_directed() else out
    arrays = (K.to_host(pull.row_ptr).astype(np.int64), K.to_host(pull.col).astype(np.int64)[:pull.nnz],
              np.ones(pull.nnz) if pull.w is None else K.to_host(pull.w)[:pull.nnz])
    rng = np.random.default_rng(9)
    sources = rng.permutation(np.arange(host.n) if host.n >= 69 else np.repeat(np.arange(host.n), 69))[:69]
    sources = np.append(sources, sources[0])                    # 70: shuffled, a repeat, no multiple of 16
    return G, graph, pull, arrays, sources


@functools.lru_cache(maxsize=None)
def _expected(key, batch):
    _, _, _, arrays, sources = _case(key)
    return so.weighted_distances(*arrays, sources, batch)


def _run(key, batch, want_matrix=False):
    from graphrole_amd import kernels as K
    _, _, pull, _, sources = _case(key)
    n = pull.n
    reach, dsum, harmonic, far, ecc, dist, rounds = K.weighted_distances(pull, sources, batch, want_matrix)
    out = [K.to_host(t)[:n] for t in (reach, dsum, harmonic, far)] + [K.to_host(ecc)]
    return out, (K.to_host(dist) if want_matrix else None), rounds


def test_hub_graphs_have_hub_rows():
    assert _case('star')[2].n_hubs > 0
    _, out, tr = _case('directed_hubs')[1]._device_graph()
    assert out.n_hubs > 0 and tr.n_hubs > 0


@pytest.mark.parametrize('key', list(GRAPHS))
def test_kernel_is_the_oracle_bit_for_bit_at_every_width(key):
    first = None
    for batch in (16, 32, 64, 0):
        got, _, rounds = _run(key, batch)
        want = _expected(key, batch)
        for name, g, w in zip(('reach', 'dsum', 'harmonic', 'far', 'source_ecc'), got, want):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (batch, name, np.nonzero(g != w))
        assert rounds == want[6], batch                         # Jacobi rounds: as reproducible as the distances
        first = first or [g.tobytes() for g in got]
        assert [g.tobytes() for g in got] == first, batch       # the same bits across the widths
    again, _, _ = _run(key, 0)
    assert [g.tobytes() for g in again] == first                # and across two runs


@pytest.mark.parametrize('key', list(GRAPHS))
def test_distance_matrix_is_networkx_bit_for_bit(key):
    G, graph, _, _, sources = _case(key)
    host = graph._device_graph()[0]
    _, dist, _ = _run(key, 0, want_matrix=True)
    assert dist.shape == (70, host.n)
    labels = sorted(G)
    want = so.networkx_matrix(G, [labels[r] for r in np.asarray(host.perm)[sources]])
    got = host.to_label_order(dist)
    assert got.tobytes() == want.tobytes(), np.nonzero(got != want)
    assert got.tobytes() == host.to_label_order(_expected(key, 0)[5]).tobytes()


def test_path_runs_far_more_rounds_than_one_read_back():
    _, _, rounds = _run('path600', 64)
    assert rounds >= 599


def test_detour_takes_the_lighter_path_with_more_hops():
    from graphrole_amd import dijkstra_path_lengths
    D = dijkstra_path_lengths(so.detour_graph(), [0])
    assert D.loc[0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and D.attrs['rounds'] == 5


@pytest.mark.parametrize('key', ['er300', 'directed_hubs', 'star', 'disconnected', 'path600'])
def test_unit_weights_equal_the_bfs_kernels(key):
    import copy
    from graphrole_amd import kernels as K
    _, _, pull, _, sources = _case(key)
    unit = copy.copy(pull)
    unit.w = None
    n = pull.n
    reach, dsum, harmonic, far, ecc, _, _ = K.weighted_distances(unit, sources)
    b_reach, b_dsum, b_harmonic = K.distance_sums(pull, sources)
    b_ecc, e_reach, b_far, _ = K.eccentricity_pass(pull, sources)
    assert np.array_equal(K.to_host(reach)[:n], K.to_host(b_reach)[:n])
    assert np.array_equal(K.to_host(reach)[:n], K.to_host(e_reach)[:n])
    assert np.array_equal(K.to_host(dsum)[:n], K.to_host(b_dsum)[:n].astype(np.float64))
    assert np.array_equal(K.to_host(far)[:n], K.to_host(b_far)[:n].astype(np.float64))
    assert np.array_equal(K.to_host(ecc), K.to_host(b_ecc).astype(np.float64))
    np.testing.assert_allclose(K.to_host(harmonic)[:n], K.to_host(b_harmonic)[:n], rtol=so.RTOL, atol=0)


def _column(series, want: dict, exact: bool):
    assert series.dtype == np.float64 and list(series.index) == sorted(want)
    expected = np.array([want[v] for v in series.index], dtype=np.float64)
    if exact:
        assert series.to_numpy().tobytes() == expected.tobytes(), np.nonzero(series.to_numpy() != expected)
    else:
        np.testing.assert_allclose(series.to_numpy(), expected, rtol=so.RTOL, atol=0)


@pytest.mark.parametrize('key', [k for k in GRAPHS if k != 'star'])
def test_node_measures_by_weight_against_networkx(key):
    from graphrole_amd import node_measures
    G = GRAPHS[key]()
    M = node_measures(G, ['closeness_centrality', 'harmonic_centrality'], distance='weight')
    _column(M['closeness_centrality'], nx.closeness_centrality(G, distance='weight'), exact=key in INTEGER_WEIGHTS)
    _column(M['harmonic_centrality'], nx.harmonic_centrality(G, distance='weight'), exact=False)
    if G.number_of_nodes() < 100:
        got = node_measures(G, ['closeness_centrality'], distance='weight', wf_improved=False)['closeness_centrality']
        _column(got, nx.closeness_centrality(G, distance='weight', wf_improved=False), exact=key in INTEGER_WEIGHTS)
    try:
        want = nx.eccentricity(G, weight='weight')
    except nx.NetworkXError as exc:
        with pytest.raises(nx.NetworkXError, match=str(exc)):
            node_measures(G, ['eccentricity'], distance='weight')
    else:
        _column(node_measures(G, ['eccentricity'], distance='weight')['eccentricity'], want, exact=True)


def test_star_node_measures_by_weight_against_networkx_on_a_sample():
    """The undirected hub row through node_measures with every node a source: 1 501 sources, 24 batches, the last one
    partial.  networkx needs one Dijkstra per node for each of its all-node calls (about 20 s for the three), so the
    reference is networkx's own per-node form on the hub and 40 leaves: closeness_centrality(G, u=v), eccentricity(G,
    v=[...]), and harmonic centrality from single_source_dijkstra_path_length (d(s, v) = d(v, s) on an undirected
    graph), added in networkx's way."""
    from graphrole_amd import node_measures
    G = GRAPHS['star']()
    M = node_measures(G, ['closeness_centrality', 'harmonic_centrality', 'eccentricity'], distance='weight')
    assert list(M.index) == sorted(G) and all(M[c].dtype == np.float64 for c in M.columns)
    sample = [0] + sorted(np.random.default_rng(3).choice(np.arange(1, 1501), size=40, replace=False).tolist())
    got = M.loc[sample]
    ecc = nx.eccentricity(G, v=sample, weight='weight')
    assert got['eccentricity'].to_numpy().tobytes() == np.array([ecc[v] for v in sample], dtype=np.float64).tobytes()
    closeness = [nx.closeness_centrality(G, u=v, distance='weight') for v in sample]
    np.testing.assert_allclose(got['closeness_centrality'].to_numpy(), closeness, rtol=so.RTOL, atol=0)
    harmonic = []
    for v in sample:
        total = 0
        for s, d in nx.single_source_dijkstra_path_length(G, v, weight='weight').items():
            if d != 0:
                total += 1 / d
        harmonic.append(total)
    np.testing.assert_allclose(got['harmonic_centrality'].to_numpy(), harmonic, rtol=so.RTOL, atol=0)


def test_unweighted_graph_by_weight_has_the_bits_of_the_unweighted_columns():
    from graphrole_amd import node_measures
    G = nx.barabasi_albert_graph(300, 3, seed=2)
    by_weight = node_measures(G, ['closeness_centrality', 'harmonic_centrality', 'eccentricity'], distance='weight')
    hops = node_measures(G, ['closeness_centrality', 'harmonic_centrality', 'eccentricity'])
    assert by_weight['closeness_centrality'].to_numpy().tobytes() == hops['closeness_centrality'].to_numpy().tobytes()
    assert np.array_equal(by_weight['eccentricity'].to_numpy(), hops['eccentricity'].to_numpy().astype(np.float64))
    assert by_weight['eccentricity'].dtype == np.float64 and hops['eccentricity'].dtype == np.int64
    np.testing.assert_allclose(by_weight['harmonic_centrality'], hops['harmonic_centrality'], rtol=so.RTOL, atol=0)


def test_dijkstra_path_lengths_rows_are_networkx():
    from graphrole_amd import dijkstra_path_lengths
    G = GRAPHS['directed_er300']()
    sources = [299, 0, 900, 0, 150]
    D = dijkstra_path_lengths(G, sources)
    assert list(D.index) == sources and list(D.columns) == sorted(G)
    assert D.to_numpy().tobytes() == so.networkx_matrix(G, sources).tobytes()


def test_karate_end_to_end_sense_making():
    from graphrole_amd import RecursiveFeatureExtractor, RoleExtractor, node_measures
    G = nx.karate_club_graph()
    features = RecursiveFeatureExtractor(G).extract_features()
    np.random.seed(0)
    role_extractor = RoleExtractor(n_roles=3)
    role_extractor.extract_role_factors(features)
    names = ['degree', 'closeness_centrality', 'harmonic_centrality', 'eccentricity']
    M = node_measures(G, names, distance='weight')
    assert list(M.columns) == names
    _column(M['closeness_centrality'], nx.closeness_centrality(G, distance='weight'), exact=True)
    _column(M['eccentricity'], nx.eccentricity(G, weight='weight'), exact=True)
    assert not M['closeness_centrality'].equals(node_measures(G, ['closeness_centrality'])['closeness_centrality'])
    E = role_extractor.sense_making(M)
    assert list(E.columns) == names and np.all(E.to_numpy() >= 0)
    assert all(E[nm].sum() > 0 for nm in names[1:])
