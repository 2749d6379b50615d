"""
Edge betweenness centrality on the MI355X: graphrole_amd.edge_betweenness_centrality against
nx.edge_betweenness_centrality computed here, index and values, within tests/betweenness_oracle.py's one tolerance
(atol = 0, and what networkx has at exactly 0 is exactly 0), on every graph kind and option, by hops and by weight; the
whole small-graph atlas; the same bits for every batch width and run; the identity that ties the edge values to the
node betweenness that exists; and 1 M nodes against the numpy restatement.
"""
import random

import networkx as nx
import numpy as np
import pytest

from tests import atlas
from tests import edge_betweenness_oracle as eo
from tests import weighted_betweenness_oracle as wo

pytestmark = pytest.mark.gpu


def _directed_loops_isolated():
    G = nx.gnm_random_graph(300, 1200, seed=7, directed=True)
    G.add_edges_from([(3, 3), (10, 10)])
    G.add_nodes_from([900, 901])
    return G


def _directed_hubs():
    """One in-hub (1500 arcs into node 0) and another out-hub (1500 arcs out of node 1): two hub lists."""
    G = nx.gnm_random_graph(2000, 8000, seed=12, directed=True)
    G.add_edges_from((v, 0) for v in range(2, 1502))
    G.add_edges_from((1, v) for v in range(500, 2000))
    return G


def _disconnected():
    G = nx.disjoint_union(nx.barabasi_albert_graph(200, 2, seed=1), nx.cycle_graph(9))
    G.add_nodes_from([1000, 1001])
    G.add_edge(4, 4)                                            # an undirected self-loop: a key at 0.0
    return G


def _grid():
    """40 x 40 grid; with integer weights lightest paths of equal weight differ in their number of arcs."""
    return nx.convert_node_labels_to_integers(nx.grid_2d_graph(40, 40))


GRAPHS = {
    'karate': nx.karate_club_graph,
    'er300': lambda: nx.gnm_random_graph(300, 1200, seed=1),
    'ba300': lambda: nx.barabasi_albert_graph(300, 3, seed=2),
    'ba2000': lambda: nx.barabasi_albert_graph(2000, 5, seed=3),
    'star': lambda: nx.star_graph(1500),
    'directed_loops_isolated': _directed_loops_isolated,
    'directed_hubs': _directed_hubs,
    'disconnected': _disconnected,
    'strings': lambda: nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
    'path600': lambda: nx.path_graph(600),
    'n1': lambda: nx.empty_graph(1),
    'n2': lambda: nx.path_graph(2),
    'n3': lambda: nx.path_graph(3),
}

OPTIONS = [dict(normalized=False), dict(k=40, seed=3), dict(k=40, seed=random.Random(11))]


def _fresh(opts):
    opts = dict(opts)
    if isinstance(opts.get('seed'), random.Random):
        opts['seed'] = random.Random(11)
    return opts


def _check(G, series, want: dict):
    want = eo.by_sorted_ends(G, want)
    assert series.dtype == np.float64 and series.name == 'edge_betweenness_centrality'
    assert list(series.index.names) == ['u', 'v'] and list(series.index) == sorted(want)
    got, ref = series.to_numpy(), np.array([want[e] for e in series.index], dtype=np.float64)
    np.testing.assert_allclose(got, ref, rtol=eo.RTOL, atol=0)
    assert np.array_equal(got == 0, ref == 0)


def test_hub_graphs_have_hub_rows():
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    for key in ('star', 'ba2000'):
        assert NetworkxInterface(GRAPHS[key]())._device_graph()[1].n_hubs > 0, key
    _, out, tr = NetworkxInterface(_directed_hubs())._device_graph()
    assert out.n_hubs > 0 and tr.n_hubs > 0
    assert set(out.hub_rows.cpu().tolist()) != set(tr.hub_rows.cpu().tolist())


@pytest.mark.parametrize('key', list(GRAPHS))
def test_matches_networkx(key):
    from graphrole_amd import edge_betweenness_centrality
    G = GRAPHS[key]()
    _check(G, edge_betweenness_centrality(G), nx.edge_betweenness_centrality(G))


@pytest.mark.parametrize('opts', OPTIONS, ids=['raw', 'k_int', 'k_random'])
@pytest.mark.parametrize('key', ['ba2000', 'star', 'directed_loops_isolated', 'directed_hubs', 'disconnected', 'n3'])
def test_options_match_networkx(key, opts):
    from graphrole_amd import edge_betweenness_centrality
    G = GRAPHS[key]()
    if opts.get('k', 0) > G.number_of_nodes():
        opts = dict(opts, k=G.number_of_nodes())
    _check(G, edge_betweenness_centrality(G, **_fresh(opts)), nx.edge_betweenness_centrality(G, **_fresh(opts)))


WEIGHTED = {
    'ba2000/ints': lambda: wo.with_weights(GRAPHS['ba2000'](), 'ints', seed=1),
    'directed_hubs/ints': lambda: wo.with_weights(_directed_hubs(), 'ints', seed=2),
    'grid40/ints': lambda: wo.with_weights(_grid(), 'ints', seed=3),
    'ba300/uniform': lambda: wo.with_weights(GRAPHS['ba300'](), 'uniform', seed=4),
    'disconnected/ints': lambda: wo.with_weights(_disconnected(), 'ints', seed=5),
}


@pytest.mark.parametrize('key', list(WEIGHTED))
def test_weighted_matches_networkx(key):
    from graphrole_amd import edge_betweenness_centrality
    G = WEIGHTED[key]()
    opts = dict(k=40, seed=3) if G.number_of_nodes() > 1000 else dict()         # networkx's Dijkstra: seconds
    got = edge_betweenness_centrality(G, weight='weight', **opts)
    _check(G, got, nx.edge_betweenness_centrality(G, weight='weight', **opts))
    assert got.attrs['levels'] >= 2 and got.attrs['rounds'] >= got.attrs['levels']
    if key == 'grid40/ints':                                    # deeper than the hop count of the lightest paths alone
        assert set(np.unique([d['weight'] for _, _, d in G.edges(data=True)])) == {1.0, 2.0, 3.0, 4.0, 5.0}


# ------------------------------------------------------------------------------------------- the small-graph atlas
def _atlas_want(variant, relabel):
    """networkx on every atlas graph by itself, unnormalised (the raw sums do not depend on the number of nodes of the
    union), re-keyed by the labels of the union."""
    label = atlas.relabelling(relabel)
    directed = variant == 'directed'
    want = {}
    for _, first, H in atlas.small_graphs(variant):
        values = nx.edge_betweenness_centrality(H, normalized=False, weight='weight' if variant == 'weighted' else None)
        for (a, b), c in values.items():
            a, b = int(label[first + a]), int(label[first + b])
            want[(a, b) if directed or a <= b else (b, a)] = c
    return want


@pytest.mark.parametrize('relabel', atlas.RELABELLINGS)
@pytest.mark.parametrize('variant', atlas.VARIANTS)
def test_whole_atlas(variant, relabel):
    from graphrole_amd import edge_betweenness_centrality
    G = atlas.graph(variant, relabel)
    got = edge_betweenness_centrality(G, normalized=False, weight='weight' if variant == 'weighted' else None)
    want = _atlas_want(variant, relabel)
    assert len(want) == G.number_of_edges()
    _check(G, got, want)


# ------------------------------------------------------------------------------------------------------- same bits
def _batched(G, batch, weighted=False, **kw):
    """The per-arc array of the kernel with an explicit batch width."""
    from graphrole_amd import kernels as K
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    from graphrole_amd.measures import _betweenness_sources, _rescale_e_factor
    g = NetworkxInterface(G)
    host, out, tr = g._device_graph()
    sources = np.asarray(host.inv)[_betweenness_sources(g, kw.get('k'), kw.get('seed'))]
    scale = _rescale_e_factor(host.n, True, G.is_directed())
    if weighted:
        return K.to_host(K.weighted_edge_betweenness(out, tr, sources, scale, batch=batch)[0])[:out.nnz]
    return K.to_host(K.edge_betweenness(out, tr, sources, scale, batch=batch))[:out.nnz]


@pytest.mark.parametrize('key', ['ba2000', 'directed_loops_isolated', 'directed_hubs', 'star'])
def test_same_bits_for_every_batch_and_run(key):
    G = GRAPHS[key]()
    ref = _batched(G, 0)
    assert np.count_nonzero(ref) > 0
    for batch in (64, 128, 0):
        assert _batched(G, batch).tobytes() == ref.tobytes(), batch
    sampled = _batched(G, 0, k=70, seed=5)                       # 70 sources: a partial last batch
    for batch in (64, 128, 0):
        assert _batched(G, batch, k=70, seed=5).tobytes() == sampled.tobytes(), batch


@pytest.mark.parametrize('key', ['ba2000', 'directed_loops_isolated', 'directed_hubs', 'star'])
def test_weighted_same_bits_for_every_batch_and_run(key):
    G = wo.with_weights(GRAPHS[key](), 'ints', seed=6)
    ref = _batched(G, 0, True, k=70, seed=5)                     # 70 sources: partial last batches of 16, 32 and 64
    assert np.count_nonzero(ref) > 0
    for batch in (16, 32, 64, 0):
        assert _batched(G, batch, True, k=70, seed=5).tobytes() == ref.tobytes(), batch


def test_unit_weights_agree_with_the_unweighted_kernel():
    """With every weight 1 the weighted DAG is the BFS DAG: the two entry points form the same terms."""
    G = GRAPHS['ba300']()
    a = _batched(G, 64, k=70, seed=5)
    for u, v in G.edges():
        G[u][v]['weight'] = 1.0
    np.testing.assert_allclose(_batched(G, 64, True, k=70, seed=5), a, rtol=eo.RTOL, atol=0)


# ------------------------------------------------------------------------------- consistency with what exists
def test_incident_edges_sum_to_twice_the_node_betweenness():
    """Undirected, every node a source, unnormalised: the edge values at v sum to 2 * bc(v) + (reach(v) - 1) -- a path
    through v uses two of v's edges, a path that ends at v one (tests/test_edge_betweenness_cpu.py proves it on the
    oracle).  Bound: RTOL times the degree, relative to the sum."""
    from graphrole_amd import betweenness_centrality, edge_betweenness_centrality
    G = GRAPHS['ba300']()
    edges = edge_betweenness_centrality(G, normalized=False)
    node = betweenness_centrality(G, normalized=False)
    total = dict.fromkeys(G, 0.0)
    for (a, b), c in edges.items():
        total[a] += c
        total[b] += c
    assert nx.is_connected(G)
    reach = G.number_of_nodes()
    for v in G:
        assert abs(total[v] - (reach - 1) - 2 * node[v]) <= eo.RTOL * G.degree(v) * total[v], v


def test_csr_input_equals_networkx_input():
    from graphrole_amd import edge_betweenness_centrality
    from graphrole_amd.graph.csr import CSRGraph
    G = GRAPHS['ba2000']()
    src, dst = np.array(list(G.edges)).T
    a = edge_betweenness_centrality(G, k=100, seed=1)
    b = edge_betweenness_centrality(CSRGraph(G.number_of_nodes(), src, dst), k=100, seed=1)
    assert a.to_numpy().tobytes() == b.to_numpy().tobytes() and list(a.index) == list(b.index)


def test_fullsize_ba_sampled():
    from graphrole_amd import edge_betweenness_centrality, synth
    g = synth.ba_graph(1_000_000, 10, seed=0)
    got = edge_betweenness_centrality(g, k=64, seed=0)
    sources = random.Random(0).sample(list(range(g.n)), 64)
    arc = eo.arc_sums(g.row_ptr, g.col, sources)
    u, v, want = eo.edge_values(g.row_ptr, g.col, arc, False, eo.rescale_e_factor(g.n, True, False))
    assert np.count_nonzero(want) > 1_000_000
    order = np.lexsort((v, u))
    index = got.index
    assert np.array_equal(index.get_level_values(0).to_numpy(), u[order])
    assert np.array_equal(index.get_level_values(1).to_numpy(), v[order])
    np.testing.assert_allclose(got.to_numpy(), want[order], rtol=eo.RTOL, atol=0)
    assert np.array_equal(got.to_numpy() == 0, want[order] == 0)
