"""
RolX sense making on the MI355X: graphrole_amd.node_measures against networkx 3.4.2 computed here (degrees,
clustering and effective size bit-equal; PageRank and eigenvector centrality to 1e-12 relative with the iteration
count of tests/sense_oracle.py's restatement of networkx's loops; at 1 M nodes the eigenvector against the long-double
oracle of tests/measures_oracle.py), and RoleExtractor.sense_making end to end.
"""
import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import measures_oracle, sense_oracle
from tests.test_gpu_closeness import _directed_hubs, _disconnected

pytestmark = pytest.mark.gpu


def _weighted(seed=5):
    G = nx.gnm_random_graph(300, 1200, seed=seed)
    rng = np.random.default_rng(seed)
    for u, v in G.edges:
        if rng.random() < 0.8:                                  # partial weights: the rest weigh 1
            G[u][v]['weight'] = float(rng.uniform(0.1, 4.0))
    return G


def _directed_weighted(seed=6):
    G = nx.gnm_random_graph(300, 1500, seed=seed, directed=True)
    rng = np.random.default_rng(seed)
    for u, v in G.edges:
        G[u][v]['weight'] = float(rng.uniform(0.1, 4.0))
    G.add_edge(4, 4, weight=2.0)
    G.add_nodes_from([900, 901])                                # isolated: dangling for PageRank
    return G


def _loops_isolated():
    G = nx.gnm_random_graph(150, 400, seed=4)
    G.add_edge(3, 3)
    G.add_edge(9, 9)
    G.add_edge(500, 500)                                        # only neighbour is itself: effective size NaN here
    G.add_nodes_from([1000, 1001])
    return G


def _strings():
    G = nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}')
    for u, v in G.edges:
        G[u][v].pop('weight', None)
    return G


def _multigraph():
    G = nx.MultiGraph()
    G.add_edges_from([(0, 1), (0, 1), (1, 2), (2, 0), (2, 3), (3, 3), (3, 4), (4, 5), (5, 3)])
    G.add_edge(1, 2, weight=2.5)
    return G


def _multidigraph():
    G = nx.MultiDiGraph()
    G.add_edges_from([(0, 1), (0, 1), (1, 0), (1, 2), (2, 0), (2, 3), (3, 3), (3, 3), (3, 4), (4, 5), (5, 3), (5, 3),
                      (5, 3), (6, 5)])
    G.add_edge(1, 2, weight=2.5)
    G.add_node(7)
    return G


def _directed_hubs_weighted(seed=12):
    G = _directed_hubs()                                        # in-hub 0, out-hub 1 (tests/test_gpu_closeness.py)
    rng = np.random.default_rng(seed)
    for u, v in G.edges:
        G[u][v]['weight'] = float(rng.uniform(0.1, 4.0))
    return G


GRAPHS = {
    'karate': lambda: nx.karate_club_graph(),
    'er300': lambda: nx.gnm_random_graph(300, 1500, seed=1),
    'ba300': lambda: nx.barabasi_albert_graph(300, 3, seed=2),
    'ba2000': lambda: nx.barabasi_albert_graph(2000, 5, seed=3),
    'weighted': _weighted,
    'directed_weighted': _directed_weighted,
    'loops_isolated': _loops_isolated,
    'strings': _strings,
    'multigraph': _multigraph,
    'multidigraph': _multidigraph,
    'star1500': lambda: nx.star_graph(1500),
    'directed_hubs_weighted': _directed_hubs_weighted,
    'disconnected': _disconnected,
}

# networkx's default max_iter = 100 unless the graph needs more: the eigenvector iteration of a star contracts by
# (sqrt(n) - 1) / (sqrt(n) + 1) per step
MAX_ITER = {'star1500': 1000}


def _series(d, index):
    return np.array([d[k] for k in index], dtype=np.float64)


def _expected(G, name, index, max_iter=100):
    if name == 'degree':
        return _series(dict(G.degree()), index), None
    if name == 'weighted_degree':
        return _series(dict(G.degree(weight='weight')), index), None
    if name == 'in_degree':
        return _series(dict(G.in_degree()), index), None
    if name == 'out_degree':
        return _series(dict(G.out_degree()), index), None
    if name == 'clustering':
        return _series(nx.clustering(G), index), None
    if name == 'effective_size':
        own = {v for v in G if set(G[v]) == {v}}               # networkx raises ZeroDivisionError on these
        H = G.copy()
        H.remove_nodes_from(own)
        d = nx.effective_size(H)
        d.update({v: np.nan for v in own})
        return _series(d, index), None
    if name == 'pagerank':
        x, it = sense_oracle.pagerank(G, max_iter=max_iter)
        assert np.allclose(_series(x, index), _series(nx.pagerank(G, max_iter=max_iter), index), rtol=1e-12, atol=0)
        return _series(x, index), it
    x, it = sense_oracle.eigenvector(G, max_iter=max_iter)
    return _series(x, index), it


@pytest.mark.parametrize('key', list(GRAPHS))
def test_node_measures_match_networkx(key):
    from graphrole_amd import node_measures
    G = GRAPHS[key]()
    max_iter = MAX_ITER.get(key, 100)
    M = node_measures(G) if max_iter == 100 else node_measures(G, max_iter=max_iter)
    index = sorted(G.nodes)
    assert list(M.index) == index
    directed, multi = G.is_directed(), G.is_multigraph()
    expected_cols = ['degree', 'weighted_degree'] + (['in_degree', 'out_degree'] if directed else []) \
        + (['clustering', 'effective_size'] if not directed and not multi else []) + ['pagerank'] \
        + ([] if multi else ['eigenvector'])
    assert list(M.columns) == expected_cols
    for name in M.columns:
        want, it = _expected(G, name, index, max_iter)
        got = M[name].to_numpy(dtype=np.float64)
        if name in ('pagerank', 'eigenvector'):
            assert M.attrs['iterations'][name] == it, (name, M.attrs['iterations'][name], it)
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=name)
        elif name == 'weighted_degree' and M[name].dtype.kind == 'f':
            # non-integer weights: the row sums add in CSR column order, networkx in adjacency order
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=name)
        else:
            assert np.array_equal(np.isnan(got), np.isnan(want)), name
            ok = ~np.isnan(want)
            assert np.array_equal(got[ok], want[ok]), (name, np.flatnonzero(got[ok] != want[ok])[:5])


def test_multigraph_and_directed_scope():
    from graphrole_amd import node_measures
    with pytest.raises(NotImplementedError):
        node_measures(_multigraph(), ['clustering'])
    with pytest.raises(NotImplementedError):
        node_measures(_multigraph(), ['eigenvector'])
    with pytest.raises(NotImplementedError, match='nx.clustering'):
        node_measures(_directed_weighted(), ['clustering'])
    with pytest.raises(NotImplementedError, match='nx.effective_size'):
        node_measures(_directed_weighted(), ['effective_size'])
    with pytest.raises(ValueError, match='catalogue'):
        node_measures(nx.karate_club_graph(), ['betweenness'])


def test_csr_input_equals_networkx_input_and_repeats_bitwise():
    from graphrole_amd import node_measures
    from graphrole_amd.graph.csr import CSRGraph
    G = nx.barabasi_albert_graph(2000, 5, seed=3)
    src, dst = np.array(list(G.edges)).T
    g = CSRGraph(G.number_of_nodes(), src, dst)
    a = node_measures(G)
    b = node_measures(g)
    c = node_measures(g)
    assert list(a.columns) == list(b.columns)
    for name in a.columns:
        assert np.array_equal(a[name].to_numpy(), b[name].to_numpy()), name
    assert c.to_numpy().tobytes() == b.to_numpy().tobytes()
    assert c.attrs['iterations'] == b.attrs['iterations']


def test_non_convergence_raises():
    from graphrole_amd import ConvergenceError, node_measures
    G = nx.barabasi_albert_graph(300, 3, seed=2)
    with pytest.raises(ConvergenceError) as info:
        node_measures(G, ['pagerank'], max_iter=2)
    assert info.value.iterations == 2
    assert isinstance(info.value, RuntimeError)
    with pytest.raises(ConvergenceError):
        node_measures(G, ['eigenvector'], max_iter=2)
    # networkx's own defaults do not converge on the star: the same error, after the same 100 iterations
    star = GRAPHS['star1500']()
    with pytest.raises(nx.PowerIterationFailedConvergence):
        nx.eigenvector_centrality(star)
    with pytest.raises(ConvergenceError) as info:
        node_measures(star, ['eigenvector'])
    assert info.value.iterations == 100


def test_fullsize_ba_pagerank_and_clustering():
    from graphrole_amd import node_measures, synth
    g = synth.ba_graph(1_000_000, 10, seed=0)
    M = node_measures(g, ['pagerank', 'clustering'])
    A = sense_oracle.csr_adjacency(g)
    x, it = sense_oracle.pagerank_matrix(A)
    assert M.attrs['iterations']['pagerank'] == it
    np.testing.assert_allclose(M['pagerank'].to_numpy(), x, rtol=1e-12, atol=0)
    assert np.array_equal(M['clustering'].to_numpy(), sense_oracle.clustering_arrays(g))


def test_fullsize_ba_eigenvector():
    """ev_iter_kernel and ev_normalize_kernel at 1 M nodes (their grid-stride loops take a second trip) against the
    long-double oracle; the same 1e-12 and the same iteration count."""
    from graphrole_amd import node_measures, synth
    g = synth.ba_graph(1_000_000, 10, seed=0)
    M = node_measures(g, ['eigenvector'])
    x, it, errs = measures_oracle.eigenvector_ld(g.row_ptr, g.col, g.w)
    thresh = g.n * 1e-6
    assert min(abs(float(e) / thresh - 1.0) for e in errs[-2:]) > 1e-6      # the count cannot flip under rounding
    assert M.attrs['iterations']['eigenvector'] == it
    got = M['eigenvector'].to_numpy()
    print(f'fullsize eigenvector: iterations {it}, max relative deviation {measures_oracle.max_rel_dev(got, x):.3e}')
    np.testing.assert_allclose(got.astype(np.longdouble), x, rtol=1e-12, atol=0)


def test_karate_end_to_end_sense_making():
    scipy_optimize = pytest.importorskip('scipy.optimize')
    from graphrole_amd import RecursiveFeatureExtractor, RoleExtractor, node_measures
    G = nx.karate_club_graph()
    features = RecursiveFeatureExtractor(G).extract_features()
    np.random.seed(0)
    role_extractor = RoleExtractor(n_roles=3)
    role_extractor.extract_role_factors(features)
    M = node_measures(G)
    E = role_extractor.sense_making(M)
    assert E is role_extractor.role_measure_factor
    assert list(E.index) == ['role_0', 'role_1', 'role_2'] and list(E.columns) == list(M.columns)
    Gf = role_extractor.node_role_factor.to_numpy(dtype=np.float64)
    Mv = M.to_numpy(dtype=np.float64)
    assert np.all(E.to_numpy() >= 0)
    for j, name in enumerate(M.columns):
        e, m = E[name].to_numpy(), Mv[:, j]
        g = Gf.T @ (Gf @ e - m)
        eps = 1e-8 * np.sqrt(np.max(np.sum(Gf * Gf, axis=0)) * (m @ m))
        assert np.all(g[e == 0] >= -eps) and np.all(np.abs(g[e > 0]) <= eps), name
        x_ref, _ = scipy_optimize.nnls(Gf, m)
        obj, obj_ref = np.sum((Gf @ e - m) ** 2), np.sum((Gf @ x_ref - m) ** 2)
        assert abs(obj - obj_ref) <= 1e-10 * (m @ m), name
    # the same table in another row order and normalised
    shuffled = M.iloc[np.random.default_rng(0).permutation(len(M))]
    assert role_extractor.sense_making(shuffled).equals(E)
    En = role_extractor.sense_making(M, normalize=True)
    assert np.all(En.to_numpy() >= 0)
    with pytest.raises(NotImplementedError):
        role_extractor.explain()
