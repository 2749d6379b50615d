"""
The small-graph atlas on the CPU: the fixture tests/golden/atlas_union.npz against networkx's Atlas of Graphs
regenerated now, its stored slow columns against a recomputation on a seeded sample, and EVERY numpy oracle next to the
tests run over the whole atlas and compared with networkx (or, for graphlets, with enumeration) at the exactness or
tolerance its own ``_cpu`` test uses.  tests/test_gpu_atlas.py compares the kernels with the same references; this file
is where an oracle that shares a misconception with its kernel would show, on every graph of up to 7 nodes.

Oracles run on the union in one call (seconds, measured on the CPU host): betweenness_oracle 1.5 s per variant,
closeness_oracle 0.4 s, sssp_oracle's distance matrix of 64 sources < 0.1 s, clustering_oracle 0.3 s,
square_clustering_oracle 0.4 s, structural_holes_oracle 0.2 s, kcore_oracle, truss_oracle, components_oracle < 0.2 s
each, biconnected_oracle 0.2 s, graphlet_oracle 0.3 s, measures_oracle < 0.1 s per iteration loop.  Run one atlas graph
at a time instead: weighted_betweenness_oracle (72 s on the union: every batch of 64 sources carries dense n x 64
tables; 1 s one graph at a time), sssp_oracle's sums over EVERY source (24 s on the union for the same reason; 1 s one
graph at a time) and eccentricity_oracle (per component by its nature: networkx raises on the union, and so does the
oracle).  The whole file takes about 30 s.

No atlas graph disagreed with networkx in any oracle when this file was written: 0 in each of the 14.
"""
import importlib.util
import os
from collections import Counter

import networkx as nx
import numpy as np
import pytest

from tests import atlas
from tests import betweenness_oracle as bo
from tests import biconnected_oracle as bio
from tests import closeness_oracle as co
from tests import clustering_oracle as clo
from tests import components_oracle as cpo
from tests import eccentricity_oracle as eo
from tests import graphlet_oracle as go
from tests import kcore_oracle as ko
from tests import measures_oracle as mo
from tests import sense_oracle
from tests import square_clustering_oracle as sqo
from tests import sssp_oracle as so
from tests import structural_holes_oracle as sho
from tests import truss_oracle as to
from tests import weighted_betweenness_oracle as wo

N = atlas.n_nodes()
SAMPLE_SEED, SAMPLE = 7, 125


def _generator():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'make_golden_atlas.py')
    spec = importlib.util.spec_from_file_location('make_golden_atlas', path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def _col(values: dict) -> np.ndarray:
    return atlas.of_dict(values, range(N))


def _graph(variant='undirected'):
    return atlas.graph(variant, 'identity')


def _symmetric_csr():
    src, dst, _ = atlas.arcs('undirected')
    return ko.symmetric_csr(N, np.stack([src, dst], axis=1))


def _directed_csrs():
    src, dst, _ = atlas.arcs('directed')
    return ko.directed_csr(N, np.stack([src, dst], axis=1)) + ko.directed_csr(N, np.stack([dst, src], axis=1))


def _same(got, want, what):
    """Equal as floats / integers, NaNs in the same places."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(got, want, equal_nan=True), (what, np.flatnonzero(~((got == want) | np.isnan(want)))[:5])


# ------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_is_the_atlas_of_graphs_regenerated_now():
    """Fixture drift, or a networkx whose atlas changed, fails here: edges, graph ids, and the seeded relabelling,
    orientation and weights, array for array; and the quantities the union is known by."""
    fresh, stored = _generator().structure(), atlas.load()
    for key, value in fresh.items():
        assert stored[key].dtype == value.dtype and np.array_equal(stored[key], value), key
    assert set(stored) == set(fresh) | set(atlas.STORED) | {'seed', 'networkx_version'}
    atlas_graphs = nx.graph_atlas_g()
    assert len(atlas_graphs) == 1253 and len(atlas.small_graphs()) == 1252
    for (a, lo, G), H in zip(atlas.small_graphs(), atlas_graphs[1:]):
        assert nx.utils.graphs_equal(G, _plain(H)) and lo == sum(len(g) for g in atlas_graphs[:a]), a
    U = _graph()
    assert (U.number_of_nodes(), U.number_of_edges()) == (8475, 12342) == (N, len(stored['src']))
    assert nx.number_connected_components(U) == 1610
    assert sum(1 for _, d in U.degree() if d == 0) == 296 and max(d for _, d in U.degree()) == 6
    assert sorted(stored['perm'].tolist()) == list(range(N))
    first, size = atlas.bounds()
    spread = [np.ptp(stored['perm'][lo:lo + k]) for lo, k in zip(first, size) if k > 1]
    assert min(spread) > 7                                     # 'perm' interleaves: no component stays contiguous
    assert set(np.unique(stored['orient'])) == {0, 1, 2} and set(np.unique(stored['weight'])) == {1, 2, 3}
    for variant in atlas.VARIANTS:
        for relabel in atlas.RELABELLINGS:
            G = atlas.graph(variant, relabel)
            assert sorted(G) == list(range(N)) and G.is_directed() == (variant == 'directed')
    assert list(atlas.graph('undirected', 'perm')) != sorted(atlas.graph('undirected', 'perm'))
    D = _graph('directed')
    both = int((stored['orient'] == atlas.BOTH).sum())
    assert D.number_of_edges() == 12342 + both and nx.utils.graphs_equal(D.to_undirected(), U)
    C = atlas.cone('perm')
    assert C.degree(atlas.apex()) == N and C.number_of_edges() == 12342 + N


def _plain(H):
    """An atlas graph without networkx's graph attributes (its name)."""
    G = nx.Graph()
    G.add_nodes_from(H)
    G.add_edges_from(H.edges())
    return G


def test_stored_columns_equal_a_recomputation_on_a_seeded_sample():
    """125 seeded atlas graphs, each recomputed with networkx on the small graph alone, equal as floats; and
    betweenness recomputed on the union of the sample in one call (the stored columns rest on every one of these
    measures being local to a component)."""
    rng = np.random.default_rng(SAMPLE_SEED)
    first, size = atlas.bounds()
    sample = np.sort(rng.choice(len(first), size=SAMPLE, replace=False))
    stored = atlas.load()
    graphs, directed = atlas.small_graphs('weighted'), atlas.small_graphs('directed')
    assert len({graphs[i][2].number_of_nodes() for i in sample}) >= 4
    for i in sample.tolist():
        _, lo, G = graphs[i]
        D = directed[i][2]
        k = G.number_of_nodes()
        alone = [v for v in G if G.degree(v) == 0]
        H = G.subgraph([v for v in G if G.degree(v) > 0])
        fresh = {
            'betweenness': nx.betweenness_centrality(G, normalized=False),
            'betweenness_endpoints': nx.betweenness_centrality(G, normalized=False, endpoints=True),
            'betweenness_directed': nx.betweenness_centrality(D, normalized=False),
            'betweenness_weighted': nx.betweenness_centrality(G, normalized=False, weight='weight'),
            'constraint': nx.constraint(H), 'constraint_weighted': nx.constraint(H, weight='weight'),
            'effective_size': nx.effective_size(H), 'effective_size_weighted': nx.effective_size(H, weight='weight'),
        }
        assert set(fresh) == set(atlas.STORED)
        for name, values in fresh.items():
            want = np.array([values.get(v, np.nan) for v in range(k)], dtype=np.float64)
            assert np.isnan(want).sum() == (len(alone) if name.startswith(('constraint', 'effective')) else 0)
            _same(stored[name][lo:lo + k], want, (name, graphs[i][0]))
    nodes = np.concatenate([np.arange(first[i], first[i] + size[i]) for i in sample])
    S = _graph().subgraph(nodes.tolist())
    for name, endpoints in (('betweenness', False), ('betweenness_endpoints', True)):
        got = nx.betweenness_centrality(S, normalized=False, endpoints=endpoints)
        np.testing.assert_allclose([got[v] for v in nodes.tolist()], stored[name][nodes], rtol=bo.RTOL, atol=0)


def test_place_and_by_label_round_trip():
    degrees = [dict(G.degree()) for _, _, G in atlas.small_graphs()]
    placed = atlas.place(degrees, dtype=np.int64)
    assert np.array_equal(placed, _col(dict(_graph().degree())))
    for relabel in atlas.RELABELLINGS:
        series = atlas.by_label(placed, relabel, 'degree')
        G = atlas.graph('undirected', relabel)
        assert series.to_dict() == dict(G.degree())
        assert np.array_equal(atlas.atlas_order(series, relabel), placed)
        assert np.array_equal(atlas.stored('betweenness', relabel).to_numpy()[atlas.relabelling(relabel)],
                              atlas.load()['betweenness'])
    vectors = atlas.place([[[v, G.degree(v)] for v in G] for _, _, G in atlas.small_graphs()], dtype=np.int64)
    assert vectors.shape == (N, 2) and np.array_equal(vectors[:, 1], placed)


# ------------------------------------------------------------------------------------------- the oracles on the union
@pytest.mark.parametrize('variant, stored', [('undirected', 'betweenness'), ('undirected', 'betweenness_endpoints'),
                                             ('directed', 'betweenness_directed')])
def test_betweenness_oracle_on_the_union(variant, stored):
    got = bo.betweenness(_graph(variant), normalized=False, endpoints=stored.endswith('endpoints'))
    np.testing.assert_allclose(_col(got), atlas.load()[stored], rtol=bo.RTOL, atol=0)


def test_weighted_betweenness_oracle_one_atlas_graph_at_a_time_and_its_uneven_ties():
    """One atlas graph at a time (the union takes 72 s).  Integer weights 1 .. 3 put equally light paths of different
    hop counts -- a node whose tight predecessors lie at different depths of the shortest-path DAG, the case
    ``uneven_ties_graph`` builds by hand -- into a large share of the graphs, counted here from the oracle's depths:
    5127 (source, node) cells in 871 of the 1252 graphs with the fixture's seed."""
    stored = atlas.load()['betweenness_weighted']
    uneven_cells = uneven_graphs = 0
    for a, lo, G in atlas.small_graphs('weighted'):
        k = G.number_of_nodes()
        labels, out, inn = wo.csr_pair(G)
        assert labels == list(range(k))
        sources = np.arange(k, dtype=np.int64)
        terms, _, _ = wo.source_terms(out, inn, sources)
        bc = wo.accumulate(terms, k, False, 0.5)
        np.testing.assert_allclose(bc, stored[lo:lo + k], rtol=wo.RTOL, atol=0, err_msg=str(a))
        row_ptr, col, w = inn
        dist, _ = so.relax(row_ptr, col, w, sources)
        v = np.repeat(np.arange(k), np.diff(row_ptr))
        cells = 0
        for (s, depth, _), D in zip(terms, dist):
            tight = np.isfinite(D[v]) & (D[col] + w == D[v]) & (D[col] < D[v])
            lowest, highest = np.full(k, k), np.full(k, -1)
            np.minimum.at(lowest, v[tight], depth[col[tight]])
            np.maximum.at(highest, v[tight], depth[col[tight]])
            cells += int((highest > lowest).sum())
        uneven_cells += cells
        uneven_graphs += cells > 0
    print(f'uneven ties: {uneven_cells} (source, node) cells in {uneven_graphs} of {len(atlas.small_graphs())} graphs')
    assert uneven_cells > 0 and uneven_graphs > 0
    assert uneven_graphs >= 300, (uneven_graphs, uneven_cells)   # "a large share": at least a quarter of the graphs


def test_closeness_oracle_on_the_union():
    U, D = _graph(), _graph('directed')
    for G in (U, D):
        for wf in (True, False):
            assert co.closeness(G, wf_improved=wf) == nx.closeness_centrality(G, wf_improved=wf)
        want = nx.harmonic_centrality(G)
        np.testing.assert_allclose(_col(co.harmonic(G)), _col(want), rtol=co.HARMONIC_RTOL, atol=0)
    assert co.harmonic(U) == co.harmonic_fsum(U)                # both are the correctly rounded sum
    assert sum(1 for x in co.closeness(U).values() if x == 0.0) == 296     # the zero-distance branch: isolated nodes


def test_sssp_oracle_on_the_union():
    W = _graph('weighted')
    sources = np.random.default_rng(64).choice(N, size=64, replace=False)
    labels, row_ptr, col, w = so.pulled_csr(W)
    assert labels == list(range(N))
    reach, dsum, harmonic, far, source_ecc, dist, rounds = so.weighted_distances(row_ptr, col, w, sources)
    want = so.networkx_matrix(W, sources.tolist())
    assert np.array_equal(dist, want) and np.isinf(want).any() and rounds >= 2
    for a, lo, G in atlas.small_graphs('weighted'):             # the sums over every source: one atlas graph at a time
        k = G.number_of_nodes()
        _, row_ptr, col, w = so.pulled_csr(G)
        reach, dsum, harmonic, *_ = so.weighted_distances(row_ptr, col, w, np.arange(k, dtype=np.int64))
        closeness = nx.closeness_centrality(G, distance='weight')
        np.testing.assert_allclose(so.closeness(reach, dsum, k), [closeness[v] for v in range(k)], rtol=so.RTOL,
                                   atol=0, err_msg=str(a))
        want = nx.harmonic_centrality(G, distance='weight')
        np.testing.assert_allclose(harmonic, [want[v] for v in range(k)], rtol=so.RTOL, atol=0, err_msg=str(a))


@pytest.mark.parametrize('variant, weight', [('undirected', None), ('weighted', 'weight'), ('directed', None)])
def test_clustering_oracle_on_the_union(variant, weight):
    G = _graph(variant)
    got, _ = clo.exact(*clo.directional_csr(G, weight))
    want = np.array([float(x) for x in _col(nx.clustering(G, weight=weight))])
    clo.assert_close(got, want, variant)
    if weight is None:
        assert np.array_equal(got, want)                        # integers only: networkx bit for bit


def test_square_clustering_oracle_on_the_union():
    _, _, got = sqo.square_clustering(*_symmetric_csr())
    want = nx.square_clustering(_graph())
    assert got.tolist() == [float(want[v]) for v in range(N)]


@pytest.mark.parametrize('variant, weight, suffix', [('undirected', None, ''), ('weighted', 'weight', '_weighted')])
def test_structural_holes_oracle_on_the_union(variant, weight, suffix):
    row_ptr, col, z, out_row_ptr = sho.mutual_csr(_graph(variant), weight)
    stored = atlas.load()
    want = (stored['constraint' + suffix], stored['effective_size' + suffix], None)
    sho.assert_close(sho.exact(row_ptr, col, z, out_row_ptr), want, row_ptr, variant)
    sho.assert_close(sho.sparse(row_ptr, col, z, out_row_ptr), want, row_ptr, (variant, 'sparse'))


def test_kcore_oracle_on_the_union():
    U, D = _graph(), _graph('directed')
    r = ko.core_numbers(*_symmetric_csr())
    assert np.array_equal(r.core, _col(nx.core_number(U))) and np.array_equal(r.onion, _col(nx.onion_layers(U)))
    assert r.n_rounds == max(nx.onion_layers(U).values())
    assert np.array_equal(ko.core_numbers(*_directed_csrs()).core, _col(nx.core_number(D)))


def test_truss_oracle_on_the_union():
    row_ptr, col = _symmetric_csr()
    r = to.truss_numbers(row_ptr, col)
    edge_t, node_t = to.networkx_truss_numbers(_graph())
    rows = np.repeat(np.arange(N), np.diff(row_ptr))
    assert r.arc_truss.tolist() == [edge_t[frozenset(e)] for e in zip(rows.tolist(), col.tolist())]
    assert np.array_equal(r.node_truss, _col(node_t))
    assert sorted(set(r.arc_truss.tolist())) == [2, 3, 4, 5, 6, 7]            # K7: every edge in 5 triangles


def test_biconnected_oracle_on_the_union():
    U = _graph()
    r = bio.biconnected(*_symmetric_csr())
    blocks = {frozenset(c) for c in nx.biconnected_components(U)}
    assert bio.components(r.parent, r.label) == blocks and r.n_components == len(blocks)
    counts = Counter(v for c in blocks for v in c)
    assert r.count.tolist() == [counts.get(v, 0) for v in range(N)]
    assert set(np.flatnonzero(r.count > 1).tolist()) == set(nx.articulation_points(U))
    assert any(len(b) == 2 for b in blocks)                     # the 2-node blocks (bridges) are there


def test_components_oracle_on_the_union():
    U, D = _graph(), _graph('directed')
    r = cpo.components(*_symmetric_csr(), mode=cpo.CONNECTED)
    assert cpo.partition(r.label) == frozenset(frozenset(c) for c in nx.connected_components(U))
    assert r.n_components == 1610
    row_ptr, col, in_row_ptr, in_col = _directed_csrs()
    weak, strong = cpo.components(row_ptr, col, mode=cpo.WEAK), cpo.components(row_ptr, col, mode=cpo.STRONG)
    assert cpo.partition(weak.label) == frozenset(frozenset(c) for c in nx.weakly_connected_components(D))
    assert cpo.partition(strong.label) == frozenset(frozenset(c) for c in nx.strongly_connected_components(D))
    assert np.array_equal(strong.size, np.bincount(strong.label, minlength=N)[strong.label])
    from tests.test_components_cpu import _bow_tie_by_definition
    assert np.array_equal(cpo.bow_tie(row_ptr, col, in_row_ptr, in_col), _bow_tie_by_definition(D, list(range(N))))
    for s in np.random.default_rng(64).choice(N, size=64, replace=False).tolist():
        flag = np.zeros(N, dtype=np.int32)
        flag[s] = 1
        assert set(np.flatnonzero(cpo.reachable(row_ptr, col, flag)[0]).tolist()) - {s} == nx.descendants(D, s)
        assert set(np.flatnonzero(cpo.reachable(in_row_ptr, in_col, flag)[0]).tolist()) - {s} == nx.ancestors(D, s)


def test_graphlet_oracle_on_the_union():
    """The kernel's formulas on the union against enumeration, one atlas graph at a time (there is no networkx function
    to restate)."""
    want = atlas.place([go.brute_orbits(G) for _, _, G in atlas.small_graphs()], dtype=np.int64)
    got = go.orbits(*_symmetric_csr())
    assert np.array_equal(got.orbits.T, want)
    assert np.array_equal(want[:, 0], _col(dict(_graph().degree())))
    assert np.array_equal(want[:, 3], _col(nx.triangles(_graph())))
    assert want[:, 14].sum() > 0 and want[:, 8].sum() > 0 and np.all(want.sum(axis=0) > 0)    # every orbit occurs


@pytest.mark.parametrize('variant', ['undirected', 'directed'])
def test_measures_oracle_on_the_union(variant):
    """pagerank / eigenvector in float64 and in long double against networkx's own loops, iteration counts included
    (the stopping decision is nowhere near a tie: the last errors are 0.95 and 1.002 of the threshold); the local
    measures bit-equal to networkx."""
    G = _graph(variant)
    src, dst, _ = atlas.arcs(variant)
    if variant == 'undirected':
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    csr = mo.csr_from_arcs(N, src, dst)
    pr, pr_it = sense_oracle.pagerank(G)
    ev, ev_it = sense_oracle.eigenvector(G)
    np.testing.assert_allclose(_col(pr), _col(nx.pagerank(G)), rtol=mo.RTOL, atol=0)
    np.testing.assert_allclose(_col(ev), _col(nx.eigenvector_centrality(G)), rtol=mo.RTOL, atol=0)
    thresh = N * 1e-6
    for run, want, want_it in ((mo.pagerank_f64, pr, pr_it), (mo.pagerank_ld, pr, pr_it),
                               (mo.eigenvector_f64, ev, ev_it), (mo.eigenvector_ld, ev, ev_it)):
        x, it, errs = run(csr.row_ptr, csr.col, None)
        assert it == want_it and min(abs(float(e) / thresh - 1.0) for e in errs[-2:]) > 1e-6
        np.testing.assert_allclose(x.astype(np.float64), _col(want), rtol=mo.RTOL, atol=0)
    if variant == 'undirected':
        deg = np.diff(csr.row_ptr)
        own, nl = mo.loop_counts(csr.row_ptr, csr.col)
        cl, es = mo.local_measures(deg, own, _col(nx.triangles(G)), nl)
        _same(cl, _col(nx.clustering(G)), 'clustering')
        _same(es, atlas.load()['effective_size'], 'effective_size')


def test_eccentricity_oracle_per_component():
    """One atlas graph at a time: both methods equal networkx on the connected graphs and raise networkx's error on the
    others (as on the union itself)."""
    connected = 0
    for a, lo, G in atlas.small_graphs():
        nodes = list(G)
        row_ptr, col = eo.pull_csr(G, nodes)
        if nx.is_connected(G):
            connected += 1
            want = _small(nx.eccentricity(G), nodes)
            for method in ('all', 'bounds'):
                assert np.array_equal(eo.eccentricity(row_ptr, col, method=method, batch=2)[0], want), (a, method)
        else:
            for method in ('all', 'bounds'):
                with pytest.raises(nx.NetworkXError, match='not connected'):
                    eo.eccentricity(row_ptr, col, method=method, batch=2)
    assert connected == 1 + 1 + 2 + 6 + 21 + 112 + 853          # the connected graphs on 1 .. 7 nodes
    row_ptr, col = _symmetric_csr()
    with pytest.raises(nx.NetworkXError, match='not connected'):
        eo.eccentricity(row_ptr, col, method='all')


def _small(values, nodes):
    return np.array([values[v] for v in nodes], dtype=np.int64)
