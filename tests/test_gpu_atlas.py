"""
Every sense-making measure over the whole small-graph atlas on the MI355X: the disjoint union of all 1252 non-null
graphs on 1-7 nodes (tests/atlas.py; 8475 nodes, 12342 edges, 1610 components, 296 isolated nodes, maximum degree 6),
so one device call per measure tests it on every graph of up to 7 nodes at once -- "K4 minus an edge hanging off a
bridge next to an isolated node" included -- and loads the component, union-find and peeling machinery with 1610
components at the same moment.  One test per measure family through the public functions of graphrole_amd (so the
labels <-> rows map is tested too), each under two relabellings: 'identity' (components contiguous in id space) and
'perm' (interleaved).  The maximum degree is 6: by design these are the short-row (lane-group) paths; the cone at the
end of the file puts one hub row of 8475 arcs over every small structure.

References: networkx on the union, computed once on the 'identity' graph and placed by label (a relabelling changes
none of these values, only the order of floating-point sums), the slow columns from the fixture
(tools/make_golden_atlas.py; tests/test_atlas_cpu.py recomputes a sample), graphlets from brute-force enumeration per
atlas graph.  Tolerances are imported from the family's own oracle module, never restated.

Equivariance: the results under 'identity' and under 'perm', mapped back by label, are compared in every test.
  * bitwise: every integer-valued measure, and every float measure whose value is one or two IEEE operations on exact
    integers (clustering without weights, effective size without weights, closeness, square clustering) or the
    correctly rounded value of an exact sum (harmonic centrality: grx_closeness.hip, "the same bits for every W, source
    order and run");
  * at the family tolerance: the float measures whose kernels add fp64 terms in arc order or source order
    (betweenness, weighted betweenness, constraint, weighted effective size, weighted clustering, PageRank, eigenvector
    centrality).  Their headers promise the same bits in every RUN; the arc order of a row follows the ids of its
    neighbours (the internal order is degree-descending, ties by id), so a relabelling reorders those sums.  Measured
    on the MI355X, entries whose bits differ between the two relabellings (largest relative difference): PageRank 687
    of 8475 (9e-16), eigenvector 7736 (3e-15), constraint 185 (4e-16), weighted constraint 585, weighted effective size
    465, weighted clustering 464 (4e-16 each), weighted betweenness 6 (3e-16), betweenness without weights 0 -- its
    sums are short enough here to come out the same, which nothing promises;
  * not asserted where the documented result itself depends on the ids: ``component_table`` ranks, ``largest_component``
    and ``bow_tie`` break ties between equally large components by the first member in the index.

networkx on the cone (one apex joined to all 8475 nodes), measured on the CPU host: nx.triangles 0.06 s, nx.clustering
1.8 s, nx.core_number 0.09 s, nx.biconnected_components 0.03 s, nx.articulation_points 0.02 s,
nx.connected_components < 0.01 s.  nx.k_truss on the whole cone takes 12.5 s for k = 2 .. 9 (it rebuilds the apex's
neighbour set per edge), so the truss reference is computed one atlas graph at a time (0.4 s): every triangle of the
cone lies inside the cone over ONE atlas graph, so the peeling of the cone is the peeling of those 1252 small cones side
by side (checked once against the 12.5 s computation: equal on every edge and node).  nx.square_clustering walks 36 M
neighbour pairs of the apex and is not run.

Measured on the MI355X: the 43 cases of this file take 12.6 s together, the slowest (the first catalogue call, which
also loads the library) 1.3 s; each all-sources betweenness test (8475 sources, both relabellings, both `endpoints`)
stays under 0.1 s, so the sources are not cut.  ``closeness_centrality`` itself refuses ``distance=``: the column by
weight comes from ``node_measures(G, ['closeness_centrality'], distance='weight')``, as its message says.

No atlas graph disagreed with its reference in any family when this file was written: 0 of 1252 in each.
"""
import functools
from collections import Counter

import networkx as nx
import numpy as np
import pytest

from tests import atlas
from tests import betweenness_oracle as bo
from tests import closeness_oracle as co
from tests import clustering_oracle as clo
from tests import graphlet_oracle as go
from tests import measures_oracle as mo
from tests import sense_oracle
from tests import sssp_oracle as so
from tests import structural_holes_oracle as sho
from tests import truss_oracle as to
from tests import weighted_betweenness_oracle as wo
from tests.guard_scenarios import LANES

pytestmark = pytest.mark.gpu

RELABEL = pytest.mark.parametrize('relabel', atlas.RELABELLINGS)
N = atlas.n_nodes()
#: graphlet -> (an orbit of it, the nodes of one copy on that orbit): Przulj's table, restated
GRAPHLETS = {'edge': (0, 2), 'path3': (2, 1), 'triangle': (3, 3), 'path4': (4, 2), 'star4': (7, 1), 'cycle4': (8, 4),
             'paw': (9, 1), 'diamond': (13, 2), 'clique4': (14, 4)}
SOURCE_SEED = 64


# --------------------------------------------------------------------------------------------------------- helpers
def _col(values: dict) -> np.ndarray:
    """networkx's dict on an 'identity' graph as an array in atlas order."""
    return atlas.of_dict(values, range(N))


def _rows(series, relabel) -> np.ndarray:
    """A result behind the sorted labels, in atlas order."""
    assert len(series) == N and np.array_equal(np.asarray(series.index), np.arange(N))
    return atlas.atlas_order(series, relabel)


def _inverse(relabel) -> np.ndarray:
    inv = np.empty(N, dtype=np.int64)
    inv[atlas.relabelling(relabel)] = np.arange(N)
    return inv


def _sets_in_atlas_ids(sets, relabel) -> frozenset:
    inv = _inverse(relabel)
    return frozenset(frozenset(inv[list(s)].tolist()) for s in sets)


def _exact(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype.kind == 'f' or want.dtype.kind == 'f':
        assert np.array_equal(np.isnan(got), np.isnan(want)), (what, 'NaN places')
        ok = ~np.isnan(want.astype(np.float64))
        got, want = got[ok], want[ok]
    bad = np.flatnonzero(got != want)
    assert not len(bad), (what, bad[:5], got[bad[:5]], want[bad[:5]])


def _close(got, want, rtol, what):
    """NaNs in the same places, rtol relative elsewhere with atol = 0 (so exact zeros stay exact zeros)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, 'NaN places')
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=rtol, atol=0, err_msg=str(what))


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype)
    if a.dtype.kind == 'f':
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, 'NaN places')
        a, b = np.where(np.isnan(a), 0.0, a), np.where(np.isnan(b), 0.0, b)
    assert a.tobytes() == b.tobytes(), (what, 'identity vs perm', np.argwhere(a != b)[:5])


_GOT = {}


def _got(key, relabel, run):
    """run(relabel) once per relabelling for the whole module: a dict name -> result in atlas order / atlas ids."""
    if (key, relabel) not in _GOT:
        _GOT[key, relabel] = run(relabel)
    return _GOT[key, relabel]


def _equivariant(key, run, bitwise=(), close=None):
    """The two relabellings against each other, mapped back by label: `bitwise` names with the same bits, `close`
    name -> rtol at the family tolerance (atol 0, NaNs in the same places) or a check(a, b) of the family's own."""
    a, b = _got(key, 'identity', run), _got(key, 'perm', run)
    for name in bitwise:
        if isinstance(a[name], np.ndarray):
            _same_bits(a[name], b[name], (key, name))
        else:
            assert a[name] == b[name], (key, name, 'identity vs perm')
    for name, rtol in (close or {}).items():
        if callable(rtol):
            rtol(a[name], b[name])
        else:
            _close(a[name], b[name], rtol, (key, name, 'identity vs perm'))


def _sources(seed=SOURCE_SEED, k=64) -> np.ndarray:
    """64 seeded atlas nodes."""
    return np.random.default_rng(seed).choice(N, size=k, replace=False)


# ------------------------------------------------------------------------------------------------ undirected union
@functools.lru_cache(maxsize=None)
def _want_power(variant):
    """(pagerank, its iterations, eigenvector, its iterations) of networkx's loops (tests/sense_oracle.py) on the
    'identity' graph, the PageRank checked against nx.pagerank itself as tests/test_gpu_sense.py does."""
    G = atlas.graph(variant, 'identity')
    pr, pr_it = sense_oracle.pagerank(G)
    np.testing.assert_allclose(_col(pr), _col(nx.pagerank(G)), rtol=mo.RTOL, atol=0)
    ev, ev_it = sense_oracle.eigenvector(G)
    np.testing.assert_allclose(_col(ev), _col(nx.eigenvector_centrality(G)), rtol=mo.RTOL, atol=0)
    return _col(pr), pr_it, _col(ev), ev_it


def _run_catalogue(variant, relabel):
    from graphrole_amd import node_measures
    from graphrole_amd.measures import available_measures
    G = atlas.graph(variant, relabel)
    names = available_measures(G.is_directed(), False)
    M = node_measures(G, names)                                 # every name in one call
    assert list(M.columns) == names
    out = {name: _rows(M[name], relabel) for name in names}
    out['iterations'] = dict(M.attrs['iterations'])
    return out


@RELABEL
def test_catalogue_of_the_undirected_union(relabel):
    """Every name of available_measures(False, False) in one node_measures call.  Eigenvector centrality is not defined
    on a disconnected graph; measures.py documents no special case -- the column restates networkx's power iteration
    with networkx's start vector and stopping rule, which converges here (75 iterations: the K7 component wins) -- so
    the whole column is compared with that iteration, count included."""
    run = functools.partial(_run_catalogue, 'undirected')
    got = _got('catalogue', relabel, run)
    U = atlas.graph('undirected', 'identity')
    assert [k for k in got if k != 'iterations'] == ['degree', 'weighted_degree', 'clustering', 'effective_size',
                                                     'pagerank', 'eigenvector']
    degree = _col(dict(U.degree()))
    assert got['degree'].dtype == np.int64 and got['weighted_degree'].dtype == np.int64
    _exact(got['degree'], degree, 'degree')
    _exact(got['weighted_degree'], degree, 'weighted_degree')
    _exact(got['clustering'], _col(nx.clustering(U)), 'clustering')
    _exact(got['effective_size'], atlas.load()['effective_size'], 'effective_size')
    pr, pr_it, ev, ev_it = _want_power('undirected')
    assert got['iterations'] == {'pagerank': pr_it, 'eigenvector': ev_it}
    _close(got['pagerank'], pr, mo.RTOL, 'pagerank')
    _close(got['eigenvector'], ev, mo.RTOL, 'eigenvector')
    _equivariant('catalogue', run, bitwise=('degree', 'weighted_degree', 'clustering', 'effective_size', 'iterations'),
                 close={'pagerank': mo.RTOL, 'eigenvector': mo.RTOL})


def _run_betweenness(relabel):
    from graphrole_amd import betweenness_centrality
    G = atlas.graph('undirected', relabel)
    return {f'endpoints={e}': _rows(betweenness_centrality(G, normalized=False, endpoints=e), relabel)
            for e in (False, True)}


@RELABEL
def test_betweenness_from_all_sources(relabel):
    """normalized=False, endpoints both ways, all 8475 sources (133 batches of 64) against the stored networkx columns.
    Tolerance class: the dependencies of a node are added in arc order and source order."""
    got = _got('betweenness', relabel, _run_betweenness)
    _close(got['endpoints=False'], atlas.load()['betweenness'], bo.RTOL, 'betweenness')
    _close(got['endpoints=True'], atlas.load()['betweenness_endpoints'], bo.RTOL, 'betweenness with endpoints')
    _equivariant('betweenness', _run_betweenness, close={'endpoints=False': bo.RTOL, 'endpoints=True': bo.RTOL})


def _run_closeness(relabel):
    from graphrole_amd import closeness_centrality, harmonic_centrality
    G = atlas.graph('undirected', relabel)
    out = {f'wf_improved={wf}': _rows(closeness_centrality(G, wf_improved=wf), relabel) for wf in (True, False)}
    out['harmonic'] = _rows(harmonic_centrality(G), relabel)
    return out


@RELABEL
def test_closeness_and_harmonic_centrality(relabel):
    """The zero-distance branch of closeness (296 isolated nodes) next to every component size 2 .. 7.  Bitwise class:
    closeness is three IEEE operations on exact integers, harmonic the correctly rounded value of an exact sum."""
    got = _got('closeness', relabel, _run_closeness)
    U = atlas.graph('undirected', 'identity')
    for wf in (True, False):
        _exact(got[f'wf_improved={wf}'], _col(nx.closeness_centrality(U, wf_improved=wf)), ('closeness', wf))
    _close(got['harmonic'], _col(nx.harmonic_centrality(U)), co.HARMONIC_RTOL, 'harmonic')
    _equivariant('closeness', _run_closeness, bitwise=('wf_improved=True', 'wf_improved=False', 'harmonic'))


def _run_peeling(relabel):
    from graphrole_amd import core_number, onion_layers
    G = atlas.graph('undirected', relabel)
    return {'core': _rows(core_number(G), relabel), 'onion': _rows(onion_layers(G), relabel)}


@RELABEL
def test_core_numbers_and_onion_layers(relabel):
    """Every peeling round structure on up to 7 nodes, 1610 components peeled side by side.  Bitwise class: integers."""
    got = _got('peeling', relabel, _run_peeling)
    U = atlas.graph('undirected', 'identity')
    assert got['core'].dtype == np.int64 and got['onion'].dtype == np.int64
    _exact(got['core'], _col(nx.core_number(U)), 'core_number')
    _exact(got['onion'], _col(nx.onion_layers(U)), 'onion_layers')
    _equivariant('peeling', _run_peeling, bitwise=('core', 'onion'))


def _run_biconnected(relabel):
    from graphrole_amd import articulation_points, biconnected_component_counts, biconnected_components
    G = atlas.graph('undirected', relabel)
    points = articulation_points(G)
    assert points == sorted(points)                             # index order
    return {'counts': _rows(biconnected_component_counts(G), relabel),
            'points': frozenset(_inverse(relabel)[points].tolist()),
            'blocks': _sets_in_atlas_ids(biconnected_components(G), relabel)}


@RELABEL
def test_biconnected_components_and_articulation_points(relabel):
    """Every block structure on up to 7 nodes, the 2-node blocks (bridges) among them, in 1610 trees of one forest.
    Bitwise class: integers and sets of nodes (mapped back to atlas ids)."""
    got = _got('biconnected', relabel, _run_biconnected)
    U = atlas.graph('undirected', 'identity')
    blocks = [frozenset(c) for c in nx.biconnected_components(U)]
    counts = Counter(v for c in blocks for v in c)
    _exact(got['counts'], np.array([counts.get(v, 0) for v in range(N)], dtype=np.int64), 'counts')
    assert got['points'] == frozenset(nx.articulation_points(U))
    assert got['blocks'] == frozenset(blocks) and len(got['blocks']) == len(blocks)
    _equivariant('biconnected', _run_biconnected, bitwise=('counts', 'points', 'blocks'))


def _run_clustering(relabel):
    from graphrole_amd import average_clustering, clustering, square_clustering
    G = atlas.graph('undirected', relabel)
    return {'clustering': _rows(clustering(G), relabel), 'square': _rows(square_clustering(G), relabel),
            'average': average_clustering(G), 'average_nonzero': average_clustering(G, count_zeros=False)}


@RELABEL
def test_clustering_and_square_clustering(relabel):
    """Bitwise class: integers until one division.  (The averages are math.fsum means on the host: correctly rounded,
    so they do not depend on the order either.)"""
    got = _got('clustering', relabel, _run_clustering)
    U = atlas.graph('undirected', 'identity')
    _exact(got['clustering'], _col(nx.clustering(U)), 'clustering')
    _exact(got['square'], np.array([float(x) for x in _col(nx.square_clustering(U))]), 'square_clustering')
    for name, count_zeros in (('average', True), ('average_nonzero', False)):
        want = nx.average_clustering(U, count_zeros=count_zeros)
        assert abs(got[name] - want) <= clo.RTOL * want, (name, got[name], want)
    _equivariant('clustering', _run_clustering, bitwise=('clustering', 'square', 'average', 'average_nonzero'))


def _run_structural_holes(relabel):
    from graphrole_amd import constraint, effective_size
    G = atlas.graph('undirected', relabel)
    return {'constraint': _rows(constraint(G), relabel), 'effective_size': _rows(effective_size(G), relabel)}


def _effective_size_close(g, w, what='effective_size'):
    """The family's bound: |got - want| <= ES_ATOL * max(d, 1), absolute because the terms cancel."""
    deg = np.maximum(_col(dict(atlas.graph('undirected', 'identity').degree())), 1)
    assert np.array_equal(np.isnan(g), np.isnan(w)), (what, 'NaN places')
    ok = ~np.isnan(w)
    err = np.abs(g[ok] - w[ok])
    assert np.all(err <= sho.ES_ATOL * deg[ok]), (what, float(err.max()))


def _check_structural_holes(got, suffix):
    _close(got['constraint'], atlas.load()['constraint' + suffix], sho.RTOL, 'constraint' + suffix)
    _effective_size_close(got['effective_size'], atlas.load()['effective_size' + suffix], 'effective_size' + suffix)


@RELABEL
def test_constraint_and_effective_size(relabel):
    """Against the stored networkx columns (NaN on the 296 isolated nodes).  Constraint: tolerance class (sums in arc
    order); effective size without weights is the integer formula n - 2t/n: bitwise class."""
    got = _got('holes', relabel, _run_structural_holes)
    _check_structural_holes(got, '')
    _equivariant('holes', _run_structural_holes, bitwise=('effective_size',), close={'constraint': sho.RTOL})


def _edge_values(series, relabel) -> np.ndarray:
    """An edge Series (MultiIndex u < v of labels, lexicographic) as an array over the fixture's edges."""
    label = atlas.relabelling(relabel)
    src, dst, _ = atlas.arcs('undirected')
    a, b = label[src], label[dst]
    key = np.minimum(a, b) * N + np.maximum(a, b)
    have = (series.index.get_level_values('u').to_numpy().astype(np.int64) * N
            + series.index.get_level_values('v').to_numpy().astype(np.int64))
    assert len(have) == len(key) and np.all(np.diff(have) > 0)
    at = np.searchsorted(have, key)
    assert np.array_equal(have[at], key)
    return series.to_numpy()[at]


@functools.lru_cache(maxsize=None)
def _want_truss():
    """(t(e) over the fixture's edges, t(v) in atlas order) from nx.k_truss on the 'identity' union."""
    edge_t, node_t = to.networkx_truss_numbers(atlas.graph('undirected', 'identity'))
    src, dst, _ = atlas.arcs('undirected')
    return (np.array([edge_t[frozenset(e)] for e in zip(src.tolist(), dst.tolist())], dtype=np.int64),
            _col(node_t).astype(np.int64))


def _run_truss(relabel):
    from graphrole_amd import node_truss_number, truss_number
    G = atlas.graph('undirected', relabel)
    return {'edge': _edge_values(truss_number(G), relabel), 'node': _rows(node_truss_number(G), relabel)}


@RELABEL
def test_truss_numbers_and_k_truss(relabel):
    """Edge and node truss numbers against nx.k_truss for every k, and k_truss(G, k) for k = 2 .. 6 as graphs.  Bitwise
    class: integers (grx_truss.hip: "the same bits ... for every relabelling")."""
    from graphrole_amd import k_truss
    got = _got('truss', relabel, _run_truss)
    want_edge, want_node = _want_truss()
    assert got['edge'].dtype == np.int64 and got['node'].dtype == np.int64
    _exact(got['edge'], want_edge, 'truss_number')
    _exact(got['node'], want_node, 'node_truss_number')
    G = atlas.graph('undirected', relabel)
    for k in range(2, 7):
        assert nx.utils.graphs_equal(k_truss(G, k), nx.k_truss(G, k)), k
    _equivariant('truss', _run_truss, bitwise=('edge', 'node'))


@functools.lru_cache(maxsize=None)
def _want_orbits():
    """int64[n, 15] by direct enumeration of every 3- and 4-subset, one atlas graph at a time."""
    return atlas.place([go.brute_orbits(G) for _, _, G in atlas.small_graphs()], dtype=np.int64)


def _run_graphlets(relabel):
    from graphrole_amd import graphlet_counts, graphlet_degree_vectors
    G = atlas.graph('undirected', relabel)
    frame = graphlet_degree_vectors(G)
    assert list(frame.columns) == [f'orbit_{k}' for k in range(15)] and all(frame.dtypes == np.int64)
    counts = graphlet_counts(G)
    assert frame.attrs['graphlets'] == counts.to_dict()
    return {'orbits': np.ascontiguousarray(_rows(frame, relabel)), 'counts': counts.to_dict()}


@RELABEL
def test_graphlet_degree_vectors_and_counts(relabel):
    """Every orbit formula on every graph of up to 7 nodes, against enumeration (tests/graphlet_oracle.py has no
    networkx to lean on: ``brute_orbits`` is the authority).  Bitwise class: integers (grx_graphlets.hip: "the same
    bits in every run, for every lanes_per_row and every relabelling")."""
    got = _got('graphlets', relabel, _run_graphlets)
    want = _want_orbits()
    _exact(got['orbits'], want, 'orbits')
    assert got['counts'] == {name: int(want[:, orbit].sum()) // times for name, (orbit, times) in GRAPHLETS.items()}
    _equivariant('graphlets', _run_graphlets, bitwise=('orbits', 'counts'))


def _labelled(sets_in_atlas_ids, relabel):
    """Components given in atlas ids as label sets, ordered by first member in the index."""
    label = atlas.relabelling(relabel)
    return sorted((set(label[list(s)].tolist()) for s in sets_in_atlas_ids), key=min)


def _check_table(table, ordered, n_components):
    """component = the rank by decreasing size, ties by first member in the index; component_size."""
    assert list(table.columns) == ['component', 'component_size'] and all(table.dtypes == np.int64)
    assert np.array_equal(np.asarray(table.index), np.arange(N))
    ranked = sorted(ordered, key=lambda s: (-len(s), min(s)))
    rank, size = np.empty(N, dtype=np.int64), np.empty(N, dtype=np.int64)
    for r, s in enumerate(ranked):
        members = list(s)
        rank[members], size[members] = r, len(s)
    _exact(table['component'].to_numpy(), rank, 'component')
    _exact(table['component_size'].to_numpy(), size, 'component_size')
    assert table.attrs['n_components'] == n_components
    return ranked


@RELABEL
def test_connected_components_of_1610_components(relabel):
    """The union-find with 1610 components at once, hook order under contiguous and under interleaved ids.  Both
    relabellings are held against the SAME networkx partition placed by label, which is the equivariance of the
    partition; ranks and the largest component break ties by label and are checked per relabelling."""
    import graphrole_amd as ga
    G = atlas.graph('undirected', relabel)
    want = _labelled(nx.connected_components(atlas.graph('undirected', 'identity')), relabel)
    assert len(want) == 1610
    got = ga.connected_components(G)
    assert got == want                                          # ordered by first member in the index
    assert ga.number_connected_components(G) == 1610 and ga.is_connected(G) is False
    ranked = _check_table(ga.component_table(G), want, 1610)
    assert list(ga.largest_component(G)) == sorted(ranked[0]) and len(ranked[0]) == 7


def test_eccentricity_and_its_kin_raise_on_the_union():
    """The public contract: networkx's error on a graph that is not connected.  (Values: test_gpu_eccentricity.py.)"""
    import graphrole_amd as ga
    G = atlas.graph('undirected', 'perm')
    with pytest.raises(nx.NetworkXError, match='Found infinite path length because the graph is not connected'):
        nx.eccentricity(G)
    for call in (ga.eccentricity, ga.diameter, ga.radius, ga.center, ga.periphery,
                 lambda g: ga.eccentricity(g, method='bounds'), lambda g: ga.node_measures(g, ['eccentricity'])):
        with pytest.raises(nx.NetworkXError, match='Found infinite path length because the graph is not connected'):
            call(G)
    D = atlas.graph('directed', 'perm')
    with pytest.raises(nx.NetworkXError, match='Found infinite path length because the digraph is not strongly'):
        ga.eccentricity(D)


# -------------------------------------------------------------------------------------------------- directed union
@RELABEL
def test_catalogue_of_the_directed_union(relabel):
    """Every name of available_measures(True, False) on the seeded orientation (u -> v, v -> u or both per edge)."""
    run = functools.partial(_run_catalogue, 'directed')
    got = _got('catalogue_directed', relabel, run)
    D = atlas.graph('directed', 'identity')
    assert [k for k in got if k != 'iterations'] == ['degree', 'weighted_degree', 'in_degree', 'out_degree', 'pagerank',
                                                     'eigenvector']
    _exact(got['degree'], _col(dict(D.degree())), 'degree')
    _exact(got['weighted_degree'], _col(dict(D.degree(weight='weight'))), 'weighted_degree')
    _exact(got['in_degree'], _col(dict(D.in_degree())), 'in_degree')
    _exact(got['out_degree'], _col(dict(D.out_degree())), 'out_degree')
    pr, pr_it, ev, ev_it = _want_power('directed')
    assert got['iterations'] == {'pagerank': pr_it, 'eigenvector': ev_it}
    _close(got['pagerank'], pr, mo.RTOL, 'pagerank')
    _close(got['eigenvector'], ev, mo.RTOL, 'eigenvector')
    _equivariant('catalogue_directed', run,
                 bitwise=('degree', 'weighted_degree', 'in_degree', 'out_degree', 'iterations'),
                 close={'pagerank': mo.RTOL, 'eigenvector': mo.RTOL})


def _run_directed(relabel):
    from graphrole_amd import betweenness_centrality, clustering
    D = atlas.graph('directed', relabel)
    return {'betweenness': _rows(betweenness_centrality(D, normalized=False), relabel),
            'clustering': _rows(clustering(D), relabel)}


@RELABEL
def test_directed_betweenness_and_directed_clustering(relabel):
    """Betweenness: tolerance class.  Fagiolo's clustering without weights is a ratio of integers: bitwise class."""
    got = _got('directed', relabel, _run_directed)
    _close(got['betweenness'], atlas.load()['betweenness_directed'], bo.RTOL, 'directed betweenness')
    want = np.array([float(x) for x in _col(nx.clustering(atlas.graph('directed', 'identity')))])
    clo.assert_close(got['clustering'], want, 'directed clustering')
    _exact(got['clustering'], want, 'directed clustering')      # integers only: networkx bit for bit
    _equivariant('directed', _run_directed, bitwise=('clustering',), close={'betweenness': bo.RTOL})


def _bow_tie_by_definition(D, index):
    """The six categories from nx.strongly_connected_components, nx.descendants and nx.ancestors; S = the largest
    component, ties by first member in the index."""
    S = min(nx.strongly_connected_components(D), key=lambda c: (-len(c), min(c)))
    anc = set().union(*(nx.ancestors(D, v) for v in S)) - S
    des = set().union(*(nx.descendants(D, v) for v in S)) - S
    from_in = set(anc).union(*(nx.descendants(D, v) for v in anc)) if anc else set()
    to_out = set(des).union(*(nx.ancestors(D, v) for v in des)) if des else set()
    code = np.full(len(index), 5, dtype=np.int8)
    for i, v in enumerate(index):
        if v in S:
            code[i] = 0
        elif v in anc:
            code[i] = 1
        elif v in des:
            code[i] = 2
        elif v in from_in and v in to_out:
            code[i] = 3
        elif v in from_in or v in to_out:
            code[i] = 4
    return code


@RELABEL
def test_strong_and_weak_components_and_bow_tie(relabel):
    """Trim / colour / close rounds over every orientation pattern of every small graph at once.  Both relabellings are
    held against the same networkx partitions placed by label (the equivariance of the partitions); the bow tie hangs
    on WHICH of the equally large strong components comes first in the index, so it is checked against its definition
    per relabelling."""
    import graphrole_amd as ga
    D = atlas.graph('directed', relabel)
    D0 = atlas.graph('directed', 'identity')
    weak = _labelled(nx.weakly_connected_components(D0), relabel)
    strong = _labelled(nx.strongly_connected_components(D0), relabel)
    got_weak, got_strong = ga.weakly_connected_components(D), ga.strongly_connected_components(D)
    assert got_weak == weak and got_strong == strong
    assert len(weak) == 1610 and ga.number_weakly_connected_components(D) == 1610
    assert ga.number_strongly_connected_components(D) == len(strong)
    assert ga.is_weakly_connected(D) is False and ga.is_strongly_connected(D) is False
    _check_table(ga.component_table(D), weak, 1610)
    table = ga.component_table(D, kind='strong')
    ranked = _check_table(table, strong, len(strong))
    assert table.attrs['rounds'] >= 1
    assert list(ga.largest_component(D, kind='strong')) == sorted(ranked[0])
    tie = ga.bow_tie(D)
    want = _bow_tie_by_definition(D, range(N))
    assert np.array_equal(np.asarray(tie.index), np.arange(N))
    _exact(tie.cat.codes.to_numpy(), want, 'bow_tie')
    assert tie.attrs['sizes'] == {c: int((want == k).sum()) for k, c in enumerate(tie.cat.categories)}


@RELABEL
def test_descendants_and_ancestors_of_64_sources(relabel):
    import graphrole_amd as ga
    D = atlas.graph('directed', relabel)
    label = atlas.relabelling(relabel)
    for v in label[_sources()].tolist():
        assert ga.descendants(D, v) == nx.descendants(D, v), v
        assert ga.ancestors(D, v) == nx.ancestors(D, v), v


# -------------------------------------------------------------------------------------------------- weighted union
def _run_weighted_betweenness(relabel):
    from graphrole_amd import weighted_betweenness_centrality
    W = atlas.graph('weighted', relabel)
    return {'betweenness': _rows(weighted_betweenness_centrality(W, normalized=False), relabel)}


@RELABEL
def test_weighted_betweenness_from_all_sources(relabel):
    """Integer weights 1 .. 3: equally light paths of different hop counts in a large share of the components
    (tests/test_atlas_cpu.py counts them) -- the tie logic ``uneven_ties`` tests on one graph.  Tolerance class."""
    got = _got('weighted_betweenness', relabel, _run_weighted_betweenness)
    _close(got['betweenness'], atlas.load()['betweenness_weighted'], wo.RTOL, 'weighted betweenness')
    _equivariant('weighted_betweenness', _run_weighted_betweenness, close={'betweenness': wo.RTOL})


def _run_distances(relabel):
    from graphrole_amd import dijkstra_path_lengths
    W = atlas.graph('weighted', relabel)
    label = atlas.relabelling(relabel)
    frame = dijkstra_path_lengths(W, sources=label[_sources()].tolist())
    assert list(frame.index) == label[_sources()].tolist() and np.array_equal(np.asarray(frame.columns), np.arange(N))
    return {'dist': np.ascontiguousarray(frame.to_numpy()[:, label])}


@RELABEL
def test_dijkstra_path_lengths_of_64_sources(relabel):
    """Bit for bit networkx's Dijkstra distances (sums of small integers), inf outside the source's component."""
    got = _got('distances', relabel, _run_distances)
    want = so.networkx_matrix(atlas.graph('weighted', 'identity'), _sources().tolist())
    assert np.isinf(want).any() and np.array_equal(got['dist'], want)
    _equivariant('distances', _run_distances, bitwise=('dist',))


def _run_weighted(relabel):
    from graphrole_amd import clustering, constraint, effective_size, node_measures
    W = atlas.graph('weighted', relabel)
    return {'clustering': _rows(clustering(W, weight='weight'), relabel),
            'constraint': _rows(constraint(W, weight='weight'), relabel),
            'effective_size': _rows(effective_size(W, weight='weight'), relabel),
            'closeness': _rows(node_measures(W, ['closeness_centrality'], distance='weight')['closeness_centrality'],
                               relabel)}


@RELABEL
def test_weighted_clustering_structural_holes_and_closeness(relabel):
    """clustering(weight=), constraint(weight=), effective_size(weight=) and closeness by weight.  Tolerance class for
    the first three (cube roots and quotients added in arc order); closeness by weight is three IEEE operations on
    exact sums of small integers: bitwise class."""
    got = _got('weighted', relabel, _run_weighted)
    W = atlas.graph('weighted', 'identity')
    want = np.array([float(x) for x in _col(nx.clustering(W, weight='weight'))])
    clo.assert_close(got['clustering'], want, 'weighted clustering')
    _check_structural_holes(got, '_weighted')
    _close(got['closeness'], _col(nx.closeness_centrality(W, distance='weight')), so.RTOL, 'closeness by weight')
    _equivariant('weighted', _run_weighted, bitwise=('closeness',),
                 close={'clustering': clo.RTOL, 'constraint': sho.RTOL, 'effective_size': _effective_size_close})


# ------------------------------------------------------------------------------------- generation-0 ReFeX features
@RELABEL
def test_generation_0_features_on_the_union(relabel):
    """kernels.row_sums, egonet_features (both kernels) and triangle_counts on the union's CSR against oracle.refex, as
    tests/test_gpu_kernels.py::test_row_sums_and_egonet_vs_oracle; the triangle counts against networkx."""
    from graphrole_amd import kernels as K
    from oracle import refex
    label = atlas.relabelling(relabel)
    src, dst, _ = atlas.arcs('undirected')
    og = refex.graph_from_arrays(N, label[src], label[dst], None, False)
    csr = K.DeviceCSR(og.row_ptr, og.col, og.w, agg_col=og.adj_col)
    loc, ego = refex.local_features_c(og), refex.egonet_features_c(og)
    assert np.array_equal(K.row_sums(csr, True).cpu().numpy()[:N], loc['degree'])
    for internal, external in (K.egonet_features(csr, False), K.egonet_features_general(csr, False)):
        assert np.array_equal(internal.cpu().numpy()[:N], ego['internal_edges'])
        assert np.array_equal(external.cpu().numpy()[:N], ego['external_edges'])
    T = K.triangle_counts(csr).cpu().numpy()[:N].astype(np.int64)
    want = _col(nx.triangles(atlas.graph('undirected', 'identity')))
    _exact(T[label], want, 'triangle_counts')


# ------------------------------------------------------------------------------------------------ cone over the atlas
@functools.lru_cache(maxsize=None)
def _want_cone():
    """networkx on the 'identity' cone, in atlas order with the apex last; the truss numbers one small cone at a time
    (see the module docstring): (edge truss over the fixture's edges, apex-edge truss per atlas node, node truss)."""
    C = atlas.cone('identity')
    n1 = N + 1
    col = lambda d: atlas.of_dict(d, range(n1))                 # noqa: E731
    src, dst, _ = atlas.arcs('undirected')
    first, _ = atlas.bounds()
    owner = np.searchsorted(first, src, side='right') - 1
    edge = np.zeros(len(src), dtype=np.int64)
    spoke = np.zeros(N, dtype=np.int64)
    node = np.zeros(n1, dtype=np.int64)
    by_owner = np.argsort(owner, kind='stable')
    cuts = np.searchsorted(owner[by_owner], np.arange(len(first) + 1))
    for i, (_, lo, G) in enumerate(atlas.small_graphs()):
        k = G.number_of_nodes()
        H = G.copy()
        H.add_edges_from((k, v) for v in range(k))
        edge_t, node_t = to.networkx_truss_numbers(H)
        for e in by_owner[cuts[i]:cuts[i + 1]].tolist():
            edge[e] = edge_t[frozenset((int(src[e]) - lo, int(dst[e]) - lo))]
        for v in range(k):
            spoke[lo + v] = edge_t[frozenset((k, v))]
            node[lo + v] = node_t[v]
        node[N] = max(node[N], node_t[k])
    blocks = frozenset(frozenset(c) for c in nx.biconnected_components(C))
    return dict(triangles=col(nx.triangles(C)), clustering=col(nx.clustering(C)), core=col(nx.core_number(C)),
                edge_truss=edge, spoke_truss=spoke, node_truss=node, blocks=blocks,
                points=sorted(nx.articulation_points(C)))


def _cone_labels(relabel):
    return np.concatenate([atlas.relabelling(relabel), [N]])


def _cone_csr(relabel):
    """(row_ptr, col) of the cone with the rows in label order."""
    from tests.kcore_oracle import symmetric_csr
    label = _cone_labels(relabel)
    src, dst, _ = atlas.arcs('undirected')
    edges = np.concatenate([np.stack([label[src], label[dst]], axis=1),
                            np.stack([np.full(N, N), np.arange(N)], axis=1)])
    return symmetric_csr(N + 1, edges)


def _cone_arc_truss(row_ptr, col, relabel):
    """The reference truss number of every arc of ``_cone_csr``."""
    want = _want_cone()
    label = _cone_labels(relabel)
    src, dst, _ = atlas.arcs('undirected')
    n1 = N + 1
    key = np.concatenate([label[src] * n1 + label[dst], label[dst] * n1 + label[src],
                          N * n1 + label[:N], label[:N] * n1 + N])
    val = np.concatenate([want['edge_truss'], want['edge_truss'], want['spoke_truss'], want['spoke_truss']])
    order = np.argsort(key)
    rows = np.repeat(np.arange(n1, dtype=np.int64), np.diff(row_ptr))
    have = rows * n1 + np.asarray(col, dtype=np.int64)
    assert np.array_equal(key[order], have)
    return val[order]


@RELABEL
def test_cone_public_functions(relabel):
    """The union plus one apex joined to all 8475 nodes: the apex row takes the hub launches, and every row
    intersection pairs that hub row with a short row.  The apex is the only articulation point, with one block per
    former component."""
    import graphrole_amd as ga
    C = atlas.cone(relabel)
    want = _want_cone()
    label = _cone_labels(relabel)
    back = lambda s: s.to_numpy()[label]                        # noqa: E731
    _exact(back(ga.clustering(C)), want['clustering'], 'clustering')
    _exact(back(ga.core_number(C)), want['core'], 'core_number')
    _exact(back(ga.node_truss_number(C)), want['node_truss'], 'node_truss_number')
    t = ga.truss_number(C)
    u, v = t.index.get_level_values('u').to_numpy(), t.index.get_level_values('v').to_numpy()
    inv = np.empty(N + 1, dtype=np.int64)
    inv[label] = np.arange(N + 1)
    a, b = inv[u], inv[v]                                       # the edge's ends in atlas ids (the apex: N)
    got = dict(zip(zip(np.minimum(a, b).tolist(), np.maximum(a, b).tolist()), t.to_numpy().tolist()))
    src, dst, _ = atlas.arcs('undirected')
    expect = dict(zip(zip(np.minimum(src, dst).tolist(), np.maximum(src, dst).tolist()), want['edge_truss'].tolist()))
    expect.update(zip(zip(range(N), [N] * N), want['spoke_truss'].tolist()))
    assert got == expect
    assert ga.articulation_points(C) == [N] == want['points']
    blocks = frozenset(frozenset(inv[list(b)].tolist()) for b in ga.biconnected_components(C))
    assert blocks == want['blocks'] and len(blocks) == 1610 and all(N in b for b in blocks)
    counts = back(ga.biconnected_component_counts(C))
    assert counts[N] == 1610 and np.all(counts[:N] == 1)
    assert ga.connected_components(C) == [set(range(N + 1))] and ga.is_connected(C) is True


@RELABEL
@pytest.mark.parametrize('lanes', LANES)
def test_cone_kernels_at_both_lane_widths(relabel, lanes):
    """The kernels that take `lanes`, with the hub list of that width (the apex row of 8475 arcs is a hub at 4 lanes,
    above 128 arcs, and at 32 lanes, above 1024), and the triangle counts, on the cone's CSR in label order."""
    from graphrole_amd import kernels as K
    row_ptr, col = _cone_csr(relabel)
    csr = K.DeviceCSR(row_ptr, col)
    assert K._hubs_for(csr, lanes)[1] == 1
    want = _want_cone()
    label = _cone_labels(relabel)
    n1 = N + 1
    _exact(K.to_host(K.triangle_counts(csr))[:n1].astype(np.int64)[label], want['triangles'], 'triangle_counts')
    cl, tri = K.clustering(csr, want_triangles=True, lanes=lanes)
    _exact(K.to_host(cl)[:n1][label], want['clustering'], 'clustering')
    _exact(K.to_host(tri)[:n1][label], 2.0 * want['triangles'], 'clustering numerator')
    arc, node, _, _ = K.truss_numbers(csr, lanes=lanes)
    _exact(K.to_host(arc)[:len(col)].astype(np.int64), _cone_arc_truss(row_ptr, col, relabel), 'arc truss')
    _exact(K.to_host(node)[:n1][label], want['node_truss'], 'node truss')
    lab, size, n_components, _ = K.components(csr, lanes=lanes)
    assert n_components == 1 and not K.to_host(lab)[:n1].any() and np.all(K.to_host(size)[:n1] == n1)
    core, _, _ = K.core_numbers(csr)
    _exact(K.to_host(core)[:n1][label], want['core'], 'core')
