"""
Eccentricity on the MI355X.  Kernel parity: kernels.eccentricity_pass (grx_eccentricity) against the numpy restatement
of tests/eccentricity_oracle.py, all four arrays bit-equal, at the smallest shapes that reach each code path -- the
level-batch boundaries of the round loop, a hub row, every source width with partial words and batches, repeated and
out-of-range sources, bounds carried across calls, and the call without upper bounds.  API parity: graphrole_amd's
eccentricity (both methods), diameter, radius, center, periphery and the node_measures column equal to networkx.
"""
import functools

import networkx as nx
import numpy as np
import pytest

from tests import eccentricity_oracle as eo

pytestmark = pytest.mark.gpu


def _pass(row_ptr, col, sources, words, bounds=None, want_upper=False):
    """One kernel call on the CSR arrays: (host arrays, device (lower, upper))."""
    from graphrole_amd import kernels as K
    n = len(row_ptr) - 1
    csr = K.DeviceCSR(row_ptr, col)
    ecc, reach, lower, upper = K.eccentricity_pass(csr, np.asarray(sources), words, bounds=bounds,
                                                   want_upper=want_upper)
    host = (K.to_host(ecc), K.to_host(reach)[:n], K.to_host(lower)[:n], None if upper is None else K.to_host(upper)[:n])
    return host, (lower, upper)


def _same(got, want):
    for name, g, w in zip(('source_ecc', 'reach', 'lower', 'upper'), got, want):
        if w is None:
            assert g is None, name
            continue
        assert g.dtype == w.dtype, name
        assert np.array_equal(g, w), (name, np.nonzero(g != w)[0][:8], g[:8], w[:8])


def _check(row_ptr, col, sources, words, want_upper=True):
    got, _ = _pass(row_ptr, col, sources, words, want_upper=want_upper)
    _same(got, eo.eccentricity_pass(row_ptr, col, sources, want_upper=want_upper))


def _directed_cycle_pull(k):
    """The in-adjacency of the directed cycle 0 -> 1 -> ... -> k - 1 -> 0 (k = 1: one node, no arc)."""
    if k == 1:
        return np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.arange(k + 1, dtype=np.int64), (np.arange(k, dtype=np.int64) - 1) % k


@pytest.mark.parametrize('lo', [1, 11, 21, 31])
def test_paths_and_directed_cycles_across_the_level_batches(lo):
    # k - 1 levels from an end: the read-backs of the round loop fall at 8, 16, 24 and 32 levels
    for k in range(lo, lo + 10):
        row_ptr, col = eo.csr_of(nx.path_graph(k), list(range(k)))
        _check(row_ptr, col, np.arange(k), 1)
        _check(*_directed_cycle_pull(k), np.arange(k), 1)


@pytest.mark.parametrize('words', [1, 16])
def test_star_with_a_hub_row(words):
    from graphrole_amd import kernels as K
    probe = K.DeviceCSR(*eo.csr_of(nx.star_graph(8), list(range(9))))
    leaves = K.HUB_FACTOR * probe.lanes_per_row + 5            # the centre row is longer than the hub threshold
    row_ptr, col = eo.csr_of(nx.star_graph(leaves), list(range(leaves + 1)))
    csr = K.DeviceCSR(row_ptr, col)
    assert csr.lanes_per_row == probe.lanes_per_row and csr.n_hubs == 1
    assert row_ptr[1] - row_ptr[0] > K.HUB_FACTOR * csr.lanes_per_row
    _check(row_ptr, col, [0, 3, 9, leaves], words)              # the centre is a source
    _check(row_ptr, col, [1, 2, 70, leaves], words)             # it is not
    _check(row_ptr, col, np.arange(leaves + 1), words)          # every node: several batches at W = 1


@functools.lru_cache(maxsize=None)
def _width_graph(kind):
    if kind == 'ba':
        G = nx.barabasi_albert_graph(200, 2, seed=5)
    else:
        G = nx.convert_node_labels_to_integers(nx.grid_2d_graph(15, 15))   # 28 levels
    n = G.number_of_nodes()
    row_ptr, col = eo.csr_of(G, list(range(n)))
    order = np.random.default_rng(1).permutation(n)
    return row_ptr, col, order


@pytest.mark.parametrize('kind', ['ba', 'grid'])
@pytest.mark.parametrize('count', [1, 63, 64, 65, 130])
def test_every_width_with_partial_words_and_batches(kind, count):
    row_ptr, col, order = _width_graph(kind)
    want = eo.eccentricity_pass(row_ptr, col, order[:count], want_upper=True)
    for words in (1, 2, 16):
        got, _ = _pass(row_ptr, col, order[:count], words, want_upper=True)
        _same(got, want)


def test_repeated_and_out_of_range_sources():
    row_ptr, col, order = _width_graph('ba')
    n = len(row_ptr) - 1
    repeated = np.concatenate([order[:40], order[:40], [order[0]] * 5])     # 85 lanes, one node up to 7 times
    outside = np.array([3, -1, n, 7, 2 ** 31 - 1, -7, 3])
    for words in (1, 2):
        _check(row_ptr, col, repeated, words)
        _check(row_ptr, col, outside, words)
    got, _ = _pass(row_ptr, col, [-1, n], 1, want_upper=True)  # no valid source: nothing is written through
    assert got[0].tolist() == [0, 0] and not got[1].any() and not got[2].any() and np.all(got[3] == eo.INF)


def test_bounds_carried_across_two_calls():
    row_ptr, col, order = _width_graph('grid')
    first, second = order[:70], order[70:100]
    want1 = eo.eccentricity_pass(row_ptr, col, first, want_upper=True)
    want2 = eo.eccentricity_pass(row_ptr, col, second, want1[2], want1[3])
    got1, bounds = _pass(row_ptr, col, first, 1, want_upper=True)          # accumulate = 0
    _same(got1, want1)
    got2, _ = _pass(row_ptr, col, second, 1, bounds=bounds)                # accumulate = 1
    _same(got2, want2)
    assert np.all(got2[2] >= got1[2]) and np.all(got2[3] <= got1[3]) and np.any(got2[3] < got1[3])
    # the oracle's own two rounds of the driver, by its selection rule
    rounds = eo.bounds_rounds(row_ptr, col, 64)
    bounds = None
    for _ in range(2):
        sources, lower, upper = next(rounds)
        got, bounds = _pass(row_ptr, col, sources, 1, bounds=bounds, want_upper=True)
        assert np.array_equal(got[2], lower) and np.array_equal(got[3], upper)


def test_without_upper_there_is_no_second_pass():
    row_ptr, col, order = _width_graph('grid')
    got, _ = _pass(row_ptr, col, order[:100], 2, want_upper=False)
    want = eo.eccentricity_pass(row_ptr, col, order[:100])
    _same(got, want)
    assert got[3] is None
    D = eo.distance_table(row_ptr, col, order[:100])
    assert np.array_equal(got[2], D.max(axis=0))                # the per-target maximum distance only
    with_upper, _ = _pass(row_ptr, col, order[:100], 2, want_upper=True)
    assert np.all(with_upper[2] >= got[2]) and np.any(with_upper[2] > got[2])


# ------------------------------------------------------------------------------------------------------ public API
def _strong_digraph():
    G = nx.gnm_random_graph(200, 500, seed=5, directed=True)
    nx.add_cycle(G, range(200))
    return G


API_GRAPHS = {
    'karate': nx.karate_club_graph,
    'grid20': lambda: nx.grid_2d_graph(20, 20),
    'c17': lambda: nx.cycle_graph(17),
    'c200': lambda: nx.cycle_graph(200),                        # never prunes: four rounds at W = 1
    'tree500': lambda: nx.random_labeled_tree(500, seed=1),
    'ba2000': lambda: nx.barabasi_albert_graph(2000, 3, seed=3),
    'digraph200': _strong_digraph,
}


@functools.lru_cache(maxsize=None)
def _reference(key):
    G = API_GRAPHS[key]()
    return G, nx.eccentricity(G)


@pytest.mark.parametrize('key', list(API_GRAPHS))
def test_eccentricity_equals_networkx_by_both_methods(key):
    from graphrole_amd import eccentricity
    G, want = _reference(key)
    for method, words in (('bounds', 1), ('bounds', 0), ('all', 0)):
        got = eccentricity(G, method=method, words=words)
        assert got.name == 'eccentricity' and got.dtype == np.int64 and list(got.index) == sorted(want)
        assert got.to_dict() == want, (method, words)
        if G.is_directed():
            assert got.attrs['method'] == 'all'
    if key == 'c200':
        assert eccentricity(G, method='bounds', words=1).attrs == {'method': 'bounds', 'rounds': 4, 'sources': 200}
    if key == 'ba2000':
        assert eccentricity(G, method='bounds', words=1).attrs['sources'] < 2000     # pruned


def test_nodes_nbunches_and_the_derived_measures():
    from graphrole_amd import center, diameter, eccentricity, periphery, radius
    for key in ('grid20', 'digraph200'):
        G, want = _reference(key)
        nodes = sorted(G)
        assert eccentricity(G, v=nodes[7]) == want[nodes[7]]
        bunch = [nodes[50], nodes[3], 'nobody', nodes[120]]
        assert eccentricity(G, v=bunch).to_dict() == {v: want[v] for v in bunch if v != 'nobody'}
        assert (diameter(G), radius(G)) == (max(want.values()), min(want.values()))
        assert center(G) == sorted(nx.center(G, e=want)) and periphery(G) == sorted(nx.periphery(G, e=want))


def test_both_networkx_errors():
    from graphrole_amd import eccentricity, node_measures
    G = nx.disjoint_union(nx.barabasi_albert_graph(300, 2, seed=1), nx.cycle_graph(9))
    with pytest.raises(nx.NetworkXError) as theirs:
        nx.eccentricity(G)
    for call in (lambda: eccentricity(G), lambda: eccentricity(G, method='bounds'), lambda: eccentricity(G, v=3),
                 lambda: node_measures(G, ['eccentricity'])):
        with pytest.raises(nx.NetworkXError) as mine:
            call()
        assert str(mine.value) == str(theirs.value)
    D = _strong_digraph()
    D.add_edge(0, 500)                                          # 500 reaches nothing
    with pytest.raises(nx.NetworkXError) as theirs:
        nx.eccentricity(D)
    for call in (lambda: eccentricity(D), lambda: eccentricity(D, v=500)):
        with pytest.raises(nx.NetworkXError) as mine:
            call()
        assert str(mine.value) == str(theirs.value)
    assert eccentricity(D, v=0) == nx.eccentricity(D, v=0)     # 0 does reach every node


def test_node_measures_column():
    from graphrole_amd import closeness_centrality, eccentricity, node_measures
    for key in ('ba2000', 'digraph200'):
        G, want = _reference(key)
        M = node_measures(G, ['closeness_centrality', 'eccentricity'])
        assert list(M.columns) == ['closeness_centrality', 'eccentricity']
        assert M['eccentricity'].dtype == np.int64 and M['eccentricity'].to_dict() == want
        assert M['eccentricity'].to_numpy().tobytes() == eccentricity(G).to_numpy().tobytes()
        assert M['closeness_centrality'].to_numpy().tobytes() == closeness_centrality(G).to_numpy().tobytes()
