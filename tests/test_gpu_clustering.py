"""
The weighted and the directed clustering coefficient on the MI355X.  Kernel parity: kernels.clustering (grx_clustering)
against the `exact` restatement of tests/clustering_oracle.py -- the coefficient and its numerator t, each unweighted,
with integer and with float weights -- at the smallest shapes that reach each code path: one to three nodes, rows longer
than a wavefront, empty intersections, a hub arc list, the hub threshold of every lane width, self-loops, isolated rows,
a directed graph with both value arrays, zero weights; the second trip of the grid-stride loops against the `sparse`
restatement; the bits that must not move.  API parity: graphrole_amd's clustering and average_clustering against
networkx itself.  Tolerances: tests/clustering_oracle.py.
"""
import functools
import random

import networkx as nx
import numpy as np
import pytest

from tests import clustering_oracle as co
from tests.rowjoin_graphs import WEIGHTS, _ba60000, _digraph, _named_pairs, _pairs_of, _threshold_pairs

pytestmark = pytest.mark.gpu


def _run(row_ptr, col, fwd=None, bwd=None, max_weight=1.0, lanes=None, want_triangles=True):
    """One kernel call on the CSR arrays: host (clustering, t or None)."""
    from graphrole_amd import kernels as K
    n = len(row_ptr) - 1
    csr = K.DeviceCSR(row_ptr, col, fwd)
    b = None if bwd is None else K.to_device(np.ascontiguousarray(bwd if len(bwd) else np.zeros(1), dtype=np.float64))
    c, t = K.clustering(csr, csr.w, b, max_weight, want_triangles=want_triangles, lanes=lanes)
    return K.to_host(c)[:n].copy(), None if t is None else K.to_host(t)[:n].copy()


def _check(row_ptr, col, fwd=None, bwd=None, max_weight=1.0, lanes=None, what=''):
    assert int(np.max(np.diff(row_ptr), initial=0)) <= co.MAX_ROW      # the rows the tolerance was derived for
    got = _run(row_ptr, col, fwd, bwd, max_weight, lanes)
    want = co.exact(row_ptr, col, fwd, bwd, max_weight)
    co.assert_close(got[0], want[0], (what, 'clustering'))
    co.assert_close(got[1], want[1], (what, 't'))
    if fwd is None:
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])      # integers only
    return got


@functools.lru_cache(maxsize=None)
def _named_case(key, weights):
    """(arrays of the kernel, the exact oracle's result), computed once per case."""
    n, pairs = _named_pairs(key)
    arrays = co.csr_from_pairs(n, pairs, WEIGHTS[weights])
    return arrays, co.exact(arrays[0], arrays[1], arrays[2], None, arrays[3])


@pytest.mark.parametrize('weights', list(WEIGHTS))
@pytest.mark.parametrize('key', ['n1', 'n1_loop', 'n2', 'n3_path', 'n3_triangle', 'path', 'star1500', 'K70', 'K40_40',
                                 'wheel1500', 'ba2000'])
def test_kernel_against_the_exact_oracle(key, weights):
    from graphrole_amd import kernels as K
    (row_ptr, col, fwd, max_weight), want = _named_case(key, weights)
    assert int(np.max(np.diff(row_ptr), initial=0)) <= co.MAX_ROW
    if key in ('star1500', 'wheel1500'):
        assert K.DeviceCSR(row_ptr, col).n_hubs == 1            # the centre goes through the hub launches
    got = _run(row_ptr, col, fwd, None, max_weight)
    co.assert_close(got[0], want[0], (key, weights, 'clustering'))
    co.assert_close(got[1], want[1], (key, weights, 't'))
    if key == 'K70' and weights == 'unweighted':
        assert np.all(got[0] == 1.0) and np.all(got[1] == 69 * 68)
    if key in ('star1500', 'K40_40', 'path', 'n1', 'n1_loop', 'n2', 'n3_path'):
        assert np.all(got[0] == 0.0) and np.all(got[1] == 0.0)


@pytest.mark.parametrize('weights', list(WEIGHTS))
@pytest.mark.parametrize('lanes', [4, 8, 16, 32])
def test_hub_threshold_of_every_lane_width(lanes, weights):
    from graphrole_amd import kernels as K
    for entries in (K.HUB_FACTOR * lanes - 1, K.HUB_FACTOR * lanes, K.HUB_FACTOR * lanes + 1):
        n, pairs = _threshold_pairs(entries)
        row_ptr, col, fwd, max_weight = co.csr_from_pairs(n, pairs, WEIGHTS[weights])
        assert int(np.diff(row_ptr).max()) == entries == row_ptr[1]
        n_hubs = K._hubs_for(K.DeviceCSR(row_ptr, col), lanes)[1]
        assert n_hubs == (1 if entries > K.HUB_FACTOR * lanes else 0)       # a hub row exactly where one is meant
        got = _check(row_ptr, col, fwd, None, max_weight, lanes=lanes, what=(lanes, entries, weights))
        assert got[0][0] > 0.0


@pytest.mark.parametrize('weights', list(WEIGHTS))
def test_self_loops_and_isolated_rows(weights):
    G = nx.gnp_random_graph(60, 0.12, seed=11)
    loops = [(v, v) for v in (0, 5, 17, 59)] + [(61, 61)]       # 60 and 62 isolated, 61 only its loop
    w_of = WEIGHTS[weights]
    # the loops weigh little, so that the maximum -- which they count in -- is the same with and without them
    light = None if w_of is None else (lambda a, b: 0.05 if a == b else w_of(a, b))
    plain = co.csr_from_pairs(63, _pairs_of(G), light)
    looped = co.csr_from_pairs(63, _pairs_of(G) + loops, light)
    assert looped[3] == plain[3] and looped[0][-1] == plain[0][-1] + len(loops)
    a = _check(plain[0], plain[1], plain[2], None, plain[3], what=(weights, 'plain'))
    b = _check(looped[0], looped[1], looped[2], None, looped[3], what=(weights, 'looped'))
    # a loop changes neither degree nor triangles (with weights it moves the arcs to other lanes: another sum order)
    for x, y in zip(a, b):
        if w_of is None:
            assert np.array_equal(x, y)
        else:
            co.assert_close(x, y, (weights, 'loops'))
    assert b[0][60] == 0.0 and b[0][61] == 0.0 and b[0][62] == 0.0 and np.any(b[0] > 0)


@pytest.mark.parametrize('weight', [None, 'weight'])
def test_directed_graph_with_both_value_arrays(weight):
    D = _digraph()
    row_ptr, col, fwd, bwd, max_weight = co.directional_csr(D, weight)
    assert np.any(fwd < 0) and np.any(bwd < 0) and np.any((fwd >= 0) & (bwd >= 0))
    c, t = _check(row_ptr, col, fwd, bwd, max_weight, what=weight)
    want = nx.clustering(D, weight=weight)
    want = np.array([want[v] for v in sorted(D)], dtype=np.float64)
    co.assert_close(c, want, 'networkx')
    assert c[42] == 0.0 and np.count_nonzero(c) > 30
    if weight is None:
        assert np.array_equal(c, want)                          # integers only: networkx bit for bit


def test_zero_weights():
    G = nx.gnp_random_graph(30, 0.3, seed=9)
    G.add_edges_from([(0, 1), (0, 2), (1, 2)])
    dead = 0                                                    # every edge at node 0 weighs 0
    row_ptr, col, fwd, max_weight = co.csr_from_pairs(30, _pairs_of(G),
                                                      lambda a, b: 0.0 if dead in (a, b) else 1.5 + a % 3)
    plain = co.csr_from_pairs(30, _pairs_of(G))
    c, t = _check(row_ptr, col, fwd, None, max_weight)
    assert _run(plain[0], plain[1])[0][dead] > 0.0              # node 0 does lie in triangles
    assert c[dead] == 0.0 and t[dead] == 0.0                    # each of which holds a zero-weight edge
    want = nx.Graph()
    want.add_nodes_from(range(30))
    want.add_weighted_edges_from((u, v, 0.0 if dead in (u, v) else 1.5 + min(u, v) % 3) for u, v in G.edges)
    ref = nx.clustering(want, weight='weight')
    co.assert_close(c, np.array([ref[v] for v in range(30)], dtype=np.float64), 'networkx')
    # a real zero-weight arc still counts in d and dt: 1 -> 2 weighs 0 and is not absent
    D = nx.DiGraph()
    D.add_weighted_edges_from([(0, 1, 2.0), (1, 2, 0.0), (2, 0, 1.0), (0, 3, 1.0), (3, 1, 4.0), (1, 0, 1.0)])
    a = co.directional_csr(D, 'weight')
    c, t = _check(*a, what='zero arc')
    ref = nx.clustering(D, weight='weight')
    co.assert_close(c, np.array([ref[v] for v in sorted(D)], dtype=np.float64), 'networkx digraph')
    absent = nx.DiGraph(D)
    absent.remove_edge(1, 2)
    c2, t2 = _check(*co.directional_csr(absent, 'weight'), what='absent arc')
    assert t2[1] == t[1] and c2[1] > c[1] > 0                   # the same triangles over a smaller denominator


def test_second_trip_of_the_grid_stride_loops():
    """BA 60 000 / m = 5 against the sparse oracle.  With 32 lanes a workgroup pass takes RJ_BLOCK / 32 = 8 rows or
    arcs, so the row kernels (cap RJ_ROW_MAX_WG) and the per-arc kernel (cap RJ_ARC_MAX_WG) both wrap; with the CSR's
    own 4 lanes the per-arc kernel wraps.  (Every other second-trip test of the suite is listed at the top of
    tests/test_gpu_second_trip.py.)"""
    from graphrole_amd import kernels as K
    n, row_ptr, col, fwd = _ba60000()
    nnz = len(col)
    assert int(np.diff(row_ptr).max()) <= co.MAX_ROW
    assert n > K.RJ_ROW_MAX_WG * (K.RJ_BLOCK // 32) and nnz > K.RJ_ARC_MAX_WG * (K.RJ_BLOCK // 32)
    csr = K.DeviceCSR(row_ptr, col)
    assert nnz > K.RJ_ARC_MAX_WG * (K.RJ_BLOCK // csr.lanes_per_row) and csr.n_hubs > 0
    max_weight = float(fwd.max())
    want = co.sparse(row_ptr, col, fwd, None, max_weight)
    for lanes in (32, None):
        got = _run(row_ptr, col, fwd, None, max_weight, lanes=lanes)
        co.assert_close(got[0], want[0], ('lanes', lanes, 'clustering'))
        co.assert_close(got[1], want[1], ('lanes', lanes, 't'))


def test_bits_that_must_not_move():
    from graphrole_amd import kernels as K
    for key in ('ba2000', 'wheel1500'):                         # without and with a hub row
        (row_ptr, col, fwd, max_weight), _ = _named_case(key, 'float')
        both = _run(row_ptr, col, fwd, None, max_weight)
        again = _run(row_ptr, col, fwd, None, max_weight)
        assert np.array_equal(both[0], again[0]) and np.array_equal(both[1], again[1])
        alone = _run(row_ptr, col, fwd, None, max_weight, want_triangles=False)
        assert alone[1] is None and np.array_equal(alone[0], both[0])
        # no weights: the bits of the existing 'clustering' column; constant weights: the same bits again
        n = len(row_ptr) - 1
        plain = _run(row_ptr, col)
        csr = K.DeviceCSR(row_ptr, col)
        old = K.to_host(K.local_structure(csr, K.triangle_counts(csr), False)[0])[:n]
        assert np.array_equal(plain[0], old)
        for constant in (1.0, 3.0, 0.1):
            same = _run(row_ptr, col, np.full(len(col), constant), None, constant)
            assert np.array_equal(same[0], plain[0]) and np.array_equal(same[1], plain[1])
    D = _digraph()                                              # and of a directed graph
    row_ptr, col, fwd, bwd, _ = co.directional_csr(D, None)
    plain = _run(row_ptr, col, fwd, bwd, 1.0)
    same = _run(row_ptr, col, np.where(fwd >= 0, 0.3, -1.0), np.where(bwd >= 0, 0.3, -1.0), 0.3)
    assert np.array_equal(same[0], plain[0]) and np.array_equal(same[1], plain[1])


# ------------------------------------------------------------------------------------------------------ API level
def _against_networkx(G, weight):
    from graphrole_amd import average_clustering, clustering
    nodes = sorted(G)
    got, want = clustering(G, weight=weight), nx.clustering(G, weight=weight)
    assert list(got.index) == nodes and got.name == 'clustering' and got.dtype == np.float64
    ref = np.array([want[v] for v in nodes], dtype=np.float64)
    co.assert_close(got.to_numpy(), ref, ('clustering', weight))
    if weight is None:
        assert np.array_equal(got.to_numpy(), ref)
    for count_zeros in (True, False):
        a = average_clustering(G, weight=weight, count_zeros=count_zeros)
        b = nx.average_clustering(G, weight=weight, count_zeros=count_zeros)
        assert abs(a - b) <= co.RTOL * b


@pytest.mark.parametrize('weight', [None, 'weight'])
def test_api_against_networkx(weight):
    _against_networkx(nx.karate_club_graph(), weight)
    D = nx.gnm_random_graph(25, 90, seed=3, directed=True)
    rng = random.Random(3)
    for u, v in D.edges:
        D[u][v]['weight'] = rng.choice([0.5, 1.0, 2.0, 7.25])
    D.add_edge(3, 3, weight=11.5)                               # the heaviest edge is a loop
    _against_networkx(D, weight)
    L = nx.gnp_random_graph(20, 0.3, seed=6)
    L.add_edges_from([(0, 0), (7, 7), (19, 19)])
    _against_networkx(L, weight)


def test_csr_graph_input_gives_the_same_bits():
    from graphrole_amd import clustering
    from graphrole_amd.graph.csr import CSRGraph
    G = nx.karate_club_graph()
    src, dst, w = zip(*G.edges(data='weight'))
    C = CSRGraph(34, src, dst, weights=np.asarray(w, dtype=np.float64))
    for weight in (None, 'weight'):
        assert np.array_equal(clustering(C, weight=weight).to_numpy(), clustering(G, weight=weight).to_numpy())
    D = _digraph()
    src, dst, w = zip(*D.edges(data='weight'))
    C = CSRGraph(D.number_of_nodes(), src, dst, weights=np.asarray(w), directed=True)
    for weight in (None, 'weight'):
        assert np.array_equal(clustering(C, weight=weight).to_numpy(), clustering(D, weight=weight).to_numpy())
    got = clustering(G, nodes=[33, 0, 5], weight='weight')
    assert list(got.index) == [0, 5, 33]
    assert np.array_equal(got.to_numpy(), clustering(G, weight='weight').to_numpy()[[0, 5, 33]])


def test_node_measures_columns_and_sense_making_on_karate():
    from graphrole_amd import RecursiveFeatureExtractor, RoleExtractor, clustering, node_measures
    G = nx.karate_club_graph()
    M = node_measures(G, ['clustering', 'degree'], clustering_weight='weight')
    assert list(M.columns) == ['clustering', 'degree'] and list(M.index) == sorted(G)
    assert np.array_equal(M['clustering'].to_numpy(), clustering(G, weight='weight').to_numpy())
    assert M['degree'].to_dict() == dict(G.degree())
    plain = node_measures(G, ['clustering'])['clustering'].to_numpy()     # without the keyword: as it always was
    want = nx.clustering(G)
    assert np.array_equal(plain, np.array([want[v] for v in sorted(G)]))
    assert not np.array_equal(plain, M['clustering'].to_numpy())
    with pytest.raises(NotImplementedError, match='nx.clustering'):
        node_measures(nx.DiGraph(G), ['clustering'])
    features = RecursiveFeatureExtractor(G).extract_features()
    np.random.seed(0)
    roles = RoleExtractor(n_roles=3)
    roles.extract_role_factors(features)
    E = roles.sense_making(M)
    assert list(E.columns) == ['clustering', 'degree'] and np.all(E.to_numpy() >= 0)
