"""
Structural-hole measures on the MI355X.  Kernel parity: kernels.structural_holes (grx_structural_holes) against the
`exact` restatement of tests/structural_holes_oracle.py -- constraint, effective size and the per-arc local constraint,
each unweighted, with integer and with float mutual weights -- at the smallest shapes that reach each code path: one to
three nodes, rows longer than a wavefront, empty intersections, a hub arc list, the hub threshold of every lane width,
self-loops, isolated rows, the directed symmetrisation with its out-adjacency row pointers, zero row sums; the second
trip of the grid-stride loops against the `sparse` restatement; two runs bit-identical.  API parity: graphrole_amd's
constraint and effective_size against networkx itself.  Tolerances: tests/structural_holes_oracle.py.
"""
import random

import networkx as nx
import numpy as np
import pytest

from tests import structural_holes_oracle as so
from tests.rowjoin_graphs import WEIGHTS, _ba60000, _digraph, _named_pairs, _pairs_of, _threshold_pairs

pytestmark = pytest.mark.gpu


def _run(row_ptr, col, z, out_row_ptr=None, lanes=None, want=(True, True, True)):
    """One kernel call on the CSR arrays: host (constraint, effective_size, local), None where not asked for."""
    import torch
    from graphrole_amd import kernels as K
    n, nnz = len(row_ptr) - 1, int(row_ptr[-1])
    csr = K.DeviceCSR(row_ptr, col, z)
    orp = None if out_row_ptr is None else torch.from_numpy(np.ascontiguousarray(out_row_ptr)).to(K.device())
    con, es, loc = K.structural_holes(csr, csr.w, orp, want_constraint=want[0], want_effective_size=want[1],
                                      want_local=want[2], lanes=lanes)
    return (None if con is None else K.to_host(con)[:n].copy(), None if es is None else K.to_host(es)[:n].copy(),
            None if loc is None else K.to_host(loc)[:nnz].copy())


def _check(row_ptr, col, z, out_row_ptr=None, lanes=None, what=''):
    assert int(np.max(np.diff(row_ptr), initial=0)) <= so.MAX_ROW      # the rows the tolerance was derived for
    got = _run(row_ptr, col, z, out_row_ptr, lanes)
    so.assert_close(got, so.exact(row_ptr, col, z, out_row_ptr), row_ptr, what)
    return got


@pytest.mark.parametrize('weights', list(WEIGHTS))
@pytest.mark.parametrize('key', ['n1', 'n1_loop', 'n2', 'n3_path', 'n3_triangle', 'path', 'star1500', 'K70', 'K40_40',
                                 'wheel1500', 'ba2000'])
def test_kernel_against_the_exact_oracle(key, weights):
    from graphrole_amd import kernels as K
    n, pairs = _named_pairs(key)
    row_ptr, col, z = so.csr_from_pairs(n, pairs, WEIGHTS[weights])
    if key in ('star1500', 'wheel1500'):
        assert K.DeviceCSR(row_ptr, col).n_hubs == 1            # the centre goes through the hub launches
    _check(row_ptr, col, z, what=(key, weights))


@pytest.mark.parametrize('weights', list(WEIGHTS))
@pytest.mark.parametrize('lanes', [4, 8, 16, 32])
def test_hub_threshold_of_every_lane_width(lanes, weights):
    from graphrole_amd import kernels as K
    for entries in (K.HUB_FACTOR * lanes - 1, K.HUB_FACTOR * lanes, K.HUB_FACTOR * lanes + 1):
        n, pairs = _threshold_pairs(entries)
        row_ptr, col, z = so.csr_from_pairs(n, pairs, WEIGHTS[weights])
        assert int(np.diff(row_ptr).max()) == entries == row_ptr[1]
        n_hubs = K._hubs_for(K.DeviceCSR(row_ptr, col), lanes)[1]
        assert n_hubs == (1 if entries > K.HUB_FACTOR * lanes else 0)       # a hub row exactly where one is meant
        _check(row_ptr, col, z, lanes=lanes, what=(lanes, entries, weights))


@pytest.mark.parametrize('weights', list(WEIGHTS))
def test_self_loops_and_isolated_rows(weights):
    G = nx.gnp_random_graph(60, 0.12, seed=11)
    pairs = _pairs_of(G) + [(v, v) for v in (0, 5, 17, 59)] + [(61, 61)]      # 60 and 62 isolated, 61 only its loop
    row_ptr, col, z = so.csr_from_pairs(63, pairs, WEIGHTS[weights])
    con, es, _ = _check(row_ptr, col, z, what=weights)
    assert np.isnan(con[60]) and np.isnan(es[62]) and not np.isnan(con[61])


@pytest.mark.parametrize('weight', [None, 'weight'])
def test_directed_graph_through_the_symmetrised_csr(weight):
    D = _digraph()
    row_ptr, col, z, out_row_ptr = so.mutual_csr(D, weight)
    con, es, _ = _check(row_ptr, col, z, out_row_ptr, what=weight)
    assert np.isnan(con[41]) and np.isnan(es[41]) and np.isnan(con[42]) and not np.isnan(con[40])
    nodes = sorted(D)
    want = nx.constraint(D, weight=weight)
    so.assert_close((con, None, None), (np.array([want[v] for v in nodes]), None, None), row_ptr, 'networkx')


def test_zero_weights_that_zero_a_row_sum():
    G = nx.gnp_random_graph(30, 0.25, seed=9)
    dead = {0, 4, 11}                                           # every edge at these nodes weighs 0: S = X = 0
    row_ptr, col, z = so.csr_from_pairs(30, _pairs_of(G), lambda a, b: 0.0 if (a in dead or b in dead) else 1.5 + a % 3)
    assert all(row_ptr[v + 1] > row_ptr[v] for v in dead)
    con, es, loc = _check(row_ptr, col, z)
    for v in dead:
        assert con[v] == 0.0 and es[v] == row_ptr[v + 1] - row_ptr[v]


def test_single_outputs_equal_the_joint_call_and_runs_are_bit_identical():
    n, pairs = _named_pairs('ba2000')
    row_ptr, col, z = so.csr_from_pairs(n, pairs, WEIGHTS['float'])
    both = _run(row_ptr, col, z)
    again = _run(row_ptr, col, z)
    for a, b in zip(both, again):
        assert np.array_equal(a, b, equal_nan=True)
    for k in range(3):
        want = tuple(j == k for j in range(3))
        alone = _run(row_ptr, col, z, want=want)
        assert [x is not None for x in alone] == list(want)
        assert np.array_equal(alone[k], both[k], equal_nan=True)
    n1, p1 = _named_pairs('wheel1500')
    r1, c1, z1 = so.csr_from_pairs(n1, p1, WEIGHTS['float'])    # with a hub row
    for a, b in zip(_run(r1, c1, z1), _run(r1, c1, z1)):
        assert np.array_equal(a, b, equal_nan=True)


def test_second_trip_of_the_grid_stride_loops():
    """BA 60 000 / m = 5 against the sparse oracle.  With 32 lanes a workgroup pass takes RJ_BLOCK / 32 = 8 rows or
    arcs, so the row kernels (cap RJ_ROW_MAX_WG) and the per-arc kernel (cap RJ_ARC_MAX_WG) both wrap; with the CSR's
    own 4 lanes the per-arc kernel wraps.  (Every other second-trip test of the suite is listed at the top of
    tests/test_gpu_second_trip.py.)"""
    from graphrole_amd import kernels as K
    n, row_ptr, col, z = _ba60000()
    nnz = len(col)
    assert int(np.diff(row_ptr).max()) <= so.MAX_ROW
    assert n > K.RJ_ROW_MAX_WG * (K.RJ_BLOCK // 32) and nnz > K.RJ_ARC_MAX_WG * (K.RJ_BLOCK // 32)
    csr = K.DeviceCSR(row_ptr, col)
    assert nnz > K.RJ_ARC_MAX_WG * (K.RJ_BLOCK // csr.lanes_per_row) and csr.n_hubs > 0
    want = so.sparse(row_ptr, col, z)
    so.assert_close(_run(row_ptr, col, z, lanes=32), want, row_ptr, 'lanes 32')
    so.assert_close(_run(row_ptr, col, z), want, row_ptr, 'own lanes')


# ------------------------------------------------------------------------------------------------------ API level
def _against_networkx(G, weight):
    from graphrole_amd import constraint, effective_size
    nodes = sorted(G)
    deg = np.array([max(len(set(nx.all_neighbors(G, v))), 1) for v in nodes])
    got, want = constraint(G, weight=weight), nx.constraint(G, weight=weight)
    assert list(got.index) == nodes and got.name == 'constraint' and got.dtype == np.float64
    g, w = got.to_numpy(), np.array([want[v] for v in nodes])
    assert np.array_equal(np.isnan(g), np.isnan(w))
    ok = ~np.isnan(w)
    assert np.all(np.abs(g[ok] - w[ok]) <= so.RTOL * np.abs(w[ok]))
    got, want = effective_size(G, weight=weight), nx.effective_size(G, weight=weight)
    assert list(got.index) == nodes and got.name == 'effective_size'
    g, w = got.to_numpy(), np.array([want[v] for v in nodes])
    assert np.array_equal(np.isnan(g), np.isnan(w))
    ok = ~np.isnan(w)
    assert np.all(np.abs(g[ok] - w[ok]) <= so.ES_ATOL * deg[ok])


@pytest.mark.parametrize('weight', [None, 'weight'])
def test_api_against_networkx(weight):
    _against_networkx(nx.karate_club_graph(), weight)
    D = nx.gnm_random_graph(25, 90, seed=3, directed=True)
    rng = random.Random(3)
    for u, v in D.edges:
        D[u][v]['weight'] = rng.choice([0.5, 1.0, 2.0, 7.25])
    D.add_edge(3, 3, weight=1.5)
    _against_networkx(D, weight)
    L = nx.gnp_random_graph(20, 0.3, seed=6)
    L.add_edges_from([(0, 0), (7, 7), (19, 19)])
    _against_networkx(L, weight)


def test_csr_graph_input_gives_the_same_bits():
    from graphrole_amd import constraint, effective_size
    from graphrole_amd.graph.csr import CSRGraph
    G = nx.karate_club_graph()
    src, dst, w = zip(*G.edges(data='weight'))
    C = CSRGraph(34, src, dst, weights=np.asarray(w, dtype=np.float64))
    for weight in (None, 'weight'):
        assert np.array_equal(constraint(C, weight=weight).to_numpy(), constraint(G, weight=weight).to_numpy())
    assert np.array_equal(effective_size(C, weight='weight').to_numpy(), effective_size(G, weight='weight').to_numpy())
    got = constraint(G, nodes=[33, 0, 5], weight='weight')
    assert list(got.index) == [0, 5, 33]
    assert np.array_equal(got.to_numpy(), constraint(G, weight='weight').to_numpy()[[0, 5, 33]])


def test_node_measures_columns_and_sense_making_on_karate():
    from graphrole_amd import RecursiveFeatureExtractor, RoleExtractor, constraint, node_measures
    G = nx.karate_club_graph()
    M = node_measures(G, ['effective_size', 'constraint'], weight='weight')
    assert list(M.columns) == ['effective_size', 'constraint'] and list(M.index) == sorted(G)
    assert np.array_equal(M['constraint'].to_numpy(), constraint(G, weight='weight').to_numpy())
    want = nx.effective_size(G)                                 # the existing column: networkx's n - 2t/n
    assert np.allclose(M['effective_size'].to_numpy(), [want[v] for v in sorted(G)], rtol=1e-12, atol=0)
    features = RecursiveFeatureExtractor(G).extract_features()
    np.random.seed(0)
    roles = RoleExtractor(n_roles=3)
    roles.extract_role_factors(features)
    E = roles.sense_making(M)
    assert list(E.columns) == ['effective_size', 'constraint'] and np.all(E.to_numpy() >= 0)
