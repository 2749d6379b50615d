"""
The square clustering coefficient on the MI355X.  API parity: graphrole_amd.square_clustering against
nx.square_clustering, equal as floats (every quantity is an integer until the one division).  Kernel parity:
kernels.square_clustering (grx_square_clustering) against tests/square_clustering_oracle.py -- the coefficient bitwise,
squares and potential as integers -- on hub rows and rows of the dense-counter tier, where networkx would take half a
minute, on hand-built rows at the two tier thresholds, with ids that collide under every power-of-two modulus, and with
a two-hop set that holds the row's own neighbours and the row itself; the bits that must not move; BA 1 M / m = 10 on
sampled rows.
"""
import functools

import networkx as nx
import numpy as np
import pytest

from tests import square_clustering_oracle as so

pytestmark = pytest.mark.gpu


def _run(row_ptr, col, lanes=None, want_counts=True):
    """One kernel call on the CSR arrays: host (C4, squares, potential)."""
    from graphrole_amd import kernels as K
    n = len(row_ptr) - 1
    c, q, p = K.square_clustering(K.DeviceCSR(row_ptr, col), want_counts=want_counts, lanes=lanes)
    return tuple(None if x is None else K.to_host(x)[:n].copy() for x in (c, q, p))


def _check(row_ptr, col, lanes=None, what=''):
    """The kernel against the oracle on every row that has an entry; an empty row gives three zeros."""
    got = _run(row_ptr, col, lanes)
    rows = np.nonzero(np.diff(row_ptr))[0]
    Q, P, C = so.square_clustering(row_ptr, col, rows)
    assert np.array_equal(got[1][rows], Q), (what, 'squares')
    assert np.array_equal(got[2][rows], P), (what, 'potential')
    assert got[0][rows].tobytes() == C.tobytes(), (what, 'square clustering')
    empty = np.diff(row_ptr) == 0
    assert not got[0][empty].any() and not got[1][empty].any() and not got[2][empty].any()
    return got


# ------------------------------------------------------------------------------------------------------ API level
def _disconnected():
    G = nx.disjoint_union(nx.complete_bipartite_graph(5, 7), nx.cycle_graph(9))
    G = nx.disjoint_union(G, nx.gnm_random_graph(40, 120, seed=2))
    G.add_nodes_from([1000, 1001, 1002])                        # isolated
    return G


def _karate_with_loops():
    G = nx.karate_club_graph()
    G.add_edges_from([(0, 0), (1, 1), (11, 11)])                # a hub, a neighbour of that hub, a leaf of it
    return G


def _multigraph():
    G = nx.gnm_random_graph(60, 240, seed=8)
    M = nx.MultiGraph(G)
    M.add_edges_from(list(G.edges)[:50])
    M.add_edges_from([(4, 4), (4, 4)])
    return M


GRAPHS = {
    'karate': nx.karate_club_graph,
    'gnm300': lambda: nx.gnm_random_graph(300, 1200, seed=1),
    'ba2000': lambda: nx.barabasi_albert_graph(2000, 5, seed=3),
    'grid30': lambda: nx.grid_2d_graph(30, 30),
    'K20_40': lambda: nx.complete_bipartite_graph(20, 40),
    'K40': lambda: nx.complete_graph(40),
    'star300': lambda: nx.star_graph(300),
    'P2': lambda: nx.path_graph(2),
    'P3': lambda: nx.path_graph(3),
    'empty5': lambda: nx.empty_graph(5),
    'n1': lambda: nx.empty_graph(1),
    'disconnected': _disconnected,
    'karate_loops': _karate_with_loops,
    'strings': lambda: nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
    'multigraph': _multigraph,
}


@pytest.mark.parametrize('key', list(GRAPHS))
def test_equals_networkx_bit_for_bit(key):
    from graphrole_amd import square_clustering
    G = GRAPHS[key]()
    got = square_clustering(G)
    assert got.name == 'square_clustering' and got.dtype == np.float64 and list(got.index) == sorted(G)
    want = nx.square_clustering(G)
    assert {v: float(x) for v, x in got.to_dict().items()} == {v: float(x) for v, x in want.items()}
    values = got.to_numpy()
    if key in ('K20_40', 'K40'):
        assert np.all(values == 1.0)
    if key in ('star300', 'P2', 'P3', 'empty5', 'n1'):
        assert np.all(values == 0.0)
    if key == 'ba2000':
        assert len(np.unique(values)) > 1000
    if key == 'karate_loops':
        assert square_clustering(G, 11) == float(want[11])


def test_nodes_argument_on_the_device():
    from graphrole_amd import square_clustering
    G = nx.karate_club_graph()
    want = nx.square_clustering(G)
    one = square_clustering(G, 5)
    assert isinstance(one, float) and one == want[5]
    some = square_clustering(G, [33, 'nobody', 0])
    assert some.to_dict() == {0: want[0], 33: want[33]}
    assert len(square_clustering(nx.Graph())) == 0
    with pytest.raises(NotImplementedError, match='insertion order'):
        square_clustering(nx.DiGraph(G))


# --------------------------------------------------------------------------- hub rows and the dense-counter tier
@functools.lru_cache(maxsize=None)
def _hub_case(key):
    """(row_ptr, col of the adapter's structure CSR, the oracle's (Q, potential, C4)), computed once."""
    from graphrole_amd import kernels as K
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    if key == 'two_hubs':
        G = nx.barabasi_albert_graph(3000, 3, seed=5)
        G.add_edges_from((0, v) for v in range(1, 2501))
        G.add_edges_from((1, v) for v in range(2, 2001))
    else:
        G = nx.star_graph(1500)
    csr = NetworkxInterface(G)._structure_csrs()[0]
    row_ptr, col = K.to_host(csr.row_ptr).copy(), K.to_host(csr.col)[:csr.nnz].copy()
    return csr, row_ptr, col, so.square_clustering(row_ptr, col)


@pytest.mark.parametrize('key', ['two_hubs', 'star1500'])
def test_hub_rows_and_both_tiers_against_the_oracle(key):
    from graphrole_amd import kernels as K
    csr, row_ptr, col, (Q, P, C) = _hub_case(key)
    assert csr.n_hubs > 0
    wedges = so.wedge_counts(row_ptr, col)
    if key == 'two_hubs':
        assert np.diff(row_ptr).max() > 2400 and wedges.max() > 20000
        assert np.any(wedges > K.SQ_LDS_MAX_WEDGES) and np.any(wedges <= K.SQ_LDS_MAX_WEDGES)
        assert np.any(wedges <= K.SQ_WAVE_MAX_WEDGES)
        assert np.count_nonzero(Q) > 2900
    else:
        assert np.all(wedges == 1500) and np.all(C == 0.0) and np.all(P[np.diff(row_ptr) == 1] == 0)
    first = None
    for lanes in (None, 4, 8, 16, 32):
        assert K._hubs_for(csr, lanes)[1] > 0
        c, q, p = K.square_clustering(csr, want_counts=True, lanes=lanes)
        c, q, p = (K.to_host(x)[:csr.n].copy() for x in (c, q, p))
        assert np.array_equal(q, Q) and np.array_equal(p, P), lanes
        assert c.tobytes() == C.tobytes(), lanes
        first = c if first is None else first
        assert c.tobytes() == first.tobytes()
    alone = K.square_clustering(csr)
    assert alone[1] is None and alone[2] is None and K.to_host(alone[0])[:csr.n].tobytes() == C.tobytes()


# -------------------------------------------------------------------------------------------- hand-built rows
def _two_level(n_neighbours, row_length, pool, extra=0, stride=1):
    """Row 0 with `n_neighbours` neighbours 1 .. a, each adjacent to 0 and to `row_length - 1` of the `pool` two-hop
    nodes stride * (a + 1 + t) (the first neighbour to `extra` more): row 0 has n_neighbours * row_length + extra
    wedges, and the shared two-hop nodes close squares."""
    a = n_neighbours
    ids = [stride * (a + 1 + t) for t in range(pool)]
    pairs = []
    for i in range(1, a + 1):
        pairs.append((0, i))
        length = row_length - 1 + (extra if i == 1 else 0)
        assert length <= pool
        pairs += [(i, ids[(7 * i + t) % pool]) for t in range(length)]
    return so.csr_from_pairs(ids[-1] + 1, pairs)


@pytest.mark.parametrize('tier', ['wave', 'lds'])
def test_rows_at_the_tier_thresholds(tier):
    from graphrole_amd import kernels as K
    threshold = {'wave': K.SQ_WAVE_MAX_WEDGES, 'lds': K.SQ_LDS_MAX_WEDGES}[tier]
    length = {'wave': 32, 'lds': 64}[tier]
    assert threshold % length == 0
    for extra in (0, 1):
        row_ptr, col = _two_level(threshold // length, length, 2 * length, extra)
        assert so.wedge_counts(row_ptr, col)[0] == threshold + extra
        c, q, p = _check(row_ptr, col, what=(tier, extra))
        assert q[0] > 0 and 0.0 < c[0] < 1.0


@pytest.mark.parametrize('slots', [1024, 4096])
def test_ids_that_collide_under_every_power_of_two_modulus(slots):
    """The two-hop ids of row 0 are multiples of 4 096, the largest table: congruent modulo every power of two up to
    the size of either table."""
    from graphrole_amd import kernels as K
    a, length, pool = (20, 31, 40) if slots == 1024 else (40, 51, 60)
    row_ptr, col = _two_level(a, length, pool, stride=4096)
    wedges = so.wedge_counts(row_ptr, col)[0]
    assert wedges == a * length
    assert (wedges <= K.SQ_WAVE_MAX_WEDGES) == (slots == 1024) and wedges <= K.SQ_LDS_MAX_WEDGES
    two_hop = np.unique(col[row_ptr[1]:row_ptr[a + 1]])
    assert np.all(two_hop % 4096 == 0) and len(two_hop) == pool + 1
    c, q, p = _check(row_ptr, col, what=slots)
    assert q[0] > 0


def test_two_hop_set_with_the_own_neighbours_and_the_row_itself():
    """A clique with loops and pendant paths: every neighbour of a clique node is also two hops away, and so is the
    node itself -- what the x != v exclusion and the look-up of the row's own entries are for."""
    G = nx.complete_graph(14)
    G.add_edges_from([(0, 0), (1, 1), (5, 5), (13, 13)])
    nx.add_path(G, [0, 14, 15, 16])
    nx.add_path(G, [3, 17, 18])
    G.add_edges_from([(15, 15), (18, 18), (19, 19)])            # 19: a loop and nothing else
    G.add_edge(20, 20)
    G.add_edge(20, 21)                                          # potential <= 0 beside squares > 0
    G.add_edge(21, 21)
    row_ptr, col = so.csr_from_pairs(22, list(G.edges))
    c, q, p = _check(row_ptr, col)
    want = nx.square_clustering(G)
    assert [float(want[v]) for v in range(22)] == c.tolist()
    assert q[20] == 1 and p[20] <= 0 and c[20] == 1.0           # networkx leaves its numerator there


# ------------------------------------------------------------------------------------- determinism, end to end
def test_relabelled_copy_and_second_run_give_the_same_bytes():
    from graphrole_amd import square_clustering
    G = nx.barabasi_albert_graph(1500, 4, seed=9)
    G.add_edges_from([(3, 3), (700, 700)])
    perm = np.random.RandomState(4).permutation(1500)
    H = nx.relabel_nodes(G, {v: int(perm[v]) for v in G})
    a, b = square_clustering(G), square_clustering(H)
    assert a.to_numpy().tobytes() == b.to_numpy()[perm].tobytes()
    assert square_clustering(G).to_numpy().tobytes() == a.to_numpy().tobytes()


def test_karate_end_to_end_sense_making():
    from graphrole_amd import RecursiveFeatureExtractor, RoleExtractor, node_measures, square_clustering
    G = nx.karate_club_graph()
    features = RecursiveFeatureExtractor(G).extract_features()
    np.random.seed(0)
    roles = RoleExtractor(n_roles=3)
    roles.extract_role_factors(features)
    M = node_measures(G, ['degree', 'clustering'])
    M['square_clustering'] = square_clustering(G)
    assert list(M.columns) == ['degree', 'clustering', 'square_clustering'] and not M.isna().any().any()
    want = nx.square_clustering(G)
    assert M['square_clustering'].to_dict() == {v: float(want[v]) for v in G}
    E = roles.sense_making(M)
    assert E.shape == (3, 3) and list(E.columns) == list(M.columns) and np.all(E.to_numpy() >= 0)


# ------------------------------------------------------------------------------------------------------ full size
def test_full_size_ba_1m_on_sampled_rows():
    """BA 1 M / m = 10 (the BASELINE graph): 512 seeded random rows and the 8 rows of largest degree against the row
    oracle; the whole A^2 would not fit on the host."""
    from graphrole_amd import kernels as K, synth
    from graphrole_amd.measures import _adapter
    csr = _adapter(synth.ba_graph(1_000_000, 10, seed=0))._structure_csrs()[0]
    c, q, p = K.square_clustering(csr, want_counts=True)
    row_ptr, col = K.to_host(csr.row_ptr), K.to_host(csr.col)[:csr.nnz]
    hubs = np.argsort(np.diff(row_ptr))[-8:]
    rows = np.unique(np.concatenate([np.random.RandomState(0).choice(csr.n, 512, replace=False), hubs]))
    Q, P, C = so.square_clustering(row_ptr, col, rows)
    assert np.array_equal(K.to_host(q)[rows], Q) and np.array_equal(K.to_host(p)[rows], P)
    assert K.to_host(c)[rows].tobytes() == C.tobytes()
    assert np.all(K.to_host(q)[hubs] > 0) and np.count_nonzero(Q) > 8 and P.max() < 2 ** 53
