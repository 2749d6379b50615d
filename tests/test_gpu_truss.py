"""
Truss numbers on the MI355X: graphrole_amd.truss_number, node_truss_number and k_truss equal to networkx's own k_truss
computed here (integers: compared with ==) on every graph kind -- hub rows, every graph on five nodes in one call (the
smallest graphs where two edges of a triangle leave in the same round), a clique behind a long tail (k jumps 2 -> 40:
both sweeps run), a triangulated cylinder that peels ring by ring over 150 rounds (several read-back batches), a wheel
whose hub row collapses in one round and a book whose spine takes 1 500 single decrements in one round while the id
rule fires 1 500 times; kernels.truss_numbers on the adapter's CSR against tests/truss_oracle.py on the same arrays,
for every lane width; the same bytes in a second run and for a relabelled copy; the refusals; and the karate
sense-making run with the node column.
"""
import functools
import itertools

import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import truss_oracle as to

pytestmark = pytest.mark.gpu


def _five_node_union():
    """The disjoint union of all 1 024 graphs on five labelled nodes: graph `mask` on the nodes 5 mask .. 5 mask + 4."""
    pairs = list(itertools.combinations(range(5), 2))
    G = nx.empty_graph(5 * 1024)
    G.add_edges_from((5 * mask + a, 5 * mask + b) for mask in range(1024)
                     for k, (a, b) in enumerate(pairs) if mask >> k & 1)
    return G


def _clique_with_tail():
    G = nx.complete_graph(40)
    nx.add_path(G, [0] + list(range(40, 240)))
    return G


def _cylinder(rings=150, width=5):
    """A triangulated cylinder: nodes (i, j), edges (i, j)-(i, j + 1 mod width), (i, j)-(i + 1, j) and
    (i, j)-(i + 1, j + 1 mod width).  Every edge has truss number 3, and the 4-truss peel eats it ring by ring."""
    G = nx.Graph()
    for i in range(rings):
        for j in range(width):
            G.add_edge((i, j), (i, (j + 1) % width))
            if i + 1 < rings:
                G.add_edge((i, j), (i + 1, j))
                G.add_edge((i, j), (i + 1, (j + 1) % width))
    return G


def _book(pages=1500):
    """Two nodes joined to each other and both to `pages` others: one hub-hub edge of support `pages`."""
    G = nx.Graph([(0, 1)])
    G.add_edges_from((s, p) for p in range(2, pages + 2) for s in (0, 1))
    return G


def _disconnected():
    G = nx.disjoint_union(nx.barabasi_albert_graph(200, 3, seed=1), nx.cycle_graph(9))
    G.add_nodes_from([1000, 1001])
    return G


GRAPHS = {
    'karate': nx.karate_club_graph,
    'ba2000': lambda: nx.barabasi_albert_graph(2000, 5, seed=3),
    'five_nodes': _five_node_union,
    'clique_tail': _clique_with_tail,
    'cylinder': _cylinder,
    'wheel': lambda: nx.wheel_graph(1501),
    'book': _book,
    'grid40': lambda: nx.grid_2d_graph(40, 40),
    'tree': lambda: nx.random_labeled_tree(500, seed=11),
    'disconnected': _disconnected,
    'strings': lambda: nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
    'empty5': lambda: nx.empty_graph(5),
    'n2': lambda: nx.path_graph(2),
    'k3': lambda: nx.complete_graph(3),
}


@functools.lru_cache(maxsize=None)
def _graph(key):
    return GRAPHS[key]()


@functools.lru_cache(maxsize=None)
def _networkx(key):
    """({frozenset edge: t}, {node: t}) from nx.k_truss alone; computed once per graph and never changed."""
    return to.networkx_truss_numbers(_graph(key))


@functools.lru_cache(maxsize=None)
def _oracle(key):
    _, row_ptr, col = to.graph_csr(_graph(key))
    return to.truss_numbers(row_ptr, col)


@pytest.mark.parametrize('key', list(GRAPHS))
def test_matches_networkx(key):
    from graphrole_amd import truss_number
    G = _graph(key)
    want, _ = _networkx(key)
    t = truss_number(G)
    assert t.name == 'truss_number' and t.dtype == np.int64
    assert isinstance(t.index, pd.MultiIndex) and t.index.nlevels == 2 and len(t) == G.number_of_edges()
    rank = {v: i for i, v in enumerate(sorted(G))}
    order = [(rank[u], rank[v]) for u, v in t.index]
    assert all(a < b for a, b in order) and order == sorted(order)
    assert {frozenset(e): int(x) for e, x in zip(t.index, t.to_numpy())} == want
    assert t.attrs['rounds'] == _oracle(key).n_rounds and t.attrs['levels'] == len(set(want.values()))


@pytest.mark.parametrize('key', list(GRAPHS))
def test_node_truss_number_matches_networkx(key):
    from graphrole_amd import node_truss_number
    G = _graph(key)
    nt = node_truss_number(G)
    assert nt.name == 'node_truss_number' and nt.dtype == np.int64 and list(nt.index) == sorted(G)
    assert nt.to_dict() == _networkx(key)[1]


def test_the_graph_kinds_are_what_they_are_here_for():
    from graphrole_amd.graph.interface.networkx import NetworkxInterface

    def values(key):
        return sorted(set(_networkx(key)[0].values()))

    assert values('karate') == [2, 3, 4, 5]
    assert values('ba2000') == [2, 3, 4, 5, 6]
    assert _oracle('ba2000').n_rounds == 15 and _oracle('ba2000').n_levels == 5        # k jumps 4 times
    for key in ('ba2000', 'wheel', 'book'):
        assert NetworkxInterface(_graph(key))._structure_csrs()[0].n_hubs > 0, key
    G = _graph('five_nodes')
    assert G.number_of_nodes() == 5120 and G.number_of_edges() == 5120
    assert max(values('five_nodes')) == 5 and _oracle('five_nodes').n_rounds == 6
    _, row_ptr, col = to.graph_csr(G)                           # the id rule matters in this very graph
    assert not np.array_equal(to.truss_numbers(row_ptr, col, dedupe=False).arc_truss, _oracle('five_nodes').arc_truss)
    assert values('clique_tail') == [2, 40] and _oracle('clique_tail').n_levels == 2   # 2 -> 40: both sweeps again
    G = _graph('cylinder')
    assert G.number_of_nodes() == 750 and G.number_of_edges() == 2240
    assert values('cylinder') == [3] and _oracle('cylinder').n_rounds == 150
    assert max(d for _, d in _graph('wheel').degree()) == 1500 and values('wheel') == [3]
    assert _oracle('wheel').n_rounds == 2                       # the rim leaves, then every spoke at once
    G = _graph('book')
    assert len(set(G[0]) & set(G[1])) == 1500 and values('book') == [3]
    assert _oracle('book').n_rounds == 2 and _oracle('book').decrements == 1500        # one per page, not two
    assert values('grid40') == [2] and values('tree') == [2]
    assert set(_networkx('grid40')[1].values()) == {2} and set(_networkx('tree')[1].values()) == {2}
    node_t = _networkx('disconnected')[1]
    assert node_t[1000] == 0 and node_t[1001] == 0 and min(v for k, v in node_t.items() if k < 1000) == 2
    assert _networkx('empty5') == ({}, {v: 0 for v in range(5)})
    assert _networkx('n2')[0] == {frozenset((0, 1)): 2} and set(_networkx('k3')[0].values()) == {3}


@pytest.mark.parametrize('key', ['karate', 'ba2000'])
def test_k_truss_equals_networkx(key):
    from graphrole_amd import k_truss
    G = _graph(key).copy()
    G.graph['name'] = key
    nx.set_node_attributes(G, {v: v % 7 for v in G}, 'mod')
    nx.set_edge_attributes(G, {e: e[0] + e[1] for e in G.edges()}, 'sum')
    top = max(_networkx(key)[0].values())
    for k in range(2, top + 2):
        H = k_truss(G, k)
        assert nx.utils.graphs_equal(H, nx.k_truss(G, k)), k
    assert H.number_of_nodes() == 0


def _kernel_run(csr, **kwargs):
    from graphrole_amd import kernels as K
    arc, node, n_rounds, n_levels = K.truss_numbers(csr, **kwargs)
    return (K.to_host(arc)[:csr.nnz].copy(), None if node is None else K.to_host(node)[:csr.n].copy(), n_rounds,
            n_levels)


@pytest.mark.parametrize('key', ['ba2000', 'book', 'cylinder', 'clique_tail', 'five_nodes'])
def test_kernel_equals_oracle_on_the_same_csr(key):
    from graphrole_amd import kernels as K
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    csr = NetworkxInterface(_graph(key))._structure_csrs()[0]
    row_ptr = K.to_host(csr.row_ptr).astype(np.int64)
    col = K.to_host(csr.col)[:csr.nnz].astype(np.int64)
    want = to.truss_numbers(row_ptr, col)
    arc, node, n_rounds, n_levels = _kernel_run(csr)
    assert arc.dtype == np.int32 and node.dtype == np.int64
    assert np.array_equal(arc, want.arc_truss) and np.array_equal(node, want.node_truss)
    assert n_rounds == want.n_rounds == _oracle(key).n_rounds and n_levels == want.n_levels
    # both arcs of every edge hold the same value
    rows = np.repeat(np.arange(csr.n, dtype=np.int64), np.diff(row_ptr))
    reverse = np.searchsorted(rows * csr.n + col, col * csr.n + rows)
    assert np.array_equal(arc[reverse], arc)
    arc2, node2, rounds2, levels2 = _kernel_run(csr, want_node=False)
    assert node2 is None and arc2.tobytes() == arc.tobytes() and (rounds2, levels2) == (n_rounds, n_levels)
    for lanes in (4, 8, 16, 32):
        arc3, node3, rounds3, levels3 = _kernel_run(csr, lanes=lanes)
        assert arc3.tobytes() == arc.tobytes() and node3.tobytes() == node.tobytes(), lanes
        assert (rounds3, levels3) == (n_rounds, n_levels), lanes


def test_relabelled_copy_and_second_run_give_the_same_bytes():
    from graphrole_amd import node_truss_number, truss_number
    G = _graph('ba2000')
    a, b = truss_number(G), truss_number(G)
    assert list(a.index) == list(b.index) and a.to_numpy().tobytes() == b.to_numpy().tobytes()
    na, nb = node_truss_number(G), node_truss_number(G)
    assert na.to_numpy().tobytes() == nb.to_numpy().tobytes()
    shuffled = np.random.default_rng(5).permutation(2000)
    H = nx.relabel_nodes(G, {v: int(shuffled[v]) for v in G})   # other ids: other rows, edge ids, lists, hub blocks
    c, nc = truss_number(H), node_truss_number(H)
    back = c.loc[[tuple(sorted((int(shuffled[u]), int(shuffled[v])))) for u, v in a.index]]
    assert back.to_numpy().tobytes() == a.to_numpy().tobytes()
    assert nc.loc[[int(shuffled[v]) for v in na.index]].to_numpy().tobytes() == na.to_numpy().tobytes()
    assert c.attrs == a.attrs


def test_refusals_reach_no_device_entry_point(monkeypatch):
    from graphrole_amd import k_truss, kernels as K, node_truss_number, truss_number
    from graphrole_amd.graph.interface.networkx import NetworkxInterface

    def no_device(*args, **kwargs):
        raise AssertionError('device work for a refused graph')

    monkeypatch.setattr(K, 'truss_numbers', no_device)
    monkeypatch.setattr(NetworkxInterface, '_device_graph', no_device)
    D = nx.gnm_random_graph(30, 90, seed=2, directed=True)
    L = nx.karate_club_graph()
    L.add_edge(3, 3)
    M = nx.MultiGraph([(0, 1), (0, 1), (1, 2)])
    for fn in (truss_number, node_truss_number, lambda G: k_truss(G, 3)):
        for G, word in ((D, 'directed'), (L, 'selfloop_edges'), (M, 'multigraph')):
            with pytest.raises(NotImplementedError, match=word):
                fn(G)
    with pytest.raises(TypeError, match='truss_number'):
        k_truss({'not': 'a graph'}, 3)


def test_karate_end_to_end_sense_making():
    from graphrole_amd import RecursiveFeatureExtractor, RoleExtractor, node_measures, node_truss_number
    G = nx.karate_club_graph()
    features = RecursiveFeatureExtractor(G).extract_features()
    np.random.seed(0)
    role_extractor = RoleExtractor(n_roles=3)
    role_extractor.extract_role_factors(features)
    M = node_measures(G, ['degree', 'core_number'])
    M['truss_number'] = node_truss_number(G)
    assert list(M.columns) == ['degree', 'core_number', 'truss_number']
    assert M['truss_number'].to_dict() == _networkx('karate')[1]
    E = role_extractor.sense_making(M)
    assert E.shape == (3, 3) and list(E.columns) == list(M.columns)
    assert np.all(E.to_numpy() >= 0)
