"""
-m "not gpu": truss numbers without a device.  tests/truss_oracle.py (the numpy restatement of the level-synchronous
edge peeling of csrc/grx_truss.hip) against networkx's own k_truss, exactly, on the seeded families of
tests/test_kcore_cpu.py (the undirected ones) with a denser G(n, m) added and on every graph on five labelled nodes --
among them the graphs where two edges of a triangle leave in the same round, which an oracle without the id rule gets
wrong; then the Python layer of graphrole_amd.truss_number / node_truss_number / k_truss over a CPU double of
kernels.truss_numbers (the oracle on the double's CSR arrays); the argument checks of grx_truss_numbers, the ctypes
signatures, the header's version and the unchanged catalogue.  The device numbers are pinned in tests/test_gpu_truss.py.
"""
import itertools
import os
import random
import re
import types

import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import fake_kernels
from tests import truss_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_as_dicts(G, **kwargs):
    nodes, row_ptr, col = to.graph_csr(G)
    r = to.truss_numbers(row_ptr, col, **kwargs)
    rows = np.repeat(np.arange(len(nodes)), np.diff(row_ptr))
    edge_t = {}
    for a, b, t in zip(rows.tolist(), col.tolist(), r.arc_truss.tolist()):
        assert edge_t.setdefault(frozenset((nodes[a], nodes[b])), t) == t      # both arcs of an edge hold one value
    return r, edge_t, {v: int(r.node_truss[i]) for i, v in enumerate(nodes)}


def _check_against_networkx(G):
    r, edge_t, node_t = _oracle_as_dicts(G)
    want_edges, want_nodes = to.networkx_truss_numbers(G)
    assert r.arc_truss.dtype == np.int32 and r.node_truss.dtype == np.int64
    assert edge_t == want_edges
    assert node_t == want_nodes
    assert all(t >= 2 for t in edge_t.values())
    assert r.n_levels == len(set(edge_t.values()))
    assert (r.n_rounds == 0) == (G.number_of_edges() == 0) and r.n_rounds >= r.n_levels
    return r


def _clique_with_tail(k, tail):
    G = nx.complete_graph(k)
    nx.add_path(G, [0] + list(range(k, k + tail)))
    return G


def _families(seed):
    """The undirected families of tests/test_kcore_cpu.py, plus a G(n, m) with up to 4 n edges: truss numbers above
    3."""
    rng = random.Random(seed)
    n = rng.randint(4, 28)
    yield nx.gnm_random_graph(n, rng.randint(0, 2 * n), seed=seed)
    yield nx.gnm_random_graph(n, rng.randint(n // 2, n + 2), seed=seed + 1)
    yield nx.barabasi_albert_graph(n, 1, seed=seed)
    yield nx.barabasi_albert_graph(n, 2, seed=seed)
    yield nx.random_labeled_tree(n, seed=seed)
    yield nx.barbell_graph(rng.randint(3, 6), rng.randint(0, 4))
    yield nx.grid_2d_graph(rng.randint(1, 5), rng.randint(2, 5))
    yield nx.star_graph(rng.randint(1, 12))
    yield nx.windmill_graph(rng.randint(2, 5), rng.randint(2, 5))
    yield nx.disjoint_union(nx.gnm_random_graph(n, n + rng.randint(0, n), seed=seed + 2),
                            nx.disjoint_union(nx.cycle_graph(rng.randint(3, 9)), nx.empty_graph(2)))
    H = nx.gnm_random_graph(n, rng.randint(n // 2, 2 * n), seed=seed + 4)
    yield nx.relabel_nodes(H, dict(zip(H, rng.sample(list(H), len(H)))))
    yield _clique_with_tail(rng.randint(3, 7), rng.randint(1, 9))
    yield nx.gnm_random_graph(n, rng.randint(2 * n, 4 * n), seed=seed + 6)     # capped at the complete graph


@pytest.mark.parametrize('block', range(10))
def test_oracle_equals_networkx_on_seeded_graphs(block):
    checked, largest = 0, 0
    for seed in range(block * 10, block * 10 + 10):
        for G in _families(7919 * seed):
            r = _check_against_networkx(G)
            checked += 1
            largest = max(largest, int(r.arc_truss.max()) if len(r.arc_truss) else 0)
    assert checked == 10 * 13
    assert largest >= 5                                         # the dense family does reach beyond triangles


def test_oracle_every_graph_on_five_nodes():
    pairs = list(itertools.combinations(range(5), 2))
    differ = []
    for mask in range(1 << len(pairs)):
        G = nx.empty_graph(5)
        G.add_edges_from(p for k, p in enumerate(pairs) if mask >> k & 1)
        r = _check_against_networkx(G)
        _, row_ptr, col = to.graph_csr(G)
        if not np.array_equal(to.truss_numbers(row_ptr, col, dedupe=False).arc_truss, r.arc_truss):
            differ.append(G)
    # the case the id rule exists for is in the set: two edges of a triangle leave in one round, and without the rule
    # the third edge loses the triangle twice
    assert differ
    assert min(G.number_of_edges() for G in differ) == 8        # K4 and a fifth node adjacent to two of its nodes
    smallest = [G for G in differ if G.number_of_edges() == 8]
    assert all(sorted(d for _, d in G.degree()) == [2, 3, 3, 4, 4] for G in smallest)


def test_oracle_named_graphs():
    r = _check_against_networkx(nx.karate_club_graph())
    assert sorted(set(r.arc_truss.tolist())) == [2, 3, 4, 5]
    r = _check_against_networkx(nx.barabasi_albert_graph(2000, 5, seed=3))
    assert sorted(set(r.arc_truss.tolist())) == [2, 3, 4, 5, 6] and r.n_rounds == 15 and r.n_levels == 5
    r = _check_against_networkx(_clique_with_tail(8, 30))
    assert sorted(set(r.arc_truss.tolist())) == [2, 8] and r.n_levels == 2 and r.n_rounds == 2
    for G in (nx.empty_graph(0), nx.empty_graph(1), nx.empty_graph(5), nx.path_graph(2), nx.complete_graph(3),
              nx.complete_graph(7), nx.grid_2d_graph(4, 4), nx.complete_bipartite_graph(5, 5)):
        _check_against_networkx(G)
    r = _check_against_networkx(nx.empty_graph(5))
    assert r.node_truss.tolist() == [0] * 5 and r.n_rounds == 0 and r.n_levels == 0 and len(r.arc_truss) == 0
    # the README's example: the same core number, another truss number
    assert set(nx.core_number(nx.complete_graph(6)).values()) == {5}
    assert set(nx.core_number(nx.complete_bipartite_graph(5, 5)).values()) == {5}
    assert set(_oracle_as_dicts(nx.complete_graph(6))[2].values()) == {6}
    assert set(_oracle_as_dicts(nx.complete_bipartite_graph(5, 5))[2].values()) == {2}


# ------------------------------------------------------------------------------------------ Python layer, CPU double
@pytest.fixture
def cpu_backend():
    import torch
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.calls = []

    def truss_numbers(csr, want_node=True, lanes=None):
        double.calls.append((csr, want_node, lanes))
        r = to.truss_numbers(csr.row_ptr, csr.col)
        return (torch.from_numpy(r.arc_truss), torch.from_numpy(r.node_truss) if want_node else None, r.n_rounds,
                r.n_levels)

    double.truss_numbers = truss_numbers
    backend.use(double)
    yield double
    backend.use(None)


def _disconnected():
    G = nx.disjoint_union(nx.barabasi_albert_graph(60, 3, seed=1), nx.cycle_graph(9))
    G.add_nodes_from([1000, 1001])
    return G


GRAPHS = {
    'karate': nx.karate_club_graph,
    'er': lambda: nx.gnm_random_graph(120, 900, seed=3),
    'disconnected': _disconnected,
    'strings': lambda: nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
    'grid': lambda: nx.grid_2d_graph(4, 5),
    'k2': lambda: nx.path_graph(2),
}


def _expected_series(G):
    """truss_number(G) as the issue defines it, from networkx and the sorted labels alone."""
    edge_t, node_t = to.networkx_truss_numbers(G)
    rank = {v: i for i, v in enumerate(sorted(G))}
    keys = sorted((tuple(sorted(e, key=rank.get)) for e in edge_t), key=lambda e: (rank[e[0]], rank[e[1]]))
    return keys, [edge_t[frozenset(e)] for e in keys], node_t


@pytest.mark.parametrize('key', list(GRAPHS))
def test_public_functions(cpu_backend, key):
    from graphrole_amd import node_truss_number, truss_number
    G = GRAPHS[key]()
    keys, values, node_t = _expected_series(G)
    t = truss_number(G)
    assert isinstance(t, pd.Series) and t.name == 'truss_number' and t.dtype == np.int64
    assert isinstance(t.index, pd.MultiIndex) and t.index.nlevels == 2
    assert list(t.index) == keys and t.tolist() == values
    assert len(t) == G.number_of_edges()
    assert len(cpu_backend.calls) == 1 and cpu_backend.calls[0][1] is False
    nt = node_truss_number(G)
    assert isinstance(nt, pd.Series) and nt.name == 'node_truss_number' and nt.dtype == np.int64
    assert list(nt.index) == sorted(G) and nt.to_dict() == node_t
    assert len(cpu_backend.calls) == 2 and cpu_backend.calls[1][1] is True
    nodes, row_ptr, col = to.graph_csr(G)
    want = to.truss_numbers(row_ptr, col)
    for s in (t, nt):
        assert s.attrs['rounds'] == want.n_rounds and s.attrs['levels'] == want.n_levels
    # the kernel got the structure CSR of the adapter
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    ref = NetworkxInterface(G)._structure_csrs()[0]
    for csr, _, _ in cpu_backend.calls:
        assert np.array_equal(csr.row_ptr, ref.row_ptr) and np.array_equal(csr.col, ref.col)


def test_multiindex_order_on_string_labels(cpu_backend):
    from graphrole_amd import node_measures, truss_number
    G = nx.Graph([('pear', 'apple'), ('fig', 'pear'), ('apple', 'fig'), ('kiwi', 'apple'), ('zucchini', 'banana')])
    t = truss_number(G)
    assert list(t.index) == [('apple', 'fig'), ('apple', 'kiwi'), ('apple', 'pear'), ('banana', 'zucchini'),
                             ('fig', 'pear')]
    assert t.tolist() == [3, 2, 3, 2, 3]
    assert t.loc[('apple', 'kiwi')] == 2
    assert list(t.index.get_level_values(0).unique()) == [v for v in node_measures(G, ['weighted_degree']).index
                                                          if v in ('apple', 'banana', 'fig')]


def test_node_column_joins_the_measure_table(cpu_backend):
    from graphrole_amd import node_measures, node_truss_number
    G = _disconnected()
    M = node_measures(G, ['weighted_degree'])
    M['truss_number'] = node_truss_number(G)
    assert M['truss_number'].dtype == np.int64 and not M['truss_number'].isna().any()
    assert M.loc[1000, 'truss_number'] == 0 and M.loc[1001, 'truss_number'] == 0
    assert (M['truss_number'][M['weighted_degree'] > 0] >= 2).all()


def test_k_truss_equals_networkx_on_karate_with_attributes(cpu_backend):
    from graphrole_amd import k_truss
    G = nx.karate_club_graph()                                  # node attribute 'club', edge attribute 'weight'
    G.graph['name'] = 'karate'
    nx.set_node_attributes(G, {v: v * v for v in G}, 'square')
    nx.set_edge_attributes(G, {e: f'{e[0]}-{e[1]}' for e in G.edges()}, 'tag')
    sizes = []
    for k in range(2, 7):
        H = k_truss(G, k)
        assert type(H) is nx.Graph
        assert nx.utils.graphs_equal(H, nx.k_truss(G, k))
        sizes.append(H.number_of_edges())
    assert sizes[0] == G.number_of_edges() and sizes[-1] == 0 and sorted(sizes, reverse=True) == sizes
    assert len(set(sizes)) == 5
    H = k_truss(G, 4)
    H.nodes[0]['club'] = 'changed'                              # a copy: G is not touched
    H.remove_edge(*next(iter(H.edges())))
    assert G.nodes[0]['club'] != 'changed' and G.number_of_edges() == 78


def test_empty_and_edgeless_graphs_make_no_kernel_call(cpu_backend):
    from graphrole_amd import k_truss, node_truss_number, truss_number
    for G in (nx.empty_graph(0), nx.empty_graph(5)):
        t = truss_number(G)
        assert t.name == 'truss_number' and t.dtype == np.int64 and len(t) == 0
        assert isinstance(t.index, pd.MultiIndex) and t.index.nlevels == 2
        nt = node_truss_number(G)
        assert nt.name == 'node_truss_number' and nt.dtype == np.int64
        assert list(nt.index) == list(G) and nt.tolist() == [0] * len(G)
        assert t.attrs == dict(rounds=0, levels=0) and nt.attrs == dict(rounds=0, levels=0)
        assert nx.utils.graphs_equal(k_truss(G, 2), nx.k_truss(G, 2))
    assert cpu_backend.calls == []


def test_every_refusal_makes_no_device_call(cpu_backend, monkeypatch):
    from graphrole_amd import k_truss, node_truss_number, truss_number
    from graphrole_amd.graph.csr import CSRGraph
    from graphrole_amd.graph.interface.networkx import NetworkxInterface

    def no_device(*args, **kwargs):
        raise AssertionError('device work for a refused graph')

    monkeypatch.setattr(cpu_backend, 'truss_numbers', no_device)
    monkeypatch.setattr(NetworkxInterface, '_device_graph', no_device)
    monkeypatch.setattr(NetworkxInterface, '_structure_csrs', no_device)
    D = nx.gnm_random_graph(30, 90, seed=2, directed=True)
    L = nx.karate_club_graph()
    L.add_edge(3, 3)
    functions = (truss_number, node_truss_number, lambda G: k_truss(G, 3))
    for fn in functions:
        with pytest.raises(NotImplementedError, match='directed'):
            fn(D)
        for M in (nx.MultiGraph([(0, 1), (0, 1), (1, 2)]), nx.MultiGraph([(0, 1), (1, 2)])):
            with pytest.raises(NotImplementedError, match='multigraph'):
                fn(M)
        with pytest.raises(NotImplementedError, match=r'G\.remove_edges_from\(nx\.selfloop_edges\(G\)\)'):
            fn(L)
    with pytest.raises(NotImplementedError, match='selfloop_edges'):
        truss_number(CSRGraph(4, np.array([0, 1, 2]), np.array([1, 2, 2])))
    for fn in (truss_number, node_truss_number):
        with pytest.raises(TypeError, match='supported libraries'):
            fn({'not': 'a graph'})
    with pytest.raises(TypeError, match='truss_number'):
        k_truss(CSRGraph(3, np.array([0, 1]), np.array([1, 2])), 3)
    assert cpu_backend.calls == []


def test_csr_input(cpu_backend):
    from graphrole_amd import node_truss_number, truss_number
    from graphrole_amd.graph.csr import CSRGraph
    G = nx.barabasi_albert_graph(60, 3, seed=8)
    src, dst = np.array(list(G.edges)).T
    g = CSRGraph(60, src, dst)
    a, b = truss_number(g), truss_number(G)
    assert list(a.index) == list(b.index) and a.to_numpy().tobytes() == b.to_numpy().tobytes()
    assert node_truss_number(g).to_numpy().tobytes() == node_truss_number(G).to_numpy().tobytes()


# ----------------------------------------------------------------------------------------------------------- the ABI
def test_ctypes_signatures_and_exports():
    import graphrole_amd
    from graphrole_amd import _lib, measures
    assert len(_lib._SIGNATURES['grx_truss_numbers'][1]) == 13
    assert len(_lib._SIGNATURES['grx_truss_numbers_workspace_bytes'][1]) == 2
    assert {'grx_truss_numbers', 'grx_truss_numbers_workspace_bytes'} <= set(_lib.EXPORTED_SYMBOLS)
    for name in ('truss_number', 'node_truss_number', 'k_truss'):
        assert getattr(graphrole_amd, name) is getattr(measures, name)
        assert name not in measures.CATALOGUE and name not in measures.OPT_IN
    assert len(measures.CATALOGUE) == 16 and len(measures.OPT_IN) == 8


def test_header_version_and_declarations():
    header = open(os.path.join(ROOT, 'include', 'grx.h')).read()
    assert int(re.search(r'#define\s+GRX_VERSION\s+(\d+)', header).group(1)) == 1100
    assert 'grx_truss_numbers(' in header and 'grx_truss_numbers_workspace_bytes(' in header


def test_argument_validation_needs_no_device():
    """GRX_REQUIRE runs before any HIP call: n range, null pointers, lanes, hub list, a workspace too short for any
    graph; each failure is GRX_ERR_INVALID (-1) with the entry point's name in grx_last_error()."""
    import ctypes
    from graphrole_amd import _lib
    lib = _lib.load()
    assert lib.grx_truss_numbers_workspace_bytes(10, 0) == 6 * 256 + 256
    assert lib.grx_truss_numbers_workspace_bytes(10, 1000) == 6 * 4096 + 256
    need = lib.grx_truss_numbers_workspace_bytes(10, 0)
    p = ctypes.c_void_p(4096)                                   # never dereferenced: every call fails validation

    def call(n=10, row_ptr=p, col=p, hubs=None, n_hubs=0, lanes=8, arc=p, ws=p, ws_bytes=need):
        return lib.grx_truss_numbers(n, row_ptr, col, hubs, n_hubs, lanes, arc, None, None, None, ws, ws_bytes, None)

    for bad in (dict(n=-1), dict(n=1 << 31), dict(row_ptr=None), dict(col=None), dict(arc=None), dict(ws=None),
                dict(lanes=0), dict(lanes=5), dict(lanes=64), dict(n_hubs=3), dict(n_hubs=-1), dict(n_hubs=11, hubs=p),
                dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert call(**bad) == -1, bad
        assert 'grx_truss_numbers' in lib.grx_last_error().decode(), bad
    rounds, levels = ctypes.c_int64(7), ctypes.c_int64(7)
    # n == 0: nothing to do, nothing looked at
    assert lib.grx_truss_numbers(0, None, None, None, 0, 8, None, None, ctypes.byref(rounds), ctypes.byref(levels),
                                 None, 0, None) == 0
    assert rounds.value == 0 and levels.value == 0
