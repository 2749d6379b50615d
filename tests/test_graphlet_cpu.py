"""
-m "not gpu": graphlet degree vectors without a device.  tests/graphlet_oracle.py holds two independent
implementations: ``orbits`` (the numpy restatement of csrc/grx_graphlets.hip: non-induced counts, then the
back-substitution) is compared with ``brute_orbits`` (enumeration of every 3- and 4-subset: the definition) exactly, on
the seeded families of tests/test_truss_cpu.py, on every graph on five labelled nodes and on G(30, p); the matrix A is
re-derived by applying the non-induced formulas to the nine graphlets themselves and compared with the oracle's table
and with the table in the kernel source; the identities with networkx's triangles, degrees and 4-node cliques and with
the squares of tests/square_clustering_oracle.py; then the Python layer of graphrole_amd.graphlet_degree_vectors /
graphlet_counts over a CPU double of kernels.graphlet_orbits (the oracle on the double's CSR arrays); the argument
checks of grx_graphlet_orbits, the ctypes signatures against the header and the unchanged catalogue.  The device
numbers are pinned in tests/test_gpu_graphlets.py.
"""
import ctypes
import itertools
import os
import re
import types

import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import fake_kernels
from tests import graphlet_oracle as go
from tests import square_clustering_oracle as sq
from tests.test_truss_cpu import _families
from tests.truss_oracle import graph_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = [f'orbit_{k}' for k in range(15)]
NAMES = ['edge', 'path3', 'triangle', 'path4', 'star4', 'cycle4', 'paw', 'diamond', 'clique4']


def _check_against_brute_force(G):
    want = go.brute_orbits(G)
    got = go.graph_orbits(G)
    assert got == want
    return want


# ------------------------------------------------------------------------------------------ oracle against brute force
@pytest.mark.parametrize('block', range(2))
def test_oracle_equals_brute_force_on_seeded_graphs(block):
    checked = 0
    seen = np.zeros(15, dtype=np.int64)
    for seed in range(block * 5, block * 5 + 5):
        for G in _families(7919 * seed):
            want = _check_against_brute_force(G)
            seen += np.array(list(want.values()), dtype=np.int64).reshape(-1, 15).sum(axis=0)
            checked += 1
    assert checked == 5 * 13
    assert np.all(seen > 0)                                     # every orbit occurs in the families


def test_oracle_every_graph_on_five_nodes():
    pairs = list(itertools.combinations(range(5), 2))
    seen = np.zeros(15, dtype=np.int64)
    for mask in range(1 << len(pairs)):
        G = nx.empty_graph(5)
        G.add_edges_from(p for k, p in enumerate(pairs) if mask >> k & 1)
        want = _check_against_brute_force(G)
        seen += np.array(list(want.values()), dtype=np.int64).sum(axis=0)
    assert np.all(seen > 0)


@pytest.mark.parametrize('p', [0.1, 0.3, 0.6])
def test_oracle_equals_brute_force_on_gnp(p):
    want = _check_against_brute_force(nx.gnp_random_graph(30, p, seed=7))
    assert sum(o[0] for o in want.values()) > 0


def test_oracle_named_graphs():
    want = _check_against_brute_force(nx.karate_club_graph())
    assert np.all(np.array(list(want.values())).sum(axis=0) > 0)          # karate has every one of the 15 orbits
    for G in (nx.empty_graph(0), nx.empty_graph(1), nx.empty_graph(5), nx.path_graph(2), nx.path_graph(4),
              nx.star_graph(3), nx.cycle_graph(4), nx.complete_graph(3), nx.complete_graph(4), nx.complete_graph(5),
              nx.grid_2d_graph(4, 4), nx.complete_bipartite_graph(4, 5), nx.wheel_graph(9)):
        _check_against_brute_force(G)
    # what the scalar measures cannot tell apart
    star, path = go.brute_orbits(nx.star_graph(3)), go.brute_orbits(nx.path_graph(4))
    assert star[0][7] == 1 and star[0][5] == 0 and path[1][5] == 1 and path[1][7] == 0
    paw = go.brute_orbits(nx.Graph([(0, 1), (1, 2), (2, 0), (0, 3)]))
    assert [paw[v].index(1, 4) for v in (3, 1, 2, 0)] == [9, 10, 10, 11]
    diamond = go.brute_orbits(nx.Graph([(0, 1), (1, 2), (2, 3), (3, 0), (0, 2)]))
    assert diamond[1][12] == diamond[3][12] == 1 and diamond[0][13] == diamond[2][13] == 1
    assert all(o[14] == 1 for o in go.brute_orbits(nx.complete_graph(4)).values())


# ------------------------------------------------------------------------------------------------------- the matrix
GRAPHLETS = {                                                   # name -> (edges, {orbit: a node on it})
    'edge': ([(0, 1)], {0: 0}),
    'path3': ([(0, 1), (1, 2)], {1: 0, 2: 1}),
    'triangle': ([(0, 1), (1, 2), (2, 0)], {3: 0}),
    'path4': ([(0, 1), (1, 2), (2, 3)], {4: 0, 5: 1}),
    'star4': ([(0, 1), (0, 2), (0, 3)], {6: 1, 7: 0}),
    'cycle4': ([(0, 1), (1, 2), (2, 3), (3, 0)], {8: 0}),
    'paw': ([(0, 1), (1, 2), (2, 0), (0, 3)], {9: 3, 10: 1, 11: 0}),
    'diamond': ([(0, 1), (1, 2), (2, 3), (3, 0), (0, 2)], {12: 1, 13: 0}),
    'clique4': ([(a, b) for a, b in itertools.combinations(range(4), 2)], {14: 0}),
}
SIZE_OF_ORBIT = [2, 3, 3, 3] + [4] * 11


def _derived_matrix():
    """A[k][c] = the non-induced count N_k, by the formulas, at a node of orbit c of the graphlet that holds orbit c --
    for the orbits k of graphlets with as many nodes (a copy of a smaller graphlet inside is counted by its own
    orbits)."""
    derived = np.zeros((15, 15), dtype=np.int64)
    for edges, where in GRAPHLETS.values():
        G = nx.Graph(edges)
        nodes, row_ptr, col = graph_csr(G)
        non = go.orbits(row_ptr, col).noninduced
        brute = go.brute_orbits(G)
        for c, v in where.items():
            assert brute[v][c] == 1 and sum(brute[v][k] for k in range(15) if SIZE_OF_ORBIT[k] == len(G)) == 1
            for k in range(15):
                if SIZE_OF_ORBIT[k] == SIZE_OF_ORBIT[c]:
                    derived[k, c] = non[k, nodes.index(v)]
    return derived


def test_matrix_is_what_the_formulas_give_on_the_nine_graphlets():
    derived = _derived_matrix()
    assert np.array_equal(derived, go.A)
    assert np.array_equal(np.triu(derived), derived) and np.all(np.diag(derived) == 1)     # unit upper triangular
    source = open(os.path.join(ROOT, 'graphrole_amd', 'csrc', 'grx_graphlets.hip')).read()
    body = re.search(r'GL_A\[GL_ORBITS\]\[GL_ORBITS\]\s*=\s*\{(.*?)\};', source, re.S).group(1)
    in_kernel = np.array([int(x) for x in re.findall(r'\d+', body)], dtype=np.int64).reshape(15, 15)
    assert np.array_equal(in_kernel, derived)


# ------------------------------------------------------------------------------------------------------ identities
@pytest.mark.parametrize('make', [nx.karate_club_graph, lambda: nx.gnp_random_graph(30, 0.3, seed=7),
                                  lambda: nx.barabasi_albert_graph(300, 4, seed=5),
                                  lambda: nx.gnm_random_graph(60, 500, seed=1)])
def test_identities(make):
    G = make()
    nodes, row_ptr, col = graph_csr(G)
    o = go.orbits(row_ptr, col).orbits
    assert dict(zip(nodes, o[3].tolist())) == nx.triangles(G)
    assert dict(zip(nodes, o[0].tolist())) == dict(G.degree())
    squares = sq.square_clustering(row_ptr, col)[0]
    assert np.array_equal(o[8] + o[12] + o[13] + 3 * o[14], squares)
    cliques4 = sum(1 for c in nx.enumerate_all_cliques(G) if len(c) == 4)
    assert int(o[14].sum()) == 4 * cliques4


# ------------------------------------------------------------------------------------------ Python layer, CPU double
@pytest.fixture
def cpu_backend():
    import torch
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.calls = []

    def graphlet_orbits(csr, want_noninduced=False, want_arc_triangles=False, lanes=None):
        double.calls.append((csr, want_noninduced, want_arc_triangles, lanes))
        r = go.orbits(csr.row_ptr, csr.col)
        return (torch.from_numpy(r.orbits), torch.from_numpy(r.noninduced) if want_noninduced else None,
                torch.from_numpy(r.arc_triangles) if want_arc_triangles else None)

    double.graphlet_orbits = graphlet_orbits
    backend.use(double)
    yield double
    backend.use(None)


def _disconnected():
    G = nx.disjoint_union(nx.barabasi_albert_graph(40, 3, seed=1), nx.cycle_graph(9))
    G.add_nodes_from([1000, 1001])
    return G


GRAPHS = {
    'karate': nx.karate_club_graph,
    'gnp': lambda: nx.gnp_random_graph(30, 0.3, seed=7),
    'disconnected': _disconnected,
    'strings': lambda: nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
    'grid': lambda: nx.grid_2d_graph(4, 5),
    'k2': lambda: nx.path_graph(2),
}


def _expected_totals(want):
    s = np.array(list(want.values()), dtype=np.int64).reshape(-1, 15).sum(axis=0)
    return dict(edge=s[0] // 2, path3=s[2], triangle=s[3] // 3, path4=s[4] // 2, star4=s[7], cycle4=s[8] // 4, paw=s[9],
                diamond=s[13] // 2, clique4=s[14] // 4)


@pytest.mark.parametrize('key', list(GRAPHS))
def test_public_functions(cpu_backend, key):
    from graphrole_amd import graphlet_counts, graphlet_degree_vectors
    G = GRAPHS[key]()
    want = go.brute_orbits(G)
    frame = graphlet_degree_vectors(G)
    assert isinstance(frame, pd.DataFrame) and list(frame.columns) == COLUMNS
    assert all(dt == np.int64 for dt in frame.dtypes)
    assert list(frame.index) == sorted(G)
    assert {v: frame.loc[[v]].to_numpy()[0].tolist() for v in G} == want
    assert len(cpu_backend.calls) == 1 and cpu_backend.calls[0][1:] == (False, False, None)
    totals = _expected_totals(want)
    assert frame.attrs['graphlets'] == totals and list(frame.attrs['graphlets']) == NAMES
    assert totals['edge'] == G.number_of_edges() and totals['triangle'] == sum(nx.triangles(G).values()) // 3
    # path4 and diamond: both orbits of the graphlet give the same total
    s = frame.to_numpy().sum(axis=0)
    assert s[4] == s[5] and s[12] == s[13] and s[6] == 3 * s[7] and s[1] == 2 * s[2] and s[10] == 2 * s[9] == 2 * s[11]
    counts = graphlet_counts(G)
    assert isinstance(counts, pd.Series) and counts.dtype == np.int64 and counts.name == 'graphlet_counts'
    assert list(counts.index) == NAMES and counts.to_dict() == totals
    # the kernel got the structure CSR of the adapter
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    ref = NetworkxInterface(G)._structure_csrs()[0]
    for csr, *_ in cpu_backend.calls:
        assert np.array_equal(csr.row_ptr, ref.row_ptr) and np.array_equal(csr.col, ref.col)


def test_nodes_argument(cpu_backend):
    from graphrole_amd import graphlet_degree_vectors
    G = GRAPHS['strings']()
    full = graphlet_degree_vectors(G)
    one = graphlet_degree_vectors(G, 'node-05')
    assert isinstance(one, pd.Series) and list(one.index) == COLUMNS and one.dtype == np.int64
    assert one.tolist() == full.loc['node-05'].tolist()
    some = graphlet_degree_vectors(G, ['node-33', 'node-00', 'not-a-node', 'node-07'])
    assert isinstance(some, pd.DataFrame) and list(some.index) == ['node-00', 'node-07', 'node-33']
    assert some.equals(full.loc[['node-00', 'node-07', 'node-33']])
    none = graphlet_degree_vectors(G, ['not-a-node'])
    assert isinstance(none, pd.DataFrame) and len(none) == 0 and list(none.columns) == COLUMNS
    # the totals are those of the whole graph whatever the selection
    assert one.attrs['graphlets'] == some.attrs['graphlets'] == none.attrs['graphlets'] == full.attrs['graphlets']


def test_columns_join_the_measure_table(cpu_backend):
    from graphrole_amd import graphlet_degree_vectors, node_measures
    G = _disconnected()
    M = node_measures(G, ['weighted_degree'])
    M = M.join(graphlet_degree_vectors(G))
    assert list(M.columns) == ['weighted_degree'] + COLUMNS and not M.isna().any().any()
    assert (M['orbit_0'] == M['weighted_degree']).all()
    assert M.loc[1000].tolist() == [0] * 16 and M.loc[1001].tolist() == [0] * 16


def test_empty_and_edgeless_graphs_make_no_kernel_call(cpu_backend):
    from graphrole_amd import graphlet_counts, graphlet_degree_vectors
    for G in (nx.empty_graph(0), nx.empty_graph(5)):
        frame = graphlet_degree_vectors(G)
        assert list(frame.columns) == COLUMNS and all(dt == np.int64 for dt in frame.dtypes)
        assert list(frame.index) == list(G) and not frame.to_numpy().any()
        assert frame.attrs['graphlets'] == dict.fromkeys(NAMES, 0)
        assert graphlet_counts(G).tolist() == [0] * 9
    assert cpu_backend.calls == []


def test_every_refusal_makes_no_device_call(cpu_backend, monkeypatch):
    from graphrole_amd import graphlet_counts, graphlet_degree_vectors
    from graphrole_amd.graph.csr import CSRGraph
    from graphrole_amd.graph.interface.networkx import NetworkxInterface

    def no_device(*args, **kwargs):
        raise AssertionError('device work for a refused graph')

    monkeypatch.setattr(cpu_backend, 'graphlet_orbits', no_device)
    monkeypatch.setattr(NetworkxInterface, '_device_graph', no_device)
    monkeypatch.setattr(NetworkxInterface, '_structure_csrs', no_device)
    D = nx.gnm_random_graph(30, 90, seed=2, directed=True)
    L = nx.karate_club_graph()
    L.add_edge(3, 3)
    for fn in (graphlet_degree_vectors, graphlet_counts):
        with pytest.raises(NotImplementedError, match=r'directed.*G\.to_undirected\(\)'):
            fn(D)
        for M in (nx.MultiGraph([(0, 1), (0, 1), (1, 2)]), nx.MultiGraph([(0, 1), (1, 2)])):
            with pytest.raises(NotImplementedError, match=r'multigraph.*nx\.Graph\(G\)'):
                fn(M)
        with pytest.raises(NotImplementedError, match=r'G\.remove_edges_from\(nx\.selfloop_edges\(G\)\)'):
            fn(L)
        with pytest.raises(TypeError, match='supported libraries'):
            fn({'not': 'a graph'})
    with pytest.raises(NotImplementedError, match='selfloop_edges'):
        graphlet_degree_vectors(CSRGraph(4, np.array([0, 1, 2]), np.array([1, 2, 2])))
    assert cpu_backend.calls == []


def test_csr_input(cpu_backend):
    from graphrole_amd import graphlet_degree_vectors
    from graphrole_amd.graph.csr import CSRGraph
    G = nx.barabasi_albert_graph(60, 3, seed=8)
    src, dst = np.array(list(G.edges)).T
    a, b = graphlet_degree_vectors(CSRGraph(60, src, dst)), graphlet_degree_vectors(G)
    assert list(a.index) == list(b.index) and a.to_numpy().tobytes() == b.to_numpy().tobytes()


# ----------------------------------------------------------------------------------------------------------- the ABI
_C_TYPES = {'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'size_t': ctypes.c_size_t}


def _declared(header, name):
    """(restype, [argtypes]) of `name` as include/grx.h declares it: every pointer is a c_void_p."""
    ret, args = re.search(r'^(\w+)\s+' + name + r'\(([^)]*)\);', header, re.M).groups()
    out = []
    for arg in args.split(','):
        words = arg.replace('const', '').split()
        out.append(ctypes.c_void_p if '*' in arg else _C_TYPES[words[0]])
    return _C_TYPES[ret], out


def test_ctypes_signatures_match_the_header_and_the_catalogue_is_unchanged():
    import graphrole_amd
    from graphrole_amd import _lib, measures
    header = open(os.path.join(ROOT, 'include', 'grx.h')).read()
    for name, n_args in (('grx_graphlet_orbits', 15), ('grx_graphlet_orbits_workspace_bytes', 2)):
        restype, argtypes = _declared(header, name)
        assert len(argtypes) == n_args
        assert _lib._SIGNATURES[name] == (restype, argtypes)
        assert name in _lib.EXPORTED_SYMBOLS
    assert int(re.search(r'#define\s+GRX_VERSION\s+(\d+)', header).group(1)) == 1100      # added entry points only
    for name in ('graphlet_degree_vectors', 'graphlet_counts'):
        assert getattr(graphrole_amd, name) is getattr(measures, name)
        assert name not in measures.CATALOGUE and name not in measures.OPT_IN
    assert not any('orbit' in name or 'graphlet' in name for name in list(measures.CATALOGUE) + list(measures.OPT_IN))
    assert not any('orbit' in name or 'graphlet' in name for name in measures.available_measures(False, False))
    assert len(measures.CATALOGUE) == 16 and len(measures.OPT_IN) == 8


def test_argument_validation_needs_no_device():
    """GRX_REQUIRE runs before any HIP call: n range, null pointers, lanes, hub list, a workspace too short for any
    graph; each failure is GRX_ERR_INVALID (-1) with the entry point's name in grx_last_error()."""
    from graphrole_amd import _lib
    lib = _lib.load()
    assert lib.grx_graphlet_orbits_workspace_bytes(10, 0) == 10 * 256 + 3 * 256
    assert lib.grx_graphlet_orbits_workspace_bytes(1000, 1000) == 10 * 8192 + 3 * 4096
    need = lib.grx_graphlet_orbits_workspace_bytes(10, 0)
    p = ctypes.c_void_p(4096)                                   # never dereferenced: every call fails validation

    def call(n=10, row_ptr=p, col=p, o_row_ptr=p, o_col=p, hubs=None, n_hubs=0, lanes=8, squares=p, orbits=p, ws=p,
             ws_bytes=need):
        return lib.grx_graphlet_orbits(n, row_ptr, col, o_row_ptr, o_col, hubs, n_hubs, lanes, squares, orbits, None,
                                       None, ws, ws_bytes, None)

    for bad in (dict(n=-1), dict(n=1 << 31), dict(row_ptr=None), dict(col=None), dict(o_row_ptr=None), dict(o_col=None),
                dict(squares=None), dict(orbits=None), dict(ws=None), dict(lanes=0), dict(lanes=5), dict(lanes=64),
                dict(n_hubs=3), dict(n_hubs=-1), dict(n_hubs=11, hubs=p), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert call(**bad) == -1, bad
        assert 'grx_graphlet_orbits' in lib.grx_last_error().decode(), bad
    # n == 0: nothing to do, nothing looked at
    assert lib.grx_graphlet_orbits(0, None, None, None, None, None, 0, 8, None, None, None, None, None, 0, None) == 0
