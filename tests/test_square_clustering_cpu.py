"""
-m "not gpu": the square clustering coefficient without a device.  tests/square_clustering_oracle.py (the array
restatement of grx_square_clustering) against nx.square_clustering, equal as floats, with its two integers against
networkx's own loop; then the Python layer of graphrole_amd.square_clustering over a CPU double of
kernels.square_clustering (the oracle on the double's arrays); the refusal of directed graphs; the catalogue; the ctypes
signature, the header and the argument validation of the library.  The device numbers are pinned in
tests/test_gpu_square_clustering.py.
"""
import ctypes
import os
import random
import re
import types
from itertools import combinations

import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import fake_kernels
from tests import square_clustering_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = 240


def _networkx_counts(G):
    """networkx 3.4.2's loop (cluster.py, square_clustering) with its two integers kept: {v: (clustering, potential)}."""
    out = {}
    for v in G:
        clustering = potential = 0
        for u, w in combinations(G[v], 2):
            squares = len((set(G[u]) & set(G[w])) - {v})
            clustering += squares
            degm = squares + 1
            if w in G[u]:
                degm += 1
            potential += (len(G[u]) - degm) + (len(G[w]) - degm) + squares
        out[v] = (clustering, potential)
    return out


def _arrays(G):
    """The oracle's CSR of a graph whose nodes are 0 .. n - 1."""
    assert sorted(G) == list(range(len(G)))
    return so.csr_from_pairs(len(G), list(G.edges))


def _check_against_networkx(G, what):
    row_ptr, col = _arrays(G)
    Q, P, C = so.square_clustering(row_ptr, col)
    want, counts = nx.square_clustering(G), _networkx_counts(G)
    for v in range(len(G)):
        assert (int(Q[v]), int(P[v])) == counts[v], (what, v)
        assert float(C[v]) == float(want[v]), (what, v)
    some = [v for v in range(len(G)) if v % 3 == 1]
    q, p, c = so.square_clustering(row_ptr, col, some)
    assert np.array_equal(q, Q[some]) and np.array_equal(p, P[some]) and np.array_equal(c, C[some])


def _random_graph(i):
    """Graph i of the family: gnm and Barabasi-Albert, 1 to 60 nodes, every third with self-loops."""
    rng = random.Random(5000 + i)
    n = rng.randint(1, 60)
    if i % 2 == 0 or n < 3:
        G = nx.gnm_random_graph(n, rng.randint(0, min(4 * n, n * (n - 1) // 2)), seed=i)
    else:
        G = nx.barabasi_albert_graph(n, rng.randint(1, min(5, n - 1)), seed=i)
    if i % 3 == 0:
        G.add_edges_from((v, v) for v in rng.sample(list(G), max(1, n // 5)))
    return G


@pytest.mark.parametrize('batch', range(8))
def test_oracle_against_networkx(batch):
    for i in range(30 * batch, 30 * batch + 30):
        _check_against_networkx(_random_graph(i), i)


def test_the_family_has_loops_squares_and_both_generators():
    graphs = [_random_graph(i) for i in range(FAMILY)]
    assert sum(nx.number_of_selfloops(G) > 0 for G in graphs) >= FAMILY // 3
    assert min(len(G) for G in graphs) == 1 and max(len(G) for G in graphs) == 60
    assert sum(any(c > 0 for c in nx.square_clustering(G).values()) for G in graphs[:40]) > 20


def test_oracle_against_networkx_on_named_graphs():
    for name, G in (('karate', nx.karate_club_graph()), ('K6', nx.complete_graph(6)),
                    ('K4,5', nx.complete_bipartite_graph(4, 5)), ('C4', nx.cycle_graph(4)),
                    ('petersen', nx.petersen_graph()),
                    ('grid', nx.convert_node_labels_to_integers(nx.grid_2d_graph(6, 6))), ('star', nx.star_graph(20)),
                    ('P2', nx.path_graph(2)), ('P3', nx.path_graph(3)), ('empty5', nx.empty_graph(5)),
                    ('empty0', nx.empty_graph(0)), ('n1', nx.empty_graph(1))):
        _check_against_networkx(G, name)
    L = nx.karate_club_graph()
    L.add_edges_from([(0, 0), (1, 1), (33, 33), (11, 11)])      # hubs, a hub's neighbour, a leaf
    _check_against_networkx(L, 'karate with loops')
    assert np.all(so.square_clustering(*_arrays(nx.complete_bipartite_graph(4, 5)))[2] == 1.0)
    assert np.all(so.square_clustering(*_arrays(nx.complete_graph(6)))[2] == 1.0)
    Q, P, C = so.square_clustering(*_arrays(nx.star_graph(20)))
    assert np.all(C == 0.0) and np.all(Q == 0) and np.all(P[1:] == 0)


def test_oracle_layout_and_wedge_counts():
    row_ptr, col = so.csr_from_pairs(4, [(0, 1), (1, 0), (1, 2), (2, 2), (1, 2)])
    assert row_ptr.tolist() == [0, 1, 3, 5, 5] and col.tolist() == [1, 0, 2, 1, 2] and col.dtype == np.int32
    assert so.wedge_counts(row_ptr, col).tolist() == [2, 1 + 2, 2 + 2, 0]
    G = nx.barabasi_albert_graph(50, 3, seed=1)
    row_ptr, col = _arrays(G)
    assert so.wedge_counts(row_ptr, col).tolist() == [sum(len(G[u]) for u in G[v]) for v in range(50)]


# ------------------------------------------------------------------------------------------ Python layer, CPU double
@pytest.fixture
def cpu_backend():
    import torch
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.calls = []

    from tests import test_sense_cpu as sense               # the double of the degree column the index is compared with
    double.row_counts = sense._row_counts

    def square_clustering(csr, want_counts=False, lanes=None):
        double.calls.append(dict(csr=csr, want_counts=want_counts))
        Q, P, C = so.square_clustering(csr.row_ptr, csr.col)
        return (torch.from_numpy(C), torch.from_numpy(Q) if want_counts else None,
                torch.from_numpy(P) if want_counts else None)

    double.square_clustering = square_clustering
    backend.use(double)
    yield double
    backend.use(None)


def _equals_networkx(series, G, nodes=None):
    assert isinstance(series, pd.Series) and series.name == 'square_clustering' and series.dtype == np.float64
    index = sorted(G) if nodes is None else sorted(set(nodes))
    assert list(series.index) == index
    want = nx.square_clustering(G)
    assert series.to_dict() == {v: float(want[v]) for v in index}


def _with_loops(G):
    G.add_edges_from([(0, 0), (7, 7), (19, 19)])
    return G


API_GRAPHS = {
    'karate': nx.karate_club_graph,
    'strings': lambda: nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
    'loops': lambda: _with_loops(nx.gnp_random_graph(20, 0.3, seed=6)),
    'bipartite': lambda: nx.complete_bipartite_graph(3, 6),
    'isolated': lambda: nx.disjoint_union(nx.cycle_graph(4), nx.empty_graph(2)),
}


@pytest.mark.parametrize('key', list(API_GRAPHS))
def test_series_of_every_node(cpu_backend, key):
    from graphrole_amd import node_measures, square_clustering
    G = API_GRAPHS[key]()
    got = square_clustering(G)
    _equals_networkx(got, G)
    (call,) = cpu_backend.calls
    assert not call['want_counts']
    assert list(got.index) == list(node_measures(G, ['degree']).index)      # joins the table of sense making


def test_nodes_argument(cpu_backend):
    from graphrole_amd import square_clustering
    G = API_GRAPHS['strings']()
    want = nx.square_clustering(G)
    one = square_clustering(G, 'node-05')
    assert isinstance(one, float) and one == want['node-05'] == nx.square_clustering(G, 'node-05')
    bunch = ['node-30', 'node-02', 'nobody', 'node-11', 'node-02']
    _equals_networkx(square_clustering(G, bunch), G, ['node-30', 'node-02', 'node-11'])
    assert set(nx.square_clustering(G, bunch)) == {'node-30', 'node-02', 'node-11'}     # networkx drops it too
    _equals_networkx(square_clustering(G, iter(['node-33'])), G, ['node-33'])
    calls = len(cpu_backend.calls)
    for none in ([], ['nobody']):
        got = square_clustering(G, none)
        assert len(got) == 0 and got.name == 'square_clustering' and got.dtype == np.float64
    assert len(cpu_backend.calls) == calls                      # nothing to compute
    K = nx.karate_club_graph()
    zero = square_clustering(nx.star_graph(5), 0)
    assert isinstance(zero, float) and zero == 0.0              # networkx: the int 0
    _equals_networkx(square_clustering(K, [33, 0, 5]), K, [33, 0, 5])


def test_empty_graph(cpu_backend):
    from graphrole_amd import square_clustering
    got = square_clustering(nx.Graph())
    assert len(got) == 0 and got.name == 'square_clustering' and got.dtype == np.float64
    assert cpu_backend.calls == []
    E = nx.empty_graph(4)
    _equals_networkx(square_clustering(E), E)


def test_multigraph_equals_its_simple_graph(cpu_backend):
    from graphrole_amd import square_clustering
    G = nx.gnm_random_graph(25, 70, seed=4)
    M = nx.MultiGraph(G)
    M.add_edges_from(list(G.edges)[:20])                        # parallel copies
    M.add_edges_from([(3, 3), (3, 3)])
    G.add_edge(3, 3)
    assert np.array_equal(square_clustering(M).to_numpy(), square_clustering(G).to_numpy())
    _equals_networkx(square_clustering(M), M)                   # networkx gives the simple graph's value as well


def test_csr_graph_input(cpu_backend):
    from graphrole_amd import square_clustering
    from graphrole_amd.graph.csr import CSRGraph
    G = nx.karate_club_graph()
    src, dst = zip(*G.edges())
    C = CSRGraph(34, src, dst)
    got = square_clustering(C)
    assert np.array_equal(got.to_numpy(), square_clustering(G).to_numpy()) and list(got.index) == sorted(G)


def test_directed_graphs_are_refused_before_any_device_work(cpu_backend, monkeypatch):
    from graphrole_amd import square_clustering
    from graphrole_amd.graph.csr import CSRGraph
    from graphrole_amd.graph.interface.base import DeviceGraphInterface

    def fail(self):
        raise AssertionError('_device_graph was called')

    monkeypatch.setattr(DeviceGraphInterface, '_device_graph', fail)
    for D in (nx.DiGraph([(0, 1), (1, 2), (2, 0)]), nx.MultiDiGraph([(0, 1), (0, 1)]),
              CSRGraph(3, [0, 1], [1, 2], directed=True)):
        for nodes in (None, 0, [0, 1]):
            with pytest.raises(NotImplementedError, match='insertion order'):
                square_clustering(D, nodes)
    assert cpu_backend.calls == []
    with pytest.raises(TypeError, match='supported libraries'):
        square_clustering({'not': 'a graph'})


def test_catalogue_and_opt_in_are_unchanged():
    from graphrole_amd import measures
    names = list(measures.CATALOGUE)
    assert len(names) == 16 and len(measures.OPT_IN) == 8 and names[-1] == 'eccentricity'
    assert 'square_clustering' not in measures.CATALOGUE and 'square_clustering' not in measures.OPT_IN
    for directed in (False, True):
        for multi in (False, True):
            assert 'square_clustering' not in measures.available_measures(directed, multi)
    assert measures.available_measures(False, False) == ['degree', 'weighted_degree', 'clustering', 'effective_size',
                                                         'pagerank', 'eigenvector']
    import graphrole_amd
    assert graphrole_amd.square_clustering is measures.square_clustering
    with pytest.raises(ValueError):
        graphrole_amd.node_measures(nx.path_graph(3), ['square_clustering'])


# ---------------------------------------------------------------------------------------------------------- ABI
_C_TYPES = {'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'size_t': ctypes.c_size_t, 'double': ctypes.c_double}


def _declared_arguments(header, name):
    text = re.search(r'\b' + name + r'\s*\(([^)]*)\)\s*;', header).group(1)
    out = []
    for arg in text.split(','):
        arg = ' '.join(arg.split())
        out.append(ctypes.c_void_p if '*' in arg else _C_TYPES[arg.replace('const ', '').rsplit(' ', 1)[0]])
    return out


def test_header_declaration_matches_the_ctypes_signature():
    from graphrole_amd import _lib, kernels
    header = open(os.path.join(ROOT, 'include', 'grx.h')).read()
    for name, restype in (('grx_square_clustering', ctypes.c_int),
                          ('grx_square_clustering_workspace_bytes', ctypes.c_size_t)):
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[name] == (restype, _declared_arguments(header, name))
    assert len(_lib._SIGNATURES['grx_square_clustering'][1]) == 12
    assert int(re.search(r'#define\s+GRX_VERSION\s+(\d+)', header).group(1)) == 1100      # an added entry point only
    assert 'below 2^53' in header and 'n < 2^31' in header
    assert callable(kernels.square_clustering)
    source = open(os.path.join(ROOT, 'graphrole_amd', 'csrc', 'grx_square_clustering.hip')).read()
    assert '#include "grx_rowjoin.h"' in source and '#pragma clang fp contract(off)' in source
    for constant in ('SQ_WAVE_MAX_WEDGES', 'SQ_LDS_MAX_WEDGES'):       # the copies the GPU test sizes its rows by
        assert int(re.search(r'constexpr int ' + constant + r' = (\d+);', source).group(1)) == getattr(kernels, constant)
    assert 'grx_square_clustering.hip' in open(os.path.join(ROOT, 'graphrole_amd', 'csrc', 'Makefile')).read()


def test_argument_validation_needs_no_device():
    """GRX_REQUIRE runs before any HIP call: n range, no output, null pointers, lanes, hub list, a workspace that is too
    small.  n = 0 is an empty result."""
    from graphrole_amd import _lib
    lib = _lib.load()
    size = lib.grx_square_clustering_workspace_bytes
    assert 8 * 1000 + 128 * 4 * 1000 <= size(1000) <= 8 * 1000 + 128 * 4 * 1000 + 129 * 256      # the stated formula
    assert size(0) > 0 and size(1001) >= size(1000)
    need = size(10)
    p = ctypes.c_void_p(4096)                                   # never dereferenced: every call fails validation

    def call(n=10, row_ptr=p, col=p, hubs=None, n_hubs=0, lanes=8, out=p, squares=None, potential=None, ws=p,
             ws_bytes=need):
        return lib.grx_square_clustering(n, row_ptr, col, hubs, n_hubs, lanes, out, squares, potential, ws, ws_bytes,
                                         None)

    for bad in (dict(n=-1), dict(n=1 << 31), dict(out=None), dict(row_ptr=None), dict(col=None), dict(ws=None),
                dict(lanes=0), dict(lanes=12), dict(lanes=64), dict(n_hubs=3), dict(n_hubs=-1), dict(n_hubs=11, hubs=p),
                dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert call(**bad) == -1, bad
        assert b'grx_square_clustering' in lib.grx_last_error()
    assert call(n=0, row_ptr=None, col=None, ws=None, ws_bytes=0) == 0
    assert call(n=0, out=None) == -1                            # the output is required even then
