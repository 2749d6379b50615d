"""
-m "not gpu": constraint and the weighted / directed effective size without a device.  tests/structural_holes_oracle.py
(the two array restatements of grx_structural_holes) against nx.constraint, nx.local_constraint and nx.effective_size
inside the tolerances the oracle module derives; then the Python layer of graphrole_amd.constraint / effective_size /
node_measures over a CPU double of kernels.structural_holes (the exact oracle on the double's arrays); the refusals;
the catalogue; the ctypes signature, the header and the argument validation of the library.  The device numbers are
pinned in tests/test_gpu_structural_holes.py.
"""
import ctypes
import os
import random
import re
import types

import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import fake_kernels
from tests import structural_holes_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_graph(i):
    """Graph i of the family: undirected and directed, self-loops, integer / float / zero weights, isolated nodes,
    directed nodes with in-arcs only."""
    rng = random.Random(1000 + i)
    n = rng.randint(2, 25)
    directed = i % 2 == 1
    G = nx.gnp_random_graph(n, rng.choice([0.08, 0.2, 0.45]), seed=i, directed=directed)
    if i % 3 == 0:
        G.add_edges_from((v, v) for v in rng.sample(list(G), min(3, n)))
    if i % 5 == 0:
        G.add_nodes_from([n, n + 1])                            # isolated
    if directed and i % 7 == 1:
        G.add_edges_from((v, n + 2) for v in rng.sample(range(n), min(2, n)))      # n + 2 has in-arcs only
    kind = i % 4
    for u, v in G.edges:
        if kind == 0:
            G[u][v]['weight'] = rng.choice([0, 1, 2, 5])        # integers and zeros
        elif kind == 1:
            G[u][v]['weight'] = rng.random()
        elif kind == 2 and rng.random() < 0.5:
            G[u][v]['weight'] = rng.choice([0.0, 0.25, 3.5])    # some edges without the attribute: they count 1
    return G


def _networkx_triple(G, weight, rp, col, nodes, arcs):
    """(constraint, effective size, local constraint at `arcs`) of networkx in the oracle's layout.  effective_size
    takes the weighted form whenever weight is given or G is directed; for the undirected unweighted case the weighted
    form is asked for with an attribute no edge has (every edge then counts 1)."""
    con = nx.constraint(G, weight=weight)
    es = nx.effective_size(G, weight=weight if (weight is not None or G.is_directed()) else 'no such attribute')
    rows = np.repeat(np.arange(len(nodes)), np.diff(rp))
    loc = [nx.local_constraint(G, nodes[rows[j]], nodes[col[j]], weight=weight) for j in arcs]
    return np.array([con[v] for v in nodes]), np.array([es[v] for v in nodes]), np.array(loc)


def _check_against_networkx(G, weight, what, max_arcs=8):
    nodes = sorted(G)
    rp, col, z, orp = so.mutual_csr(G, weight)
    rng = random.Random(len(col))
    arcs = sorted(rng.sample(range(len(col)), min(max_arcs, len(col))))
    want = _networkx_triple(G, weight, rp, col, nodes, arcs)
    for restate in (so.exact, so.sparse):
        con, es, loc = restate(rp, col, z, orp)
        assert len(loc) == len(col)
        # local constraint is compared at the sampled arcs; the bound is relative, so rows of one entry serve
        assert np.array_equal(np.isnan(loc[arcs]), np.isnan(want[2]))
        assert np.all(np.abs(loc[arcs] - want[2]) <= so.RTOL * np.abs(want[2])), (what, restate.__name__)
        so.assert_close((con, es, None), (want[0], want[1], None), rp, (what, restate.__name__))


@pytest.mark.parametrize('batch', range(8))
def test_oracles_against_networkx(batch):
    """240 graphs of at most 28 nodes, each with weight=None and weight='weight': NaNs in the same places."""
    for i in range(30 * batch, 30 * batch + 30):
        G = _random_graph(i)
        for weight in (None, 'weight'):
            _check_against_networkx(G, weight, (i, weight))


def test_oracles_against_networkx_on_karate_and_named_graphs():
    K = nx.karate_club_graph()                                  # carries its own integer weights
    _check_against_networkx(K, 'weight', 'karate weighted', max_arcs=20)
    _check_against_networkx(K, None, 'karate')
    _check_against_networkx(nx.star_graph(12), None, 'star')
    _check_against_networkx(nx.complete_graph(9), None, 'K9')
    _check_against_networkx(nx.complete_bipartite_graph(4, 5), None, 'K4,5')
    _check_against_networkx(nx.wheel_graph(14), None, 'wheel')
    _check_against_networkx(nx.path_graph(2), None, 'P2')
    _check_against_networkx(nx.empty_graph(3), None, 'empty')
    D = nx.DiGraph([(0, 1), (1, 0), (1, 2), (3, 1), (2, 2), (2, 4)])      # reciprocal pair, loop, in-only, out-only
    _check_against_networkx(D, None, 'digraph')
    Z = nx.Graph()
    Z.add_weighted_edges_from([(0, 1, 0.0), (0, 2, 0.0), (1, 2, 3.0), (2, 3, 1.0)])     # S(0) = 0
    _check_against_networkx(Z, 'weight', 'zero weights')
    con = so.exact(*so.mutual_csr(Z, 'weight'))[0]
    assert con[0] == 0.0


def test_oracle_layout_and_null_weights():
    G = nx.DiGraph([(0, 1), (1, 0), (1, 2), (2, 2), (3, 1)])
    rp, col, z, orp = so.mutual_csr(G, None)
    assert rp.tolist() == [0, 1, 4, 6, 7] and col.tolist() == [1, 0, 2, 3, 1, 2, 1]
    assert z.tolist() == [2, 2, 1, 1, 1, 2, 1]                  # reciprocal pair summed, the loop twice
    assert orp.tolist() == [0, 1, 3, 4, 5]
    U = nx.barabasi_albert_graph(40, 3, seed=2)
    rp, col, z, orp = so.mutual_csr(U, None)
    assert np.all(z == 2.0) and np.array_equal(rp, orp)
    a, b = so.exact(rp, col, z), so.exact(rp, col, None)       # the factor 2 cancels exactly
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    rp2, col2, z2 = so.csr_from_pairs(40, list(U.edges))
    assert np.array_equal(rp2, rp) and np.array_equal(col2, col) and z2 is None


# ------------------------------------------------------------------------------------------ Python layer, CPU double
@pytest.fixture
def cpu_backend():
    import torch
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.calls = []

    from tests import test_sense_cpu as sense               # the doubles of the existing effective_size column
    double.row_counts = sense._row_counts
    double.triangle_counts = sense._triangle_counts
    double.local_structure = sense._local_structure

    def structural_holes(csr, z=None, out_row_ptr=None, want_constraint=True, want_effective_size=False,
                         want_local=False):
        z = None if z is None else np.asarray(z, dtype=np.float64)
        orp = None if out_row_ptr is None else np.asarray(out_row_ptr, dtype=np.int64)
        double.calls.append(dict(csr=csr, z=z, out_row_ptr=orp, constraint=want_constraint,
                                 effective_size=want_effective_size, local=want_local))
        con, es, loc = so.exact(csr.row_ptr, csr.col, z, orp)
        return (torch.from_numpy(con) if want_constraint else None,
                torch.from_numpy(es) if want_effective_size else None,
                torch.from_numpy(loc) if want_local else None)

    double.structural_holes = structural_holes
    backend.use(double)
    yield double
    backend.use(None)


def _series_close(series, want: dict, name, G):
    assert isinstance(series, pd.Series) and series.name == name and series.dtype == np.float64
    assert list(series.index) == sorted(want)
    got = series.to_numpy()
    ref = np.array([want[v] for v in series.index])
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    if name == 'constraint':
        assert np.all(np.abs(got[ok] - ref[ok]) <= so.RTOL * np.abs(ref[ok]))
    else:
        deg = np.array([max(len(set(nx.all_neighbors(G, v))), 1) for v in series.index])
        assert np.all(np.abs(got[ok] - ref[ok]) <= so.ES_ATOL * deg[ok])


def _weighted_digraph(n=25, m=90, seed=3):
    G = nx.gnm_random_graph(n, m, seed=seed, directed=True)
    rng = random.Random(seed)
    for u, v in G.edges:
        G[u][v]['weight'] = rng.choice([0.5, 1.0, 2.0, 7.25])
    G.add_edges_from([(0, 0, {'weight': 3.0}), (4, 4, {'weight': 0.5})])
    G.add_node(n)                                               # isolated
    G.add_edge(1, n + 1, weight=2.0)                            # n + 1 has an in-arc only
    return G


API_GRAPHS = {
    'karate': nx.karate_club_graph,
    'strings': lambda: nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
    'loops': lambda: _with_loops(nx.gnp_random_graph(20, 0.3, seed=6)),
    'digraph': _weighted_digraph,
    'isolated': lambda: nx.disjoint_union(nx.path_graph(4), nx.empty_graph(2)),
}


def _with_loops(G):
    G.add_edges_from([(0, 0), (7, 7), (19, 19)])
    return G


@pytest.mark.parametrize('key', list(API_GRAPHS))
@pytest.mark.parametrize('weight', [None, 'weight'])
def test_constraint_and_effective_size_of_every_node(cpu_backend, key, weight):
    from graphrole_amd import constraint, effective_size
    G = API_GRAPHS[key]()
    _series_close(constraint(G, weight=weight), nx.constraint(G, weight=weight), 'constraint', G)
    (call,) = cpu_backend.calls
    assert call['constraint'] and not call['effective_size'] and not call['local']
    cpu_backend.calls.clear()
    _series_close(effective_size(G, weight=weight), nx.effective_size(G, weight=weight), 'effective_size', G)
    if G.is_directed() or weight is not None:
        (call,) = cpu_backend.calls
        assert call['effective_size'] and not call['constraint'] and not call['local']
    else:
        assert cpu_backend.calls == []                          # the existing column: networkx's n - 2t/n


def test_undirected_unweighted_effective_size_is_the_existing_column(cpu_backend):
    from graphrole_amd import effective_size, node_measures
    G = API_GRAPHS['loops']()
    got = effective_size(G)
    old = node_measures(G, ['effective_size'])['effective_size']
    assert got.name == 'effective_size' and np.array_equal(got.to_numpy(), old.to_numpy(), equal_nan=True)
    assert list(got.index) == list(old.index)


def test_mutual_weight_csr_of_the_undirected_graph_is_the_device_graph(cpu_backend):
    from graphrole_amd import constraint
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    G = nx.karate_club_graph()
    constraint(G, weight='weight')
    constraint(G)
    weighted, plain = cpu_backend.calls
    _, out, _ = NetworkxInterface(G)._device_graph()
    for call in (weighted, plain):
        assert np.array_equal(call['csr'].row_ptr, out.row_ptr) and np.array_equal(call['csr'].col, out.col)
        assert call['out_row_ptr'] is None
    assert np.array_equal(weighted['z'], out.w) and plain['z'] is None      # w for z = 2 w: the factor cancels


def test_directed_symmetrisation_doubles_loops_and_sums_reciprocal_arcs(cpu_backend):
    from graphrole_amd import constraint
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    D = nx.DiGraph()
    D.add_weighted_edges_from([('a', 'b', 1.5), ('b', 'a', 2.0), ('b', 'c', 4.0), ('c', 'c', 0.75), ('d', 'b', 8.0)])
    adapter = NetworkxInterface(D)
    host, out, _ = adapter._device_graph()
    labels = sorted(D)
    internal = {v: int(host.inv[i]) for i, v in enumerate(labels)}
    for weight, want in (('weight', {('a', 'b'): 3.5, ('b', 'c'): 4.0, ('c', 'c'): 1.5, ('b', 'd'): 8.0}),
                         (None, {('a', 'b'): 2.0, ('b', 'c'): 1.0, ('c', 'c'): 2.0, ('b', 'd'): 1.0})):
        cpu_backend.calls.clear()
        _series_close(constraint(D, weight=weight), nx.constraint(D, weight=weight), 'constraint', D)
        (call,) = cpu_backend.calls
        csr = call['csr']
        rows = np.repeat(np.arange(csr.n), np.diff(csr.row_ptr))
        got = {(int(r), int(c)): float(v) for r, c, v in zip(rows, csr.col, call['z'])}
        full = {}
        for (u, v), val in want.items():
            full[(internal[u], internal[v])] = val
            full[(internal[v], internal[u])] = val
        assert got == full
        for r in range(csr.n):                                  # ascending and distinct inside a row
            assert np.all(np.diff(csr.col[csr.row_ptr[r]:csr.row_ptr[r + 1]]) > 0)
        assert np.array_equal(call['out_row_ptr'], out.row_ptr)    # len(G[u]): 'd' has one out-arc, 'c' its loop
    # a second call reuses the cached CSR
    constraint(adapter.G, weight=None)


def test_nodes_argument_and_string_labels(cpu_backend):
    from graphrole_amd import constraint, effective_size
    G = API_GRAPHS['strings']()
    bunch = ['node-30', 'node-02', 'node-11', 'node-02']
    got = constraint(G, nodes=bunch, weight='weight')
    assert list(got.index) == ['node-02', 'node-11', 'node-30']
    _series_close(got, nx.constraint(G, nodes=bunch, weight='weight'), 'constraint', G)
    got = effective_size(G, nodes=iter(['node-33']), weight='weight')
    _series_close(got, nx.effective_size(G, nodes=['node-33'], weight='weight'), 'effective_size', G)
    got = effective_size(G, nodes=['node-05', 'node-00'])       # the existing column, sliced
    _series_close(got, nx.effective_size(G, nodes=['node-05', 'node-00']), 'effective_size', G)
    assert len(constraint(G, nodes=[])) == 0
    D = _weighted_digraph()
    _series_close(constraint(D, nodes=[26, 3, 25]), nx.constraint(D, nodes=[26, 3, 25]), 'constraint', D)


def test_node_measures_column_and_weight_keyword(cpu_backend):
    from graphrole_amd import node_measures
    G = nx.karate_club_graph()
    M = node_measures(G, ['weighted_degree', 'constraint', 'constraint'], weight='weight')
    assert list(M.columns) == ['weighted_degree', 'constraint', 'constraint']
    _series_close(M['constraint'].iloc[:, 0].rename('constraint'), nx.constraint(G, weight='weight'), 'constraint', G)
    assert len(cpu_backend.calls) == 1                          # computed once for both columns
    assert M['weighted_degree'].to_dict() == dict(G.degree(weight='weight'))     # `weight` applies to constraint only
    cpu_backend.calls.clear()
    M = node_measures(G, ['constraint'])
    _series_close(M['constraint'], nx.constraint(G), 'constraint', G)
    assert cpu_backend.calls[0]['z'] is None
    D = _weighted_digraph()
    M = node_measures(D, ['out_degree', 'constraint'], weight='weight')
    _series_close(M['constraint'], nx.constraint(D, weight='weight'), 'constraint', D)
    assert list(M.index) == sorted(D)
    node_measures(G, ['degree'], weight='anything')            # not validated unless 'constraint' is named


def test_csr_graph_input(cpu_backend):
    from graphrole_amd import constraint, effective_size
    from graphrole_amd.graph.csr import CSRGraph
    G = nx.karate_club_graph()
    src, dst, w = zip(*G.edges(data='weight'))
    C = CSRGraph(34, src, dst, weights=np.asarray(w, dtype=np.float64))
    assert np.array_equal(constraint(C, weight='weight').to_numpy(), constraint(G, weight='weight').to_numpy())
    assert np.array_equal(effective_size(C, weight='weight').to_numpy(),
                          effective_size(G, weight='weight').to_numpy())
    D = _weighted_digraph()
    src, dst, w = zip(*D.edges(data='weight'))
    C = CSRGraph(D.number_of_nodes(), src, dst, weights=np.asarray(w), directed=True)
    assert np.array_equal(constraint(C, weight='weight').to_numpy(), constraint(D, weight='weight').to_numpy(),
                          equal_nan=True)


def test_refusals_make_no_kernel_call(cpu_backend):
    from graphrole_amd import constraint, effective_size, node_measures
    from graphrole_amd.graph.csr import CSRGraph
    G = nx.karate_club_graph()
    for call in (lambda: constraint(G, weight='capacity'), lambda: effective_size(G, weight='capacity'),
                 lambda: constraint(G, weight=lambda u, v, d: 1), lambda: node_measures(G, ['constraint'], weight='w')):
        with pytest.raises(NotImplementedError, match=r'nx\.(constraint|effective_size)\(G, weight='):
            call()
    for M in (nx.MultiGraph([(0, 1), (0, 1), (1, 2)]), nx.MultiDiGraph([(0, 1), (1, 0), (1, 2)])):
        for call in (lambda: constraint(M), lambda: effective_size(M, weight='weight'), lambda: effective_size(M),
                     lambda: node_measures(M, ['constraint'])):
            with pytest.raises(NotImplementedError, match='multigraph'):
                call()
    for bad in (-1.0, float('nan'), float('inf')):
        B = nx.path_graph(4)
        B[1][2]['weight'] = bad
        for call in (lambda: constraint(B, weight='weight'), lambda: effective_size(B, weight='weight'),
                     lambda: node_measures(B, ['constraint'], weight='weight')):
            with pytest.raises(ValueError, match='finite and >= 0'):
                call()
        C = CSRGraph(3, [0, 1], [1, 2], weights=[1.0, bad], directed=True)
        with pytest.raises(ValueError, match='finite and >= 0'):
            constraint(C, weight='weight')
    for call in (lambda: constraint(G, nodes=[0, 99]), lambda: effective_size(G, nodes=[99], weight='weight'),
                 lambda: effective_size(G, nodes=[99])):
        with pytest.raises(KeyError):
            call()
    with pytest.raises(KeyError):
        nx.constraint(G, nodes=[0, 99])
    with pytest.raises(TypeError, match='supported libraries'):
        constraint({'not': 'a graph'})
    assert cpu_backend.calls == []
    B = nx.path_graph(4)
    B[1][2]['weight'] = -1.0
    constraint(B)                                               # weight=None never reads the attribute
    assert len(cpu_backend.calls) == 1


def test_igraph_parallel_edges_are_refused(cpu_backend):
    from graphrole_amd import constraint
    from tests.test_igraph_adapter_cpu import _pair
    ig, H = _pair(6, [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4)], False)
    _series_close(constraint(ig), nx.constraint(H), 'constraint', H)
    calls = len(cpu_backend.calls)
    ig, _ = _pair(6, [(0, 1), (0, 1), (1, 2)], False)
    with pytest.raises(NotImplementedError, match='multigraph'):
        constraint(ig)
    assert len(cpu_backend.calls) == calls


def test_catalogue_and_opt_in():
    from graphrole_amd import measures
    names = list(measures.CATALOGUE)
    assert names[names.index('effective_size') + 1] == 'constraint'
    assert names[-1] == 'eccentricity'
    assert measures.CATALOGUE['constraint'] == 'nx.constraint(G, weight=weight)'
    assert 'constraint' in measures.OPT_IN
    assert measures.available_measures(False, False) == ['degree', 'weighted_degree', 'clustering', 'effective_size',
                                                         'pagerank', 'eigenvector']
    assert measures.available_measures(True, False) == ['degree', 'weighted_degree', 'in_degree', 'out_degree',
                                                        'pagerank', 'eigenvector']
    assert measures.available_measures(False, True) == ['degree', 'weighted_degree', 'pagerank']
    assert measures.available_measures(True, True) == ['degree', 'weighted_degree', 'in_degree', 'out_degree',
                                                       'pagerank']
    assert measures._unavailable('constraint', False, False) is None
    assert measures._unavailable('constraint', True, False) is None
    assert 'multigraph' in measures._unavailable('constraint', False, True)
    assert 'multigraph' in measures._unavailable('constraint', True, True)
    import graphrole_amd
    assert graphrole_amd.constraint is measures.constraint and graphrole_amd.effective_size is measures.effective_size


# ---------------------------------------------------------------------------------------------------------- ABI
_C_TYPES = {'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'size_t': ctypes.c_size_t}


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
    for name, restype in (('grx_structural_holes', ctypes.c_int),
                          ('grx_structural_holes_workspace_bytes', ctypes.c_size_t)):
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[name] == (restype, _declared_arguments(header, name))
    assert len(_lib._SIGNATURES['grx_structural_holes'][1]) == 14
    assert 'SYMMETRIC in structure' in header and 'd_out_row_ptr' in header
    assert int(re.search(r'#define\s+GRX_VERSION\s+(\d+)', header).group(1)) == 1100
    assert callable(kernels.structural_holes)
    source = open(os.path.join(ROOT, 'graphrole_amd', 'csrc', 'grx_structural_holes.hip')).read()
    shared = open(os.path.join(ROOT, 'graphrole_amd', 'csrc', 'grx_rowjoin.h')).read()
    assert '#include "grx_rowjoin.h"' in source and 'fp contract(off)' in shared.split('#pragma once')[0]
    for constant in ('RJ_BLOCK', 'RJ_ROW_MAX_WG', 'RJ_ARC_MAX_WG'):     # the copies the GPU test sizes its graphs by
        assert int(re.search(r'constexpr int ' + constant + r' = (\d+);', shared).group(1)) == getattr(kernels, constant)
    assert '#pragma clang fp contract(off)' in source
    makefile = open(os.path.join(ROOT, 'graphrole_amd', 'csrc', 'Makefile')).read()
    assert 'grx_rowjoin.h' in re.search(r'%\.o: %\.hip (.*)', makefile).group(1)      # a dependency of every object
    assert 'grx_structural_holes.hip' in makefile and 'grx_structural_holes.o: FILEFLAGS := -ffp-contract=off' in makefile


def test_argument_validation_needs_no_device():
    """GRX_REQUIRE runs before any HIP call: n range, all outputs NULL, null pointers, lanes, hub list, a workspace
    below what the row arrays alone need.  n = 0 is an empty result."""
    from graphrole_amd import _lib
    lib = _lib.load()
    size = lib.grx_structural_holes_workspace_bytes
    assert size(10, 0) >= 16 * 10                               # S and X
    assert 16 * 10 + 20 * 1000 <= size(10, 1000) <= 16 * 10 + 20 * 1000 + 5 * 256      # + two terms and the row per arc
    assert size(0, 0) > 0 and size(10, 1001) >= size(10, 1000)
    need = size(10, 0)
    p = ctypes.c_void_p(4096)                                   # never dereferenced: every call fails validation

    def call(n=10, row_ptr=p, col=p, z=None, hubs=None, n_hubs=0, lanes=8, out_row_ptr=None, con=p, es=None, loc=None,
             ws=p, ws_bytes=need):
        return lib.grx_structural_holes(n, row_ptr, col, z, hubs, n_hubs, lanes, out_row_ptr, con, es, loc, ws,
                                        ws_bytes, None)

    for bad in (dict(n=-1), dict(n=1 << 31), dict(con=None), dict(row_ptr=None), dict(col=None), dict(ws=None),
                dict(lanes=0), dict(lanes=12), dict(lanes=64), dict(n_hubs=3), dict(n_hubs=-1), dict(n_hubs=11, hubs=p),
                dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert call(**bad) == -1, bad
        assert b'grx_structural_holes' in lib.grx_last_error()
    assert call(con=None) == -1 and b'all NULL' in lib.grx_last_error()
    assert call(n=0, row_ptr=None, col=None, ws=None, ws_bytes=0) == 0
    assert call(n=0, con=None) == -1                            # an output is required even then
