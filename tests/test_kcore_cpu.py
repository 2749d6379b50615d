"""
-m "not gpu": core number and onion layers without a device.  tests/kcore_oracle.py (the numpy restatement of the
synchronous peeling of csrc/grx_kcore.hip) against nx.core_number and nx.onion_layers, exactly, on a few thousand
seeded small graphs, directed ones with reciprocal arcs and every graph on five nodes included; then the Python layer
of graphrole_amd.core_number / onion_layers / node_measures over a CPU double of kernels.core_numbers (the oracle on
the double's CSR arrays); the ctypes signatures and the header's version.  The device numbers are pinned in
tests/test_gpu_kcore.py.
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
from tests import kcore_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_against_networkx(G):
    nodes, row_ptr, col, in_row_ptr, in_col = ko.graph_csrs(G)
    r = ko.core_numbers(row_ptr, col, in_row_ptr, in_col)
    assert r.core.dtype == np.int64 and r.onion.dtype == np.int64
    assert {v: int(r.core[i]) for i, v in enumerate(nodes)} == nx.core_number(G)
    if not G.is_directed():
        assert {v: int(r.onion[i]) for i, v in enumerate(nodes)} == nx.onion_layers(G)
    assert r.n_rounds == (int(r.onion.max()) if len(nodes) else 0)
    return r


def _clique_with_tail(k, tail):
    G = nx.complete_graph(k)
    nx.add_path(G, [0] + list(range(k, k + tail)))
    return G


def _families(seed):
    """The families of tests/test_biconnected_cpu.py without the self-loop one, plus a directed G(n, m) dense enough
    for reciprocal arcs and a clique with a tail."""
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
    yield nx.gnm_random_graph(n, rng.randint(n, min(3 * n, n * (n - 1) - 1)), seed=seed + 5, directed=True)
    yield _clique_with_tail(rng.randint(3, 7), rng.randint(1, 9))


@pytest.mark.parametrize('block', range(10))
def test_oracle_equals_networkx_on_seeded_graphs(block):
    checked = reciprocal = 0
    for seed in range(block * 25, block * 25 + 25):
        for G in _families(7919 * seed):
            _check_against_networkx(G)
            checked += 1
            if G.is_directed():
                reciprocal += any(G.has_edge(v, u) for u, v in G.edges())
    assert checked == 25 * 13
    assert reciprocal >= 10                                     # the directed family does hold reciprocal pairs


def test_oracle_every_graph_on_five_nodes():
    pairs = list(itertools.combinations(range(5), 2))
    for mask in range(1 << len(pairs)):
        G = nx.empty_graph(5)
        G.add_edges_from(p for k, p in enumerate(pairs) if mask >> k & 1)
        _check_against_networkx(G)


def test_oracle_degenerate_graphs():
    for G in (nx.empty_graph(1), nx.empty_graph(2), nx.empty_graph(5), nx.path_graph(2), nx.path_graph(3),
              nx.complete_graph(7), nx.path_graph(40), nx.empty_graph(3, create_using=nx.DiGraph),
              nx.DiGraph([(0, 1), (1, 0)]), nx.DiGraph([(0, 1), (1, 0), (1, 2)])):
        _check_against_networkx(G)
    r = _check_against_networkx(nx.empty_graph(5))
    assert r.core.tolist() == [0] * 5 and r.onion.tolist() == [1] * 5 and r.n_rounds == 1
    r = _check_against_networkx(_clique_with_tail(8, 30))
    assert sorted(set(r.core.tolist())) == [1, 7]               # the core jumps 1 -> 7 after the tail
    assert r.n_rounds == 31
    r = _check_against_networkx(nx.path_graph(2))
    assert r.core.tolist() == [1, 1] and r.onion.tolist() == [1, 1]


# ------------------------------------------------------------------------------------------ Python layer, CPU double
@pytest.fixture
def cpu_backend():
    import torch
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.calls = []

    def core_numbers(csr_out, csr_in=None, want_onion=True):
        double.calls.append((csr_out, csr_in, want_onion))
        r = ko.core_numbers(csr_out.row_ptr, csr_out.col, *(() if csr_in is None else (csr_in.row_ptr, csr_in.col)))
        return torch.from_numpy(r.core), torch.from_numpy(r.onion) if want_onion else None, r.n_rounds

    double.core_numbers = core_numbers
    backend.use(double)
    yield double
    backend.use(None)


def _disconnected():
    G = nx.disjoint_union(nx.barabasi_albert_graph(60, 2, seed=1), nx.cycle_graph(9))
    G.add_nodes_from([1000, 1001])
    return G


GRAPHS = {
    'karate': nx.karate_club_graph,
    'er': lambda: nx.gnm_random_graph(120, 400, seed=3),
    'disconnected': _disconnected,
    'strings': lambda: nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
    'grid': lambda: nx.grid_2d_graph(4, 5),
    'empty5': lambda: nx.empty_graph(5),
    'n1': lambda: nx.empty_graph(1),
    'directed': lambda: nx.gnm_random_graph(40, 300, seed=4, directed=True),
}


@pytest.mark.parametrize('key', list(GRAPHS))
def test_public_functions(cpu_backend, key):
    from graphrole_amd import core_number, onion_layers
    G = GRAPHS[key]()
    core = core_number(G)
    assert isinstance(core, pd.Series) and core.name == 'core_number' and core.dtype == np.int64
    assert list(core.index) == sorted(G)
    assert core.to_dict() == nx.core_number(G)
    assert len(cpu_backend.calls) == 1
    s_out, s_in, want_onion = cpu_backend.calls[0]
    assert not want_onion and (s_in is not None) == G.is_directed()
    if G.is_directed():
        return
    onion = onion_layers(G)
    assert isinstance(onion, pd.Series) and onion.name == 'onion_layer' and onion.dtype == np.int64
    assert list(onion.index) == sorted(G)
    assert onion.to_dict() == nx.onion_layers(G)
    # the kernel got the structure CSR of the adapter
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    want = NetworkxInterface(G)._structure_csrs()[0]
    for csr, _, _ in cpu_backend.calls:
        assert np.array_equal(csr.row_ptr, want.row_ptr) and np.array_equal(csr.col, want.col)


def test_catalogue_opt_in_and_one_call_for_both_columns(cpu_backend):
    from graphrole_amd import measures, node_measures
    assert measures.available_measures(False, False) == ['degree', 'weighted_degree', 'clustering', 'effective_size',
                                                         'pagerank', 'eigenvector']
    assert measures.available_measures(True, False) == ['degree', 'weighted_degree', 'in_degree', 'out_degree',
                                                        'pagerank', 'eigenvector']
    assert measures.available_measures(True, True) == ['degree', 'weighted_degree', 'in_degree', 'out_degree',
                                                       'pagerank']
    assert measures.CATALOGUE['core_number'] == 'nx.core_number(G)'
    assert measures.CATALOGUE['onion_layer'] == 'nx.onion_layers(G)'
    assert 'core_number' in measures.OPT_IN and 'onion_layer' in measures.OPT_IN
    G = nx.karate_club_graph()
    M = node_measures(G, ['weighted_degree', 'core_number', 'onion_layer', 'core_number'])
    assert len(cpu_backend.calls) == 1                          # one kernel call, cached inside one node_measures
    assert cpu_backend.calls[0][2] is True
    assert list(M.columns) == ['weighted_degree', 'core_number', 'onion_layer', 'core_number']
    M = node_measures(G, ['onion_layer', 'core_number'])
    assert M['core_number'].dtype == np.int64 and M['onion_layer'].dtype == np.int64
    assert list(M.index) == sorted(G)
    assert M['core_number'].to_dict() == nx.core_number(G)
    assert M['onion_layer'].to_dict() == nx.onion_layers(G)
    assert list(node_measures(G, ['weighted_degree']).columns) == ['weighted_degree']
    assert len(cpu_backend.calls) == 2


def test_every_refusal_makes_no_kernel_call(cpu_backend):
    from graphrole_amd import core_number, node_measures, onion_layers
    from graphrole_amd.graph.csr import CSRGraph
    L = nx.karate_club_graph()
    L.add_edge(3, 3)
    DL = nx.gnm_random_graph(20, 60, seed=1, directed=True)
    DL.add_edge(5, 5)
    for call in (lambda: core_number(L), lambda: onion_layers(L), lambda: core_number(DL),
                 lambda: node_measures(L, ['degree', 'core_number']),
                 lambda: core_number(CSRGraph(4, np.array([0, 1, 2]), np.array([1, 2, 2])))):
        with pytest.raises(NotImplementedError, match=r'G\.remove_edges_from\(nx\.selfloop_edges\(G\)\)'):
            call()
    for M in (nx.MultiGraph([(0, 1), (0, 1), (1, 2)]), nx.MultiDiGraph([(0, 1), (1, 2)])):
        for call in (lambda: core_number(M), lambda: onion_layers(M),
                     lambda: node_measures(M, ['core_number', 'onion_layer'])):
            with pytest.raises(NotImplementedError, match='multigraph'):
                call()
    D = nx.gnm_random_graph(30, 90, seed=2, directed=True)
    for call in (lambda: onion_layers(D), lambda: node_measures(D, ['core_number', 'onion_layer'])):
        with pytest.raises(NotImplementedError, match='directed'):
            call()
    for fn in (core_number, onion_layers):
        with pytest.raises(TypeError, match='supported libraries'):
            fn({'not': 'a graph'})
    assert cpu_backend.calls == []


def test_csr_and_igraph_inputs(cpu_backend):
    from graphrole_amd import core_number, onion_layers
    from graphrole_amd.graph.csr import CSRGraph
    from tests.test_igraph_adapter_cpu import _pair, _random_multigraph
    G = nx.barabasi_albert_graph(60, 2, seed=8)
    src, dst = np.array(list(G.edges)).T
    g = CSRGraph(60, src, dst)
    assert core_number(g).to_numpy().tobytes() == core_number(G).to_numpy().tobytes()
    assert onion_layers(g).to_dict() == nx.onion_layers(G)
    edges = sorted({(min(e), max(e)) for e in _random_multigraph(np.random.default_rng(3), 70, 90, False, False,
                                                                 False)})                   # a simple igraph graph
    ig, H = _pair(70, edges, False)
    assert core_number(ig).to_dict() == nx.core_number(nx.Graph(H))
    assert onion_layers(ig).to_dict() == nx.onion_layers(nx.Graph(H))
    calls = len(cpu_backend.calls)
    ig, _ = _pair(70, edges + [edges[0], edges[7][::-1]], False)                             # parallel edges
    with pytest.raises(NotImplementedError, match='multigraph'):
        core_number(ig)
    ig, _ = _pair(70, edges + [(5, 5)], False)                                               # a self-loop
    with pytest.raises(NotImplementedError, match='selfloop_edges'):
        onion_layers(ig)
    assert len(cpu_backend.calls) == calls


def test_ctypes_signatures_present():
    from graphrole_amd import _lib
    assert len(_lib._SIGNATURES['grx_core_numbers'][1]) == 17
    assert len(_lib._SIGNATURES['grx_core_numbers_workspace_bytes'][1]) == 1
    assert {'grx_core_numbers', 'grx_core_numbers_workspace_bytes'} <= set(_lib.EXPORTED_SYMBOLS)


def test_header_version_and_declarations():
    header = open(os.path.join(ROOT, 'include', 'grx.h')).read()
    assert int(re.search(r'#define\s+GRX_VERSION\s+(\d+)', header).group(1)) == 1100
    assert 'grx_core_numbers(' in header and 'grx_core_numbers_workspace_bytes(' in header


def test_argument_validation_needs_no_device():
    """GRX_REQUIRE runs before any HIP call: n range, null pointers, hub list, the in CSR given in part, workspace."""
    import ctypes
    from graphrole_amd import _lib
    lib = _lib.load()
    need = lib.grx_core_numbers_workspace_bytes(10)
    assert need >= 16 * 10
    p = ctypes.c_void_p(4096)                                   # never dereferenced: every call fails validation

    def call(n=10, row_ptr=p, col=p, hubs=None, n_hubs=0, lanes=8, in_row_ptr=None, in_col=None, in_hubs=None,
             n_in_hubs=0, in_lanes=0, core=p, ws=p, ws_bytes=need):
        return lib.grx_core_numbers(n, row_ptr, col, hubs, n_hubs, lanes, in_row_ptr, in_col, in_hubs, n_in_hubs,
                                    in_lanes, core, None, None, ws, ws_bytes, None)

    for bad in (dict(n=0), dict(n=1 << 31), dict(row_ptr=None), dict(col=None), dict(core=None), dict(ws=None),
                dict(lanes=0), dict(n_hubs=3), dict(n_hubs=-1), dict(in_lanes=8), dict(in_col=p),
                dict(in_row_ptr=p, in_lanes=8), dict(in_row_ptr=p, in_col=p, in_lanes=0),
                dict(in_row_ptr=p, in_col=p, in_lanes=8, n_in_hubs=2), dict(ws_bytes=need - 1)):
        assert call(**bad) != 0, bad
