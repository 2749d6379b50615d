"""
-m "not gpu": eccentricity, diameter, radius, center and periphery without a device.  tests/eccentricity_oracle.py
(the numpy restatement of grx_eccentricity and of the bounds driver) against nx.eccentricity, exactly, by both methods;
the invariants of the bounds after every round; then the Python layer of graphrole_amd.eccentricity / diameter /
radius / center / periphery / node_measures over a CPU double of kernels.eccentricity_pass (the oracle on the double's
CSR arrays); the ctypes signatures, the header and the argument validation of the library.  The device numbers are
pinned in tests/test_gpu_eccentricity.py.
"""
import ctypes
import os
import types

import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import eccentricity_oracle as eo
from tests import fake_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _largest_component(G):
    return G.subgraph(max(nx.connected_components(G), key=len)).copy()


def _strong_digraph(n=40, extra=60, seed=5):
    """A directed cycle through every node plus random arcs: strongly connected, distances not symmetric."""
    G = nx.gnm_random_graph(n, extra, seed=seed, directed=True)
    nx.add_cycle(G, range(n))
    return G


def _connected_graphs():
    yield 'karate', nx.karate_club_graph()
    for k in range(1, 41):
        yield f'P{k}', nx.path_graph(k)
    for k in range(3, 13):
        yield f'C{k}', nx.cycle_graph(k)
    yield 'star', nx.star_graph(30)
    yield 'grid12', nx.convert_node_labels_to_integers(nx.grid_2d_graph(12, 12))
    for seed in range(4):
        yield f'tree{seed}', nx.random_labeled_tree(50 + 7 * seed, seed=seed)
    yield 'gnp', _largest_component(nx.gnp_random_graph(60, 0.1, seed=2))
    yield 'digraph', _strong_digraph()


GRAPHS = dict(_connected_graphs())


@pytest.mark.parametrize('key', list(GRAPHS))
def test_oracle_equals_networkx_by_both_methods(key):
    G = GRAPHS[key]
    nodes = list(G)
    row_ptr, col = eo.pull_csr(G, nodes)
    want = nx.eccentricity(G)
    ecc, _, used = eo.eccentricity(row_ptr, col, 'all', directed=G.is_directed())
    assert ecc.dtype == np.int64 and used == len(nodes)
    assert dict(zip(nodes, ecc.tolist())) == want
    if G.is_directed():
        return
    for batch in (2, 8, 64):
        ecc, rounds, used = eo.eccentricity(row_ptr, col, 'bounds', batch=batch)
        assert dict(zip(nodes, ecc.tolist())) == want, batch
        assert used <= len(nodes) and rounds <= -(-len(nodes) // batch)


def test_oracle_reproduces_both_networkx_errors():
    G = nx.disjoint_union(nx.path_graph(5), nx.cycle_graph(4))
    for method in ('all', 'bounds'):
        with pytest.raises(nx.NetworkXError) as mine:
            eo.eccentricity(*eo.pull_csr(G, list(G)), method)
        with pytest.raises(nx.NetworkXError) as theirs:
            nx.eccentricity(G)
        assert str(mine.value) == str(theirs.value) and 'graph is not connected' in str(mine.value)
    D = nx.DiGraph([(0, 1), (1, 2), (2, 0), (2, 3)])            # 3 reaches nothing
    with pytest.raises(nx.NetworkXError) as mine:
        eo.eccentricity(*eo.pull_csr(D, list(D)), 'all', directed=True)
    with pytest.raises(nx.NetworkXError) as theirs:
        nx.eccentricity(D)
    assert str(mine.value) == str(theirs.value) and 'not strongly connected' in str(mine.value)


@pytest.mark.parametrize('key', ['karate', 'P40', 'C12', 'C11', 'star', 'grid12', 'tree0', 'tree3', 'gnp'])
@pytest.mark.parametrize('batch', [2, 6, 64])
def test_bounds_hold_and_close_after_every_round(key, batch):
    G = GRAPHS[key]
    nodes = list(G)
    ecc = np.array([nx.eccentricity(G)[v] for v in nodes])
    row_ptr, col = eo.pull_csr(G, nodes)
    unresolved = len(nodes)
    for sources, lower, upper in eo.bounds_rounds(row_ptr, col, batch):
        assert lower.dtype == np.int32 and upper.dtype == np.int32
        assert np.all(lower <= ecc) and np.all(ecc <= upper)
        assert np.all(lower[sources] == ecc[sources]) and np.all(upper[sources] == ecc[sources])
        assert 0 < len(sources) <= batch and len(set(sources.tolist())) == len(sources)
        left = int(np.count_nonzero(lower < upper))
        assert left < unresolved                                # strictly fewer every round
        unresolved = left
    assert unresolved == 0


def test_oracle_pass_semantics():
    # P5 pulled from row 0: distances 0..4; a repeated source counts again in reach; an id outside [0, n) does nothing
    row_ptr, col = eo.pull_csr(nx.path_graph(5), list(range(5)))
    ecc, reach, lower, upper = eo.eccentricity_pass(row_ptr, col, [0, 0, 7, -1])
    assert ecc.tolist() == [4, 4, 0, 0] and ecc.dtype == np.int32
    assert reach.tolist() == [0, 2, 2, 2, 2] and reach.dtype == np.int64
    assert lower.tolist() == [0, 1, 2, 3, 4] and upper is None  # the per-target maximum only
    ecc, reach, lower, upper = eo.eccentricity_pass(row_ptr, col, [0], want_upper=True)
    assert upper.tolist() == [4, 5, 6, 7, 8]
    assert lower.tolist() == [4, 3, 2, 3, 4]                    # max(d, ecc - d)
    _, reach, lower, upper = eo.eccentricity_pass(row_ptr, col, [2], lower, upper)
    assert reach.tolist() == [1, 1, 0, 1, 1]                    # this call's sources alone
    assert upper.tolist() == [4, 3, 2, 3, 4] and lower.tolist() == [4, 3, 2, 3, 4]
    # the selection rule: first round every row ties and the degree decides, then the row
    deg = np.diff(row_ptr)
    assert eo.select_sources(np.zeros(5), np.full(5, eo.INF), deg, 2).tolist() == [1, 2]
    assert eo.select_sources(np.array([4, 2, 2, 3, 4]), np.array([4, 5, 6, 6, 4]), deg, 2).tolist() == [1, 2]
    assert eo.select_sources(np.array([4, 2, 2, 3, 4]), np.array([4, 5, 6, 7, 4]), deg, 2).tolist() == [1, 3]


# ------------------------------------------------------------------------------------------ Python layer, CPU double
@pytest.fixture
def cpu_backend():
    import torch
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.calls = []

    def eccentricity_pass(csr_pull, sources, words=0, bounds=None, want_upper=False):
        sources = np.asarray(sources, dtype=np.int64)
        double.calls.append(dict(sources=sources.copy(), csr=csr_pull, words=words, accumulate=bounds is not None,
                                 upper=want_upper or (bounds is not None and bounds[1] is not None)))
        lower, upper = (None, None) if bounds is None else (bounds[0].numpy(), None if bounds[1] is None
                                                            else bounds[1].numpy())
        ecc, reach, lower, upper = eo.eccentricity_pass(csr_pull.row_ptr, csr_pull.col.astype(np.int64), sources,
                                                        lower, upper, want_upper)
        return (torch.from_numpy(ecc), torch.from_numpy(reach), torch.from_numpy(lower),
                None if upper is None else torch.from_numpy(upper))

    double.eccentricity_pass = eccentricity_pass
    backend.use(double)
    yield double
    backend.use(None)


def _series_equals(series, want: dict):
    assert isinstance(series, pd.Series) and series.name == 'eccentricity' and series.dtype == np.int64
    assert list(series.index) == sorted(want)
    assert series.to_dict() == want


API_GRAPHS = {
    'karate': nx.karate_club_graph,
    'strings': lambda: nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
    'grid': lambda: nx.grid_2d_graph(5, 7),
    'cycle200': lambda: nx.cycle_graph(200),
    'tree': lambda: nx.random_labeled_tree(300, seed=3),
    'ba': lambda: nx.barabasi_albert_graph(400, 2, seed=4),
    'n1': lambda: nx.empty_graph(1),
    'n2': lambda: nx.path_graph(2),
    'digraph': _strong_digraph,
}


@pytest.mark.parametrize('key', list(API_GRAPHS))
@pytest.mark.parametrize('method', ['bounds', 'all'])
def test_eccentricity_of_every_node(cpu_backend, key, method):
    from graphrole_amd import eccentricity
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    G = API_GRAPHS[key]()
    n = G.number_of_nodes()
    _series_equals(eccentricity(G, method=method, words=1), nx.eccentricity(G))
    s_out, s_in = NetworkxInterface(G)._structure_csrs()
    pulled = s_in if G.is_directed() else s_out                 # walking out-arcs = pulling over the in-adjacency
    for call in cpu_backend.calls:
        assert np.array_equal(call['csr'].row_ptr, pulled.row_ptr) and np.array_equal(call['csr'].col, pulled.col)
        assert call['words'] == 1
    if method == 'all' or G.is_directed():
        (call,) = cpu_backend.calls                             # one call, every node a source, pass A only
        assert call['sources'].tolist() == list(range(n)) and not call['upper'] and not call['accumulate']
    else:
        assert [c['accumulate'] for c in cpu_backend.calls] == [False] + [True] * (len(cpu_backend.calls) - 1)
        assert all(c['upper'] for c in cpu_backend.calls)
        used = np.concatenate([c['sources'] for c in cpu_backend.calls])
        assert len(set(used.tolist())) == len(used) <= n        # no row is a source twice
        assert len(cpu_backend.calls) <= -(-n // 64) and all(len(c['sources']) <= 64 for c in cpu_backend.calls)


def test_bounds_method_prunes_and_cycle_does_not(cpu_backend):
    from graphrole_amd import eccentricity
    got = eccentricity(API_GRAPHS['ba'](), method='bounds', words=1)
    assert got.attrs == {'method': 'bounds', 'rounds': len(cpu_backend.calls),
                         'sources': sum(len(c['sources']) for c in cpu_backend.calls)}
    assert got.attrs['sources'] < 400                           # pruned: not every node was a source
    assert cpu_backend.calls[0]['sources'].tolist() == list(range(64))     # first round: the 64 highest degrees
    cpu_backend.calls.clear()
    got = eccentricity(nx.cycle_graph(200), method='bounds', words=1)      # vertex-transitive: never prunes
    assert got.attrs == {'method': 'bounds', 'rounds': 4, 'sources': 200}
    assert [len(c['sources']) for c in cpu_backend.calls] == [64, 64, 64, 8]
    assert eccentricity(nx.cycle_graph(200)).attrs == {'method': 'all', 'rounds': 1, 'sources': 200}    # the default


def test_default_width_of_the_bounds_rounds(cpu_backend):
    from graphrole_amd import eccentricity, measures
    G = nx.random_labeled_tree(1500, seed=1)
    _series_equals(eccentricity(G, method='bounds'), nx.eccentricity(G))
    assert len(cpu_backend.calls[0]['sources']) == 64 * measures._ECC_BOUNDS_WORDS == 1024
    assert cpu_backend.calls[0]['words'] == 0                   # the library picks the narrowest width that holds them


def test_node_nbunch_and_non_members(cpu_backend):
    from graphrole_amd import eccentricity
    from tests.test_closeness_cpu import _internal_ids
    G = API_GRAPHS['strings']()
    want = nx.eccentricity(G)
    got = eccentricity(G, v='node-07')
    assert type(got) is int and got == want['node-07'] == nx.eccentricity(G, v='node-07')
    (call,) = cpu_backend.calls
    assert call['sources'].tolist() == _internal_ids(G, ['node-07']).tolist() and not call['upper']
    bunch = ['node-30', 'node-02', 'nobody', 'node-02', 'node-11']
    members = ['node-02', 'node-11', 'node-30']
    _series_equals(eccentricity(G, v=bunch), nx.eccentricity(G, v=bunch))
    assert cpu_backend.calls[-1]['sources'].tolist() == _internal_ids(G, members).tolist()
    assert not cpu_backend.calls[-1]['upper']                   # an nbunch takes 'all' whatever the method
    calls = len(cpu_backend.calls)
    empty = eccentricity(G, v=['nobody'])
    assert isinstance(empty, pd.Series) and len(empty) == 0 and empty.dtype == np.int64 and empty.name == 'eccentricity'
    assert nx.eccentricity(G, v=['nobody']) == {}
    K = nx.karate_club_graph()
    for bad in (99, 3.5):
        with pytest.raises(nx.NetworkXError):
            nx.eccentricity(K, v=bad)
        with pytest.raises(nx.NetworkXError):
            eccentricity(K, v=bad)
    assert len(cpu_backend.calls) == calls
    D = _strong_digraph()
    assert eccentricity(D, v=7) == nx.eccentricity(D, v=7)
    _series_equals(eccentricity(D, v=[1, 2, 3]), nx.eccentricity(D, v=[1, 2, 3]))


def test_diameter_radius_center_periphery(cpu_backend):
    from graphrole_amd import center, diameter, eccentricity, periphery, radius
    for key in ('karate', 'strings', 'grid', 'tree', 'n1', 'digraph'):
        G = API_GRAPHS[key]()
        assert (diameter(G), radius(G)) == (nx.diameter(G), nx.radius(G))
        assert type(diameter(G)) is int and type(radius(G)) is int
        assert center(G) == sorted(nx.center(G)) and periphery(G) == sorted(nx.periphery(G))    # index order
        assert diameter(G, usebounds=True) == nx.diameter(G, usebounds=True)
    G = API_GRAPHS['grid']()
    e = eccentricity(G)
    calls = len(cpu_backend.calls)
    assert (diameter(G, e=e), radius(G, e=e), center(G, e), periphery(G, e)) == \
        (nx.diameter(G), nx.radius(G), sorted(nx.center(G)), sorted(nx.periphery(G)))
    ne = nx.eccentricity(G)                                     # networkx's dict serves too, in its own order
    assert (diameter(G, e=ne), radius(G, e=ne), center(G, ne), periphery(G, ne)) == \
        (nx.diameter(G, e=ne), nx.radius(G, e=ne), nx.center(G, e=ne), nx.periphery(G, e=ne))
    assert len(cpu_backend.calls) == calls                      # a precomputed e: no kernel call


def test_empty_graph_as_networkx(cpu_backend):
    from graphrole_amd import center, diameter, eccentricity, periphery, radius
    G = nx.empty_graph(0)
    assert nx.eccentricity(G) == {}
    got = eccentricity(G)
    assert isinstance(got, pd.Series) and len(got) == 0 and got.dtype == np.int64 and got.name == 'eccentricity'
    for mine, theirs in ((diameter, nx.diameter), (radius, nx.radius), (center, nx.center),
                         (periphery, nx.periphery)):
        with pytest.raises(ValueError):
            theirs(G)
        with pytest.raises(ValueError):
            mine(G)
    assert cpu_backend.calls == []


def test_not_connected_raises_networkx_errors(cpu_backend):
    from graphrole_amd import diameter, eccentricity, node_measures
    G = nx.disjoint_union(nx.barabasi_albert_graph(100, 2, seed=1), nx.cycle_graph(9))
    with pytest.raises(nx.NetworkXError) as theirs:
        nx.eccentricity(G)
    for call in (lambda: eccentricity(G, method='bounds', words=1), lambda: eccentricity(G), lambda: diameter(G),
                 lambda: eccentricity(G, v=3), lambda: node_measures(G, ['weighted_degree', 'eccentricity'])):
        with pytest.raises(nx.NetworkXError) as mine:
            call()
        assert str(mine.value) == str(theirs.value)
    cpu_backend.calls.clear()
    with pytest.raises(nx.NetworkXError):
        eccentricity(G, method='bounds', words=1)
    assert len(cpu_backend.calls) == 1                          # found after the first round
    D = nx.DiGraph([(0, 1), (1, 2), (2, 0), (2, 3)])
    with pytest.raises(nx.NetworkXError) as theirs:
        nx.eccentricity(D)
    for call in (lambda: eccentricity(D), lambda: eccentricity(D, v=3), lambda: node_measures(D, ['eccentricity'])):
        with pytest.raises(nx.NetworkXError) as mine:
            call()
        assert str(mine.value) == str(theirs.value)
    # a source that does reach every node has its eccentricity although the digraph is not strongly connected
    assert eccentricity(nx.DiGraph([(3, 0), (0, 1), (1, 2), (2, 0)]), v=3) == \
        nx.eccentricity(nx.DiGraph([(3, 0), (0, 1), (1, 2), (2, 0)]), v=3) == 3


def test_node_measures_column_and_opt_in(cpu_backend):
    from graphrole_amd import measures, node_measures
    assert measures.available_measures(False, False) == ['degree', 'weighted_degree', 'clustering', 'effective_size',
                                                         'pagerank', 'eigenvector']
    assert measures.available_measures(True, False) == ['degree', 'weighted_degree', 'in_degree', 'out_degree',
                                                        'pagerank', 'eigenvector']
    assert list(measures.CATALOGUE)[-1] == 'eccentricity'
    assert measures.CATALOGUE['eccentricity'] == 'nx.eccentricity(G)'
    assert 'eccentricity' in measures.OPT_IN
    for directed, multi in ((False, False), (True, False), (False, True), (True, True)):
        assert measures._unavailable('eccentricity', directed, multi) is None
    G = nx.karate_club_graph()
    M = node_measures(G, ['weighted_degree', 'eccentricity', 'eccentricity'])
    assert list(M.columns) == ['weighted_degree', 'eccentricity', 'eccentricity']
    assert M['eccentricity'].iloc[:, 0].dtype == np.int64
    assert M['eccentricity'].iloc[:, 0].to_dict() == nx.eccentricity(G)
    (call,) = cpu_backend.calls                                 # method 'all', computed once for both columns
    assert not call['upper'] and call['sources'].tolist() == list(range(34))
    cpu_backend.calls.clear()
    D = _strong_digraph()
    M = node_measures(D, ['eccentricity'])
    assert M['eccentricity'].dtype == np.int64 and M['eccentricity'].to_dict() == nx.eccentricity(D)
    assert list(M.index) == sorted(D)
    (call,) = cpu_backend.calls
    assert not call['upper']                                    # a directed graph never gets the bounds


def test_refusals_make_no_kernel_call(cpu_backend, monkeypatch):
    from graphrole_amd import diameter, eccentricity, node_measures
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    G = nx.karate_club_graph()
    with pytest.raises(NotImplementedError, match=r"nx.eccentricity\(G, weight='weight'\)"):
        eccentricity(G, weight='weight')
    with pytest.raises(NotImplementedError, match='shortest-path search by weight'):
        eccentricity(G, v=3, weight='w')
    with pytest.raises(ValueError, match="'bounds' or 'all'"):
        eccentricity(G, method='exact')
    with pytest.raises(TypeError, match='supported libraries'):
        eccentricity({'not': 'a graph'})
    with pytest.raises(TypeError, match='supported libraries'):
        diameter([1, 2])
    D = _strong_digraph()
    monkeypatch.setattr(NetworkxInterface, '_structure_csrs', lambda self: (self._device_graph()[1], None))
    for call in (lambda: eccentricity(D), lambda: eccentricity(D, v=0), lambda: node_measures(D, ['eccentricity'])):
        with pytest.raises(NotImplementedError, match='in-adjacency'):
            call()
    assert cpu_backend.calls == []


def test_multigraph_edges_once_and_self_loops_ignored(cpu_backend):
    from graphrole_amd import eccentricity, periphery
    M = nx.MultiGraph([(0, 1), (0, 1), (1, 2), (2, 0), (2, 3), (3, 3), (3, 4), (4, 5), (5, 3), (5, 6), (5, 6)])
    _series_equals(eccentricity(M), nx.eccentricity(M))
    _series_equals(eccentricity(M, method='bounds'), nx.eccentricity(M))
    assert periphery(M) == sorted(nx.periphery(M))
    L = nx.karate_club_graph()
    L.add_edges_from([(3, 3), (33, 33)])
    _series_equals(eccentricity(L), nx.eccentricity(nx.karate_club_graph()))
    _series_equals(eccentricity(L, method='bounds'), nx.eccentricity(nx.karate_club_graph()))
    MD = nx.MultiDiGraph([(0, 1), (0, 1), (1, 2), (2, 0), (2, 3), (3, 1), (3, 3)])
    _series_equals(eccentricity(MD), nx.eccentricity(MD))


def test_csr_and_igraph_inputs(cpu_backend):
    from graphrole_amd import eccentricity
    from graphrole_amd.graph.csr import CSRGraph
    from tests.test_igraph_adapter_cpu import _pair
    G = nx.barabasi_albert_graph(60, 2, seed=8)
    src, dst = np.array(list(G.edges)).T
    assert eccentricity(CSRGraph(60, src, dst)).to_dict() == nx.eccentricity(G)
    edges = list(G.edges) + [(0, 1), (5, 5)]                    # parallel edge and self-loop
    ig, H = _pair(60, edges, False)
    assert eccentricity(ig).to_dict() == eccentricity(ig, method='bounds').to_dict() == nx.eccentricity(H)


# ---------------------------------------------------------------------------------------------------------- ABI
def test_ctypes_signatures_present():
    from graphrole_amd import _lib
    assert len(_lib._SIGNATURES['grx_eccentricity'][1]) == 17
    assert len(_lib._SIGNATURES['grx_eccentricity_workspace_bytes'][1]) == 3
    assert {'grx_eccentricity', 'grx_eccentricity_workspace_bytes'} <= set(_lib.EXPORTED_SYMBOLS)


def test_header_declarations():
    header = open(os.path.join(ROOT, 'include', 'grx.h')).read()
    assert 'grx_eccentricity(' in header and 'grx_eccentricity_workspace_bytes(' in header
    assert 'SYMMETRIC CSR' in header                            # the validity of the bounds pass is documented
    from graphrole_amd import kernels
    assert callable(kernels.eccentricity_pass)


def test_argument_validation_needs_no_device():
    """GRX_REQUIRE runs before any HIP call: n range, null pointers, source list, words, hub list, accumulate,
    workspace.  d_upper may be NULL (no second pass)."""
    from graphrole_amd import _lib
    lib = _lib.load()
    need = lib.grx_eccentricity_workspace_bytes(10, 1, 64)
    assert need >= 3 * 8 * 10 and lib.grx_eccentricity_workspace_bytes(10, 16, 64) >= 3 * 8 * 16 * 10
    assert lib.grx_eccentricity_workspace_bytes(10, 0, 64) == need          # 64 sources: one word
    assert lib.grx_eccentricity_workspace_bytes(10, 0, 65) == lib.grx_eccentricity_workspace_bytes(10, 2, 65)
    p = ctypes.c_void_p(4096)                                   # never dereferenced: every call fails validation

    def call(n=10, row_ptr=p, col=p, hubs=None, n_hubs=0, lanes=8, sources=p, n_sources=64, words=1, ecc=p, reach=p,
             lower=p, upper=None, accumulate=0, ws=p, ws_bytes=need):
        return lib.grx_eccentricity(n, row_ptr, col, hubs, n_hubs, lanes, sources, n_sources, words, ecc, reach,
                                    lower, upper, accumulate, ws, ws_bytes, None)

    for bad in (dict(n=0), dict(n=1 << 31), dict(row_ptr=None), dict(col=None), dict(reach=None), dict(lower=None),
                dict(ws=None), dict(sources=None), dict(ecc=None), dict(n_sources=-1), dict(n_sources=1 << 31),
                dict(words=3), dict(words=32), dict(lanes=0), dict(n_hubs=3), dict(n_hubs=-1), dict(accumulate=2),
                dict(accumulate=-1), dict(ws_bytes=need - 1)):
        assert call(**bad) == -1, bad
    assert b'grx_eccentricity' in lib.grx_last_error()
