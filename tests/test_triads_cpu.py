"""
-m "not gpu": the triad census without a device.  tests/triad_oracle.py holds two independent implementations:
``brute_census`` (every 3-subset classified by its arcs: the definition) and ``census`` (the numpy restatement of
csrc/grx_triads.hip on the kernel's own arrays).  Both are compared with ``nx.triadic_census`` of the whole graph and of
every single node, on seeded G(n, p) digraphs with an isolated node, on every digraph on three labelled nodes and on the
directed small-graph atlas; the 64-entry code table and the 7 x 6 matrix of the kernel source are re-derived from
``nx.triad_type`` on the triads themselves; the identities of the census; then the Python layer of
graphrole_amd.triadic_census / node_triad_census over a CPU double of kernels.triad_census (the oracle on the double's
CSR arrays), the refusals, the ctypes signatures against the header, the argument checks of grx_triad_census and the
unchanged catalogue.  The device numbers are pinned in tests/test_gpu_triads.py.
"""
import ctypes
import itertools
import math
import os
import re
import types

import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import atlas, fake_kernels
from tests import test_sense_cpu as sense
from tests import triad_oracle as to
from tests.test_graphlet_cpu import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'graphrole_amd', 'csrc', 'grx_triads.hip')
PS = (0.08, 0.2, 0.45, 0.8)


def seeded(n, p, seed):
    G = nx.gnp_random_graph(n, p, seed=seed, directed=True)
    G.add_node(n)                                               # isolated
    return G


def _check(G, per_node=True):
    """brute force == networkx == the formulas, for the graph and for every node."""
    nodes, c = to.graph_census(G)
    want = nx.triadic_census(G)
    assert to.brute_census(G) == want
    assert to.as_dict(c.totals) == want
    if per_node:
        for k, v in enumerate(nodes):
            at_v = nx.triadic_census(G, nodelist=[v])
            assert to.brute_census(G, v) == at_v
            assert to.as_dict(c.columns[:, k]) == at_v
    return nodes, c


# ------------------------------------------------------------------------------------------------ oracle authority
@pytest.mark.parametrize('p', PS)
def test_oracles_equal_networkx_on_seeded_digraphs(p):
    seen = np.zeros(16, dtype=np.int64)
    for seed, n in enumerate((5, 9, 14)):
        _, c = _check(seeded(n, p, 100 * seed + int(100 * p)))
        seen += c.totals
    assert seen.sum() > 0


def test_every_type_occurs_in_the_seeded_digraphs():
    seen = np.zeros(16, dtype=np.int64)
    for p in PS:
        seen += to.graph_census(seeded(14, p, 7))[1].totals
    assert np.all(seen > 0)


def test_oracles_on_every_digraph_on_three_nodes():
    names = set()
    for G in to.all_digraphs(3):
        _, c = _check(G)
        assert c.totals.sum() == 1
        names.add(to.NAMES[int(np.argmax(c.totals))])
    assert names == set(to.NAMES)


def test_oracles_on_the_directed_atlas():
    graphs = atlas.small_graphs('directed')
    assert len(graphs) > 1000
    seen = np.zeros(16, dtype=np.int64)
    for _, _, G in graphs:
        _, c = _check(G, per_node=len(G) <= 5)
        if len(G) > 5:                                          # per node against brute force alone: networkx is slow
            for k, v in enumerate(sorted(G)):
                assert to.as_dict(c.columns[:, k]) == to.brute_census(G, v)
        seen += c.totals
    assert np.all(seen[1:] > 0)


# ------------------------------------------------------------------------------------------------------ the tables
def _triad_of_code(code):
    """The triad (0, 1, 2) with the 6-bit code c(0, 1) | c(0, 2) << 2 | c(1, 2) << 4."""
    G = nx.DiGraph()
    G.add_nodes_from(range(3))
    for bit, arc in enumerate([(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)]):
        if code >> bit & 1:
            G.add_edge(*arc)
    return G


def _in_source(name, rows, cols):
    source = open(SOURCE).read()
    body = re.search(name + r'(?:\[\w+\])+\s*=\s*\{(.*?)\};', source, re.S).group(1)
    return np.array([int(x) for x in re.findall(r'\d+', body)], dtype=np.int64).reshape(rows, cols)


def test_code_table_is_what_networkx_calls_the_64_triads():
    derived = np.array([to.NAMES.index(nx.triad_type(_triad_of_code(code))) for code in range(64)])
    assert np.array_equal(derived, to.TYPE_OF_CODE)
    assert np.array_equal(_in_source('TD_TYPE', 1, 64)[0], derived)
    closed = [code for code in range(64) if code & 3 and code >> 2 & 3 and code >> 4 & 3]
    assert len(closed) == 27 and {to.NAMES[derived[code]] for code in closed} == set(to.CLOSED)


def test_matrix_is_what_dropping_a_pair_of_a_closed_triad_leaves():
    derived = {}
    for code in range(64):
        G = _triad_of_code(code)
        name = nx.triad_type(G)
        if name not in to.CLOSED:
            continue
        row = np.zeros(6, dtype=np.int64)
        for a, b in ((0, 1), (0, 2), (1, 2)):
            H = G.copy()
            H.remove_edges_from([(a, b), (b, a)])
            row[to.WEDGES.index(nx.triad_type(H))] += 1
        assert np.array_equal(derived.setdefault(name, row), row)       # a function of the closed type alone
    matrix = np.stack([derived[name] for name in to.CLOSED])
    assert np.array_equal(matrix, to.MATRIX) and np.all(matrix.sum(axis=1) == 3)
    assert np.array_equal(_in_source('TD_OPEN', 7, 6), matrix)
    assert _in_source('TD_WEDGE_COL', 1, 6)[0].tolist() == [to.T[name] for name in to.WEDGES]
    assert _in_source('TD_CLOSED_COL', 1, 7)[0].tolist() == [to.T[name] for name in to.CLOSED]
    # the wedge type of a class pair, from the wedge itself: centre 0 with the slot codes x and z
    for (x, z), name in to.WEDGE_OF.items():
        assert nx.triad_type(_triad_of_code(x | z << 2)) == name


# ------------------------------------------------------------------------------------------------------ identities
@pytest.mark.parametrize('p', PS)
def test_identities(p):
    G = seeded(13, p, 3)
    n = len(G)
    nodes, c = to.graph_census(G)
    assert np.array_equal(c.columns.sum(axis=1), 3 * c.totals)
    assert c.totals.sum() == math.comb(n, 3)
    assert np.all(c.columns.sum(axis=0) == math.comb(n - 1, 2))
    assert np.all(c.columns >= 0)
    rng = np.random.default_rng(5)
    for subset in (list(G), [nodes[3]], rng.permutation(n)[:5].tolist(), rng.permutation(n)[:9].tolist()):
        rest = G.subgraph(set(G) - set(subset))
        diff = c.totals - (to.graph_census(rest)[1].totals if len(rest) else 0)
        assert to.as_dict(diff) == nx.triadic_census(G, nodelist=subset)
    # common(u, v) is the number of common neighbours in either direction, at both slots
    _, row_ptr, col, _ = to.graph_arrays(G)
    U = G.to_undirected()
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    assert c.common.tolist() == [len(list(nx.common_neighbors(U, nodes[u], nodes[v]))) for u, v in zip(rows, col)]


@pytest.mark.parametrize('C', [3, 5])
def test_tiling_of_the_directed_motif(C):
    """What tests/test_gpu_triads_second_trip.py relies on, at a size the oracle takes in no time."""
    from tests import tiled_graphs as tg
    (m_ptr, m_col, m_codes), _, (n, row_ptr, col, codes, arc_src) = to.tiled_motif(C)
    n0 = len(m_ptr) - 1
    assert n == n0 * C and len(col) == len(m_col) * C
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    key = rows * n + col
    assert np.all(np.diff(key) > 0) and not np.any(rows == col)                # ascending, distinct, no diagonal
    assert np.array_equal(codes[np.searchsorted(key, col.astype(np.int64) * n + rows)],
                          np.array([0, 2, 1, 3], dtype=np.uint8)[codes])        # the mirror at the reverse slot
    motif, big = to.census(m_ptr, m_col, m_codes), to.census(row_ptr, col, codes)
    if C == 3:
        D = nx.DiGraph(tg.motif('directed').G)
        D.remove_edges_from(list(nx.selfloop_edges(D)))
        assert to.as_dict(motif.totals) == nx.triadic_census(D)
    local = [to.T[name] for name in to.WEDGES + to.CLOSED]
    absent = {name for name in to.WEDGES + to.CLOSED if not motif.totals[to.T[name]]}
    assert absent == {'030T', '030C'}                           # every other connected type occurs in the motif
    assert np.array_equal(big.columns[local], tg.tile_nodes(motif.columns[local], C))
    assert np.array_equal(big.common, motif.common[arc_src])
    assert np.array_equal(big.totals[local], C * motif.totals[local])
    assert big.totals.sum() == math.comb(n, 3) and np.all(big.columns.sum(axis=0) == math.comb(n - 1, 2))
    assert int(np.diff(m_ptr).max()) > 4 * 32                                   # a hub row at 4 lanes per row


# ------------------------------------------------------------------------------------------ Python layer, CPU double
@pytest.fixture
def cpu_backend():
    import torch
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.calls = []

    def triad_census(csr, codes, want_totals=True, want_arc_triads=False, lanes=None):
        double.calls.append((csr, codes, want_totals, want_arc_triads, lanes))
        r = to.census(csr.row_ptr, csr.col, codes.numpy())
        return (torch.from_numpy(r.columns), torch.from_numpy(r.totals) if want_totals else None,
                torch.from_numpy(r.common) if want_arc_triads else None)

    double.triad_census = triad_census
    double.row_counts = sense._row_counts
    double.sense_normal_equations = sense._sense_normal_equations
    double.nnls = sense._nnls
    backend.use(double)
    yield double
    backend.use(None)


def _reciprocal(n, p, seed):
    G = nx.gnp_random_graph(n, p, seed=seed, directed=True)
    G.add_nodes_from([n, n + 1])
    return G


GRAPHS = {
    'gnp': lambda: _reciprocal(25, 0.2, 4),
    'dense': lambda: _reciprocal(12, 0.7, 5),
    'strings': lambda: nx.relabel_nodes(_reciprocal(20, 0.25, 6), lambda v: f'node-{v:02d}'),
    'dag': lambda: nx.DiGraph([(u, v) for u, v in nx.gnp_random_graph(20, 0.3, seed=2).edges() if u < v]),
    'arc': lambda: nx.DiGraph([(0, 1)]),
}


@pytest.mark.parametrize('key', list(GRAPHS))
def test_public_functions(cpu_backend, key):
    from graphrole_amd import node_triad_census, triadic_census
    G = GRAPHS[key]()
    want = nx.triadic_census(G)
    census = triadic_census(G)
    assert census == want and list(census) == list(to.NAMES) and all(type(x) is int for x in census.values())
    frame = node_triad_census(G)
    assert isinstance(frame, pd.DataFrame) and list(frame.columns) == to.COLUMNS
    assert all(dt == np.int64 for dt in frame.dtypes)
    assert list(frame.index) == sorted(G)
    for v in G:
        assert dict(zip(to.NAMES, frame.loc[v].tolist())) == to.brute_census(G, v)
    assert frame.attrs['census'] == want and list(frame.attrs['census']) == list(to.NAMES)
    assert all(type(x) is int for x in frame.attrs['census'].values())
    assert frame.to_numpy().sum(axis=0).tolist() == [3 * want[name] for name in to.NAMES]
    assert len(cpu_backend.calls) == 2                          # one per function: the CSR is cached per adapter
    for csr, codes, want_totals, want_arc, lanes in cpu_backend.calls:
        assert want_totals and not want_arc and lanes is None
        assert str(codes.dtype) == 'torch.uint8'
        assert not np.any(csr.col == np.repeat(np.arange(csr.n), np.diff(csr.row_ptr)))      # no diagonal entry
        assert set(np.unique(codes.numpy()[:csr.nnz]).tolist()) <= {1, 2, 3}


def test_nodelist(cpu_backend):
    from graphrole_amd import triadic_census
    G = GRAPHS['strings']()
    rng = np.random.default_rng(3)
    nodes = sorted(G)
    for subset in (nodes, [nodes[4]], [nodes[k] for k in rng.permutation(len(nodes))[:6]], []):
        cpu_backend.calls.clear()
        assert triadic_census(G, nodelist=subset) == nx.triadic_census(G, nodelist=subset)
        assert len(cpu_backend.calls) == (0 if not subset else 2 if len(subset) < len(nodes) else 1)
    assert triadic_census(G, nodelist=iter([nodes[2], nodes[0]])) == nx.triadic_census(G, nodelist=[nodes[2], nodes[0]])


def test_nodes_argument(cpu_backend):
    from graphrole_amd import node_triad_census
    G = GRAPHS['strings']()
    full = node_triad_census(G)
    one = node_triad_census(G, 'node-05')
    assert isinstance(one, pd.Series) and list(one.index) == to.COLUMNS and one.dtype == np.int64
    assert one.tolist() == full.loc['node-05'].tolist()
    assert dict(zip(to.NAMES, one.tolist())) == nx.triadic_census(G, nodelist=['node-05'])
    some = node_triad_census(G, ['node-19', 'node-00', 'node-07'])
    assert isinstance(some, pd.DataFrame) and list(some.index) == ['node-00', 'node-07', 'node-19']
    assert some.equals(full.loc[['node-00', 'node-07', 'node-19']])
    assert one.attrs['census'] == some.attrs['census'] == full.attrs['census'] == nx.triadic_census(G)
    before = len(cpu_backend.calls)
    for bad in ('not-a-node', ['node-00', 'not-a-node']):
        with pytest.raises(KeyError):
            node_triad_census(G, bad)
    assert len(cpu_backend.calls) == before


def test_csr_input(cpu_backend):
    from graphrole_amd import node_triad_census, triadic_census
    from graphrole_amd.graph.csr import CSRGraph
    G = _reciprocal(40, 0.1, 8)
    src, dst = np.array(list(G.edges)).T
    C = CSRGraph(len(G), src, dst, directed=True)
    a, b = node_triad_census(C), node_triad_census(G)
    assert list(a.index) == list(b.index) and a.to_numpy().tobytes() == b.to_numpy().tobytes()
    assert triadic_census(C) == nx.triadic_census(G)


def test_columns_join_the_measure_table_for_sense_making(cpu_backend):
    from graphrole_amd import node_measures, node_triad_census
    G = GRAPHS['gnp']()
    M = node_measures(G, ['in_degree', 'out_degree'])
    M = M.join(node_triad_census(G))
    assert list(M.columns) == ['in_degree', 'out_degree'] + to.COLUMNS and not M.isna().any().any()
    n = len(G)
    assert (M[to.COLUMNS].sum(axis=1) == math.comb(n - 1, 2)).all()
    mutual = sum(1 for u, v in G.edges() if u < v and G.has_edge(v, u))
    asym = G.number_of_edges() - 2 * mutual                     # an isolated node sees every pair from outside
    assert M.loc[n - 1, to.COLUMNS].tolist() == [math.comb(n - 1, 2) - asym - mutual, asym, mutual] + [0] * 13
    from graphrole_amd import RoleExtractor
    ext = RoleExtractor(n_roles=3)
    ext.node_role_factor = pd.DataFrame(np.random.default_rng(0).random((n, 3)), index=M.index,
                                        columns=['role_0', 'role_1', 'role_2'])
    E = ext.sense_making(M)
    assert E.shape == (3, 18) and list(E.columns) == list(M.columns) and np.all(E.to_numpy() >= 0)
    assert np.all(np.isfinite(E.to_numpy())) and E[to.COLUMNS].to_numpy().sum() > 0


def test_empty_and_edgeless_graphs_make_no_kernel_call(cpu_backend, monkeypatch):
    from graphrole_amd import node_triad_census, triadic_census
    from graphrole_amd.graph.interface.networkx import NetworkxInterface

    def no_device(*args, **kwargs):
        raise AssertionError('device work for a graph without arcs')

    monkeypatch.setattr(NetworkxInterface, '_device_graph', no_device)
    for n in (0, 1, 2, 3, 6):
        G = nx.empty_graph(n, create_using=nx.DiGraph)
        want = nx.triadic_census(G)
        assert triadic_census(G) == want and want['003'] == math.comb(n, 3)
        frame = node_triad_census(G)
        assert list(frame.columns) == to.COLUMNS and all(dt == np.int64 for dt in frame.dtypes)
        assert list(frame.index) == list(G) and frame.attrs['census'] == want
        assert (frame['triad_003'] == math.comb(max(n - 1, 0), 2)).all()
        assert frame.to_numpy().sum() == 3 * math.comb(n, 3)
        if n >= 3:
            assert triadic_census(G, nodelist=[0, 2]) == nx.triadic_census(G, nodelist=[0, 2])
    assert cpu_backend.calls == []


def test_every_refusal_makes_no_device_call(cpu_backend, monkeypatch):
    from graphrole_amd import node_triad_census, triadic_census
    from graphrole_amd.graph.csr import CSRGraph
    from graphrole_amd.graph.interface.networkx import NetworkxInterface

    def no_device(*args, **kwargs):
        raise AssertionError('device work for a refused graph')

    monkeypatch.setattr(cpu_backend, 'triad_census', no_device)
    monkeypatch.setattr(NetworkxInterface, '_device_graph', no_device)
    monkeypatch.setattr(NetworkxInterface, '_structure_csrs', no_device)
    L = nx.gnm_random_graph(20, 60, seed=2, directed=True)
    L.add_edge(3, 3)
    for fn in (triadic_census, node_triad_census):
        with pytest.raises(NotImplementedError, match=r'undirected.*G\.to_directed\(\)'):
            fn(nx.karate_club_graph())
        for M in (nx.MultiDiGraph([(0, 1), (0, 1), (1, 2)]), nx.MultiDiGraph([(0, 1), (1, 2)])):
            with pytest.raises(NotImplementedError, match=r'multigraph.*nx\.DiGraph\(G\)'):
                fn(M)
        with pytest.raises(NotImplementedError, match=r'G\.remove_edges_from\(nx\.selfloop_edges\(G\)\)'):
            fn(L)
        with pytest.raises(TypeError, match='supported libraries'):
            fn({'not': 'a graph'})
    with pytest.raises(NotImplementedError, match='parallel arcs'):            # a CSRGraph cannot hold any
        triadic_census(nx.MultiDiGraph([(0, 1), (0, 1), (1, 0)]))
    with pytest.raises(NotImplementedError, match='undirected'):
        triadic_census(CSRGraph(4, np.array([0, 1, 2]), np.array([1, 2, 3])))
    with pytest.raises(NotImplementedError, match='selfloop_edges'):
        node_triad_census(CSRGraph(4, np.array([0, 1, 2]), np.array([1, 2, 2]), directed=True))
    D = nx.gnm_random_graph(20, 60, seed=2, directed=True)
    for bad in ([1, 1], [1, 99], [99], [[1]]):
        with pytest.raises(ValueError, match='duplicate nodes or nodes not in G'):
            triadic_census(D, nodelist=bad)
    assert cpu_backend.calls == []


# ----------------------------------------------------------------------------------------------------------- the ABI
def test_ctypes_signatures_match_the_header_and_the_catalogue_is_unchanged():
    import graphrole_amd
    from graphrole_amd import _lib, measures
    header = open(os.path.join(ROOT, 'include', 'grx.h')).read()
    for name, n_args in (('grx_triad_census', 13), ('grx_triad_census_workspace_bytes', 2)):
        restype, argtypes = _declared(header, name)
        assert len(argtypes) == n_args
        assert _lib._SIGNATURES[name] == (restype, argtypes)
        assert name in _lib.EXPORTED_SYMBOLS
    assert int(re.search(r'#define\s+GRX_VERSION\s+(\d+)', header).group(1)) == 1100      # added entry points only
    for name in ('triadic_census', 'node_triad_census'):
        assert getattr(graphrole_amd, name) is getattr(measures, name)
        assert name not in measures.CATALOGUE and name not in measures.OPT_IN
    assert tuple(measures.TRIAD_NAMES) == to.NAMES
    assert not any('triad' in name for name in list(measures.CATALOGUE) + list(measures.OPT_IN))
    for directed, multi in itertools.product((False, True), repeat=2):
        assert not any('triad' in name for name in measures.available_measures(directed, multi))
    assert len(measures.CATALOGUE) == 16 and len(measures.OPT_IN) == 8


def test_argument_validation_needs_no_device():
    """GRX_REQUIRE runs before any HIP call: n range, null pointers, lanes, hub list, a workspace too short for any
    graph; each failure is GRX_ERR_INVALID (-1) with the entry point's name in grx_last_error()."""
    from graphrole_amd import _lib
    lib = _lib.load()
    assert lib.grx_triad_census_workspace_bytes(10, 0) == 5 * 256 + 2 * 256
    assert lib.grx_triad_census_workspace_bytes(1000, 1000) == 5 * 8192 + 2 * 4096
    need = lib.grx_triad_census_workspace_bytes(10, 0)
    p = ctypes.c_void_p(4096)                                   # never dereferenced: every call fails validation

    def call(n=10, row_ptr=p, col=p, codes=p, hubs=None, n_hubs=0, lanes=8, census=p, ws=p, ws_bytes=need):
        return lib.grx_triad_census(n, row_ptr, col, codes, hubs, n_hubs, lanes, census, None, None, ws, ws_bytes, None)

    for bad in (dict(n=-1), dict(n=1 << 31), dict(row_ptr=None), dict(col=None), dict(codes=None), dict(census=None),
                dict(ws=None), dict(lanes=0), dict(lanes=5), dict(lanes=64), dict(n_hubs=3), dict(n_hubs=-1),
                dict(n_hubs=11, hubs=p), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert call(**bad) == -1, bad
        assert 'grx_triad_census' in lib.grx_last_error().decode(), bad
    # n == 0: nothing to do, nothing looked at
    assert lib.grx_triad_census(0, None, None, None, None, 0, 8, None, None, None, None, 0, None) == 0
