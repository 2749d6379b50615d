"""
The triad census on the MI355X: graphrole_amd.node_triad_census and triadic_census equal (integers: compared with ==) to
brute-force enumeration of all 3-subsets (tests/triad_oracle.py::brute_columns) on the graphs of up to 200 nodes --
the union of all 64 digraphs on three labelled nodes (every code at every vertex order, both walk directions), a
tournament (only 030T / 030C closed), a complete mutual digraph (only 300), a DAG, G(60, 0.3) with reciprocity, one arc,
one mutual pair, n = 1, 2, 3 -- and to the oracle's restatement of the formulas (tied to networkx in
tests/test_triads_cpu.py) beyond: the union of all 4 096 digraphs on four labelled nodes (every overlap of two triads
on a pair; exactly 2 048 workgroups x 8 rows at 32 lanes), the directed atlas union under both relabellings, BA(2000,
5) oriented at random with a fifth of its pairs mutual (hub rows at 4 lanes), a directed wheel whose hub row is longer
than 32 x 32 and holds every closed triad, a book of two adjacent hubs with 1 200 shared neighbours and rows of equal
length, and a graph with isolated nodes; kernels.triad_census on the adapter's CSR against the oracle on the same arrays
for every lane width (columns, totals, common neighbours per arc); the same bytes in a second run and for a relabelled
copy; nodelist; the refusals.
"""
import functools
from math import comb

import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import atlas
from tests import triad_oracle as to

pytestmark = pytest.mark.gpu

LANES = (4, 8, 16, 32)


def _union(k):
    return nx.disjoint_union_all(list(to.all_digraphs(k)))


def _oriented(G, seed, mutual=0.2):
    """Every edge of G as one arc in a seeded random direction, a fraction `mutual` of them in both."""
    rng = np.random.default_rng(seed)
    D = nx.DiGraph()
    D.add_nodes_from(G)
    for u, v in G.edges():
        x = rng.random()
        if x < mutual or rng.random() < 0.5:
            D.add_edge(u, v)
        if x < mutual or not D.has_edge(u, v):
            D.add_edge(v, u)
    return D


def _spoke(D, hub, v, k):
    """The pair (hub, v) in the class O, I or M of the hub, by k mod 3."""
    if k % 3 != 1:
        D.add_edge(hub, v)
    if k % 3 != 0:
        D.add_edge(v, hub)


def _wheel(rim=1500):
    D = nx.DiGraph()
    for k in range(rim):
        _spoke(D, 0, 1 + k, k)
        a, b = 1 + k, 1 + (k + 1) % rim
        if k % 2 or k % 7 == 0:
            D.add_edge(a, b)
        if not k % 2:
            D.add_edge(b, a)
    return D


def _book(pages=1200):
    """Two adjacent hubs 0 and 1 with the same neighbours: rows of equal length."""
    D = nx.DiGraph([(0, 1)])
    for k in range(pages):
        _spoke(D, 0, 2 + k, k)
        _spoke(D, 1, 2 + k, k // 3)
    return D


def _dag():
    G = nx.gnp_random_graph(70, 0.15, seed=4)
    return nx.DiGraph([(min(u, v), max(u, v)) for u, v in G.edges()])


def _isolated():
    D = _oriented(nx.barabasi_albert_graph(50, 3, seed=1), 2)
    D.add_nodes_from([1000, 1001, 1002])
    return D


BRUTE = {
    'union3': lambda: _union(3),
    'tournament40': lambda: _oriented(nx.complete_graph(40), 5, mutual=0.0),
    'mutual30': lambda: nx.complete_graph(30, create_using=nx.DiGraph),
    'dag': _dag,
    'gnp60': lambda: nx.gnp_random_graph(60, 0.3, seed=7, directed=True),
    'strings': lambda: nx.relabel_nodes(nx.gnp_random_graph(30, 0.2, seed=3, directed=True), lambda v: f'node-{v:02d}'),
    'arc': lambda: nx.DiGraph([(0, 1)]),
    'pair': lambda: nx.DiGraph([(0, 1), (1, 0)]),
    'n1': lambda: nx.empty_graph(1, create_using=nx.DiGraph),
    'n2': lambda: nx.empty_graph(2, create_using=nx.DiGraph),
    'path3': lambda: nx.DiGraph([(0, 1), (1, 2)]),
    'isolated': _isolated,
}
FORMULAS = {
    'union4': lambda: _union(4),
    'atlas': lambda: atlas.graph('directed', 'identity'),
    'atlas_perm': lambda: atlas.graph('directed', 'perm'),
    'ba2000': lambda: _oriented(nx.barabasi_albert_graph(2000, 5, seed=3), 6),
    'wheel': _wheel,
    'book': _book,
}
GRAPHS = {**BRUTE, **FORMULAS}


@functools.lru_cache(maxsize=None)
def _graph(key):
    return GRAPHS[key]()


@functools.lru_cache(maxsize=None)
def _want(key):
    """int64[16, n] behind the sorted nodes: by enumeration where that is affordable, else by the oracle's formulas;
    computed once per graph and never changed."""
    G = _graph(key)
    columns = to.brute_columns(G) if key in BRUTE else to.graph_census(G)[1].columns
    columns.setflags(write=False)
    return columns


@functools.lru_cache(maxsize=None)
def _frame(key):
    from graphrole_amd import node_triad_census
    return node_triad_census(_graph(key))


@pytest.mark.parametrize('key', list(GRAPHS))
def test_matches_the_oracle(key):
    from graphrole_amd import triadic_census
    G = _graph(key)
    n = len(G)
    frame = _frame(key)
    assert isinstance(frame, pd.DataFrame) and list(frame.columns) == to.COLUMNS
    assert all(dt == np.int64 for dt in frame.dtypes)
    assert list(frame.index) == sorted(G) and frame.shape == (n, 16)
    want = _want(key)
    assert np.array_equal(frame.to_numpy().T, want)
    assert not np.any(want.sum(axis=1) % 3) and np.all(want.sum(axis=0) == comb(n - 1, 2))
    census = to.as_dict(want.sum(axis=1) // 3)
    assert frame.attrs['census'] == census and sum(census.values()) == comb(n, 3)
    got = triadic_census(G)
    assert got == census and list(got) == list(to.NAMES) and all(type(x) is int for x in got.values())


def test_the_graph_kinds_are_what_they_are_here_for():
    from graphrole_amd import kernels as K, measures
    from graphrole_amd.graph.interface.networkx import NetworkxInterface

    def closed(key):
        s = _want(key).sum(axis=1)
        return {name for name in to.CLOSED if s[to.T[name]]}

    assert len(_graph('union3')) == 192 and np.all(_want('union3').sum(axis=1) > 0)
    assert len(_graph('union4')) == 16384 == K.RJ_ROW_MAX_WG * (K.RJ_BLOCK // 32)       # the capped grid, filled
    assert np.all(_want('union4').sum(axis=1) > 0)
    assert closed('tournament40') == {'030T', '030C'} and closed('mutual30') == {'300'} and closed('dag') == {'030T'}
    assert _want('mutual30')[to.T['300']].tolist() == [comb(29, 2)] * 30
    assert closed('gnp60') == set(to.CLOSED) == closed('ba2000')
    assert closed('wheel') == closed('book') == set(to.CLOSED) - {'300'}        # no two adjacent mutual spokes
    assert _want('isolated')[3:, -3:].sum() == 0 and _want('isolated')[:3, -3:].sum() > 0
    hubs = {}
    for key in ('ba2000', 'wheel', 'book'):
        graph = NetworkxInterface(_graph(key))
        csr = measures._triad_csr(graph, K)[0]
        hubs[key] = (csr.n_hubs, csr.lanes_per_row, int(np.diff(csr._host[0]).max()))
    assert hubs['ba2000'][0] > 0 and hubs['ba2000'][1] == 4
    assert hubs['wheel'] == (1, 4, 1500) and 1500 > 32 * 32
    assert hubs['book'] == (2, 4, 1201)                          # equal lengths: the tie walks u's row
    # every closed triad of the wheel holds the hub
    wheel = _want('wheel')
    rows = [to.T[name] for name in to.CLOSED]
    assert wheel[rows, 0].sum() * 3 == wheel[rows].sum() == 3 * 1500


def _kernel_run(csr, codes, **kwargs):
    from graphrole_amd import kernels as K
    columns, totals, arc = K.triad_census(csr, codes, want_totals=True, want_arc_triads=True, **kwargs)
    return K.to_host(columns).copy(), K.to_host(totals).copy(), K.to_host(arc)[:csr.nnz].copy()


def _adapter_arrays(key):
    from graphrole_amd import kernels as K, measures
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    graph = NetworkxInterface(_graph(key))
    csr, codes, host = measures._triad_csr(graph, K)
    return graph, csr, codes, host


@pytest.mark.parametrize('key', ['ba2000', 'wheel', 'book', 'union3', 'gnp60'])
def test_kernel_equals_oracle_on_the_same_csr_for_every_lane_width(key):
    _, csr, codes, (row_ptr, col, host_codes) = _adapter_arrays(key)
    assert host_codes.dtype == np.uint8 and set(np.unique(host_codes).tolist()) <= {1, 2, 3}
    rows = np.repeat(np.arange(csr.n), np.diff(row_ptr))
    assert not np.any(rows == col)                              # no diagonal entry
    mirror = np.searchsorted(rows * csr.n + col, col.astype(np.int64) * csr.n + rows)
    assert np.array_equal(host_codes[mirror], np.array([0, 2, 1, 3], dtype=np.uint8)[host_codes])
    want = to.census(row_ptr, col, host_codes)
    first = None
    for L in LANES:
        columns, totals, arc = _kernel_run(csr, codes, lanes=L)
        assert columns.dtype == np.int64 and totals.dtype == np.int64 and arc.dtype == np.int32
        assert columns.shape == (16, csr.n) and totals.shape == (16,)
        assert np.array_equal(columns, want.columns), L
        assert np.array_equal(totals, want.totals), L
        assert np.array_equal(arc, want.common), L
        again = _kernel_run(csr, codes, lanes=L)
        assert all(a.tobytes() == b.tobytes() for a, b in zip((columns, totals, arc), again)), L
        first = first or (columns, totals, arc)
        assert all(a.tobytes() == b.tobytes() for a, b in zip((columns, totals, arc), first)), L
    only = _kernel_run(csr, codes)[0]                           # the CSR's own width
    assert only.tobytes() == first[0].tobytes()


@pytest.mark.parametrize('key', ['ba2000', 'gnp60', 'book'])
def test_a_relabelled_copy_gives_the_same_rows(key):
    from graphrole_amd import node_triad_census
    G = _graph(key)
    nodes = sorted(G)
    perm = np.random.default_rng(12).permutation(len(nodes))
    relabel = {v: int(perm[k]) for k, v in enumerate(nodes)}
    H = nx.relabel_nodes(G, relabel)
    got = node_triad_census(H)
    back = got.loc[[relabel[v] for v in nodes]]
    assert back.to_numpy().tobytes() == _frame(key).to_numpy().tobytes()
    assert got.attrs['census'] == _frame(key).attrs['census']


@pytest.mark.parametrize('key', ['gnp60', 'strings'])
def test_nodelist(key):
    from graphrole_amd import node_triad_census, triadic_census
    G = _graph(key)
    nodes = sorted(G)
    rng = np.random.default_rng(9)
    for subset in ([nodes[k] for k in rng.permutation(len(nodes))[:7]], [nodes[5]], nodes):
        assert triadic_census(G, nodelist=subset) == nx.triadic_census(G, nodelist=subset)
    one = node_triad_census(G, nodes[5])
    assert isinstance(one, pd.Series) and dict(zip(to.NAMES, one.tolist())) == nx.triadic_census(G, nodelist=[nodes[5]])
    some = node_triad_census(G, [nodes[9], nodes[2]])
    assert list(some.index) == [nodes[2], nodes[9]] and some.equals(_frame(key).loc[[nodes[2], nodes[9]]])


def test_refusals_on_the_device_build():
    from graphrole_amd import node_triad_census, triadic_census
    L = nx.gnm_random_graph(20, 60, seed=2, directed=True)
    L.add_edge(3, 3)
    for fn in (triadic_census, node_triad_census):
        with pytest.raises(NotImplementedError, match=r'G\.to_directed\(\)'):
            fn(nx.karate_club_graph())
        with pytest.raises(NotImplementedError, match=r'nx\.DiGraph\(G\)'):
            fn(nx.MultiDiGraph([(0, 1), (0, 1), (1, 2)]))
        with pytest.raises(NotImplementedError, match=r'G\.remove_edges_from\(nx\.selfloop_edges\(G\)\)'):
            fn(L)
    D = _graph('gnp60')
    for bad in ([1, 1], [1, 99]):
        with pytest.raises(ValueError, match='duplicate nodes or nodes not in G'):
            triadic_census(D, nodelist=bad)
    with pytest.raises(KeyError):
        node_triad_census(D, [1, 99])
    empty = node_triad_census(nx.DiGraph())
    assert empty.shape == (0, 16) and empty.attrs['census'] == dict.fromkeys(to.NAMES, 0)
