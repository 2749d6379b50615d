"""
-m "not gpu": connected / weak / strong components, reachability and bow-tie position without a device.

* tests/components_oracle.py -- the numpy restatement of csrc/grx_components.hip the GPU tests compare the kernels
  with -- against networkx, exactly: a few thousand seeded graphs, all 4 096 digraphs on 4 nodes and all 1 024 graphs on
  5 nodes; the partition, label = the smallest row, size = the cardinality, descendants / ancestors from one and from
  several seeds, and the bow tie against its definition written with nx.descendants / nx.ancestors.
* graphrole_amd.components over a CPU double of kernels.components / kernels.reachable (the oracle on top of
  tests/fake_kernels): labels, orders, ranks and ties, every refusal, the null graph, the pinned catalogue.
* static checks of the header, the version, the ctypes table and the mirrored launch constants.
"""
import itertools
import os
import re
import types

import networkx as nx
import numpy as np
import pandas as pd
import pytest
import torch

from tests import components_oracle as co, fake_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------- the oracle against networkx
def _nx_partition(nodes, sets):
    row_of = {v: i for i, v in enumerate(nodes)}
    return frozenset(frozenset(row_of[v] for v in s) for s in sets)


def _check_labels(r, want):
    assert co.partition(r.label) == want
    assert r.n_components == len(want)
    for comp in want:
        rows = sorted(comp)
        assert np.all(r.label[rows] == rows[0]) and np.all(r.size[rows] == len(rows))
    assert r.label.dtype == np.int32 and r.size.dtype == np.int64


def _bow_tie_by_definition(G, nodes):
    """The six categories from nx.strongly_connected_components, nx.descendants and nx.ancestors; S = the largest
    component, ties by the smallest row."""
    row_of = {v: i for i, v in enumerate(nodes)}
    S = min(nx.strongly_connected_components(G), key=lambda c: (-len(c), min(row_of[v] for v in c)))
    anc = set().union(*(nx.ancestors(G, v) for v in S)) - S
    des = set().union(*(nx.descendants(G, v) for v in S)) - S
    from_in = set(anc).union(*(nx.descendants(G, v) for v in anc)) if anc else set()
    to_out = set(des).union(*(nx.ancestors(G, v) for v in des)) if des else set()
    code = np.full(len(nodes), 5, dtype=np.int8)
    for v in nodes:
        i = row_of[v]
        if v in S:
            code[i] = 0
        elif v in anc:
            code[i] = 1
        elif v in des:
            code[i] = 2
        elif v in from_in and v in to_out:
            code[i] = 3
        elif v in from_in or v in to_out:
            code[i] = 4
    return code


def _check_directed(G, rng, with_bow_tie=True):
    nodes, row_ptr, col, in_row_ptr, in_col = co.graph_csrs(G)
    _check_labels(co.components(row_ptr, col, co.STRONG), _nx_partition(nodes, nx.strongly_connected_components(G)))
    _check_labels(co.components(row_ptr, col, co.WEAK), _nx_partition(nodes, nx.weakly_connected_components(G)))
    n = len(nodes)
    for k in (1, 3):
        seeds = rng.choice(n, size=min(k, n), replace=False)
        flag = np.zeros(n, dtype=np.int32)
        flag[seeds] = 7
        down = set(seeds.tolist()).union(*({nodes.index(u) for u in nx.descendants(G, nodes[s])} for s in seeds))
        up = set(seeds.tolist()).union(*({nodes.index(u) for u in nx.ancestors(G, nodes[s])} for s in seeds))
        got, count, levels = co.reachable(row_ptr, col, flag)
        assert set(np.nonzero(got)[0].tolist()) == down and count == len(down) and got.max() == 1
        if k == 1:
            assert levels == max(nx.single_source_shortest_path_length(G, nodes[seeds[0]]).values())
        got, count, _ = co.reachable(in_row_ptr, in_col, flag)
        assert set(np.nonzero(got)[0].tolist()) == up and count == len(up)
    if with_bow_tie:
        assert np.array_equal(co.bow_tie(row_ptr, col, in_row_ptr, in_col), _bow_tie_by_definition(G, nodes))


@pytest.mark.parametrize('block', range(8))
def test_oracle_equals_networkx_on_seeded_digraphs(block):
    rng = np.random.default_rng(block)
    for seed in range(block * 60, block * 60 + 60):
        for G in co.directed_family(seed):
            _check_directed(G, rng)


@pytest.mark.parametrize('block', range(4))
def test_oracle_equals_networkx_on_seeded_undirected_graphs(block):
    for seed in range(block * 60, block * 60 + 60):
        for G in co.undirected_family(seed):
            nodes, row_ptr, col, _, _ = co.graph_csrs(G)
            _check_labels(co.components(row_ptr, col, co.CONNECTED), _nx_partition(nodes, nx.connected_components(G)))
            flag = np.zeros(len(nodes), dtype=np.int32)
            flag[0] = 1
            got, count, _ = co.reachable(row_ptr, col, flag)
            want = nx.node_connected_component(G, nodes[0])
            assert {nodes[i] for i in np.nonzero(got)[0]} == want and count == len(want)


def test_oracle_every_digraph_on_four_nodes():
    pairs = [(u, v) for u in range(4) for v in range(4) if u != v]
    n, row_ptr, col = co.all_digraphs4()
    strong, weak = co.components(row_ptr, col, co.STRONG), co.components(row_ptr, col, co.WEAK)
    C = 1 << 12
    assert n == 4 * C
    for bits in range(C):
        G = nx.DiGraph()
        G.add_nodes_from(range(4))
        G.add_edges_from(p for k, p in enumerate(pairs) if bits >> k & 1)
        rows = np.arange(4) * C + bits
        for r, sets in ((strong, nx.strongly_connected_components(G)), (weak, nx.weakly_connected_components(G))):
            for comp in sets:
                members = rows[sorted(comp)]
                assert np.all(r.label[members] == members[0]) and np.all(r.size[members] == len(members)), bits
    # the union as a whole: the same answer as each graph alone, and a few of them against the definition of the bow tie
    rng = np.random.default_rng(4)
    for bits in rng.integers(0, C, size=200):
        G = nx.DiGraph()
        G.add_nodes_from(range(4))
        G.add_edges_from(p for k, p in enumerate(pairs) if int(bits) >> k & 1)
        _check_directed(G, rng)


def test_oracle_every_graph_on_five_nodes():
    pairs = list(itertools.combinations(range(5), 2))
    n, row_ptr, col = co.all_graphs5()
    r = co.components(row_ptr, col, co.CONNECTED)
    C = 1 << 10
    assert n == 5 * C
    total = 0
    for bits in range(C):
        G = nx.empty_graph(5)
        G.add_edges_from(p for k, p in enumerate(pairs) if bits >> k & 1)
        rows = np.arange(5) * C + bits
        for comp in nx.connected_components(G):
            members = rows[sorted(comp)]
            assert np.all(r.label[members] == members[0]) and np.all(r.size[members] == len(members)), bits
            total += 1
    assert r.n_components == total


def test_oracle_round_counts_of_the_stated_cases():
    """The counts the header of csrc/grx_components.hip states: a directed k-cycle takes 2 k + 2 rounds, a directed
    k-path k / 2, the ascending chain of k two-cycles one outer iteration per component and the descending one a single
    one."""
    for k in (5, 53, 64):
        r = co.components(*co.cycle(k), co.STRONG)
        assert (r.rounds, r.outer, r.n_components) == (2 * k + 2, 1, 1)
        r = co.components(*co.path(k), co.STRONG)
        assert (r.rounds, r.outer, r.n_components) == ((k + 1) // 2, 0, k)
    up, down = co.components(*co.two_cycle_chain(32), co.STRONG), co.components(*co.two_cycle_chain(32, False), co.STRONG)
    assert up.outer == 32 and up.rounds > 2 * co.ROUND_BATCH and down.outer == 1 and down.rounds < co.ROUND_BATCH
    # the numbers the header of csrc/grx_components.hip and DESIGN.md quote
    assert (up.rounds, up.outer) == (1184, 32) and (down.rounds, down.outer) == (6, 1)
    assert up.n_components == down.n_components == 32 and np.all(up.size == 2) and np.all(down.size == 2)
    assert co.components(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), co.STRONG).n_components == 0
    for mode in (co.CONNECTED, co.WEAK, co.STRONG):
        r = co.components(np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int64), mode)
        assert r.label.tolist() == [0, 1, 2] and r.size.tolist() == [1, 1, 1] and r.n_components == 3
        loops = co.components(np.arange(4, dtype=np.int64), np.arange(3, dtype=np.int64), mode)
        assert loops.label.tolist() == [0, 1, 2] and loops.n_components == 3


def test_hub_cases_and_motif_hold_what_they_are_there_for():
    for kind in co.HUB_CASES:
        row_ptr, col = co.hub_case(kind)
        t_ptr, t_col = co.transpose(row_ptr, col)
        long_out, long_in = np.diff(row_ptr).max() > 128, np.diff(t_ptr).max() > 128
        assert (long_out, long_in) == (kind.endswith('out'), kind.endswith('in'))
        assert np.argmax(np.diff(row_ptr) + np.diff(t_ptr)) == 0 and np.diff(row_ptr)[1:].max() <= 128 >= np.diff(t_ptr)[1:].max()
        r = co.components(row_ptr, col, co.STRONG)
        gone, trimmed = co.strong_trace(row_ptr, col)
        if kind.startswith('scc'):
            assert r.size[0] > 70 and r.outer >= 1 and not trimmed[0]
        elif kind in ('source_out', 'sink_in'):
            # the hub's short row is empty: trimmed at once
            assert r.size[0] == 1 and np.count_nonzero(r.size == 3) == 3 and trimmed[0] and gone[0] == 1
        else:
            # the hub leaves in a TRIM round later than 1, because of its long row: the one entry of its short row
            # (row 1, on the 3-cycle) is still alive then, and every entry of the long row left the round before
            short = (t_ptr, t_col) if kind == 'sink_out' else (row_ptr, col)
            long_ = (row_ptr, col) if kind == 'sink_out' else (t_ptr, t_col)
            assert short[1][short[0][0]:short[0][1]].tolist() == [1]
            arms = long_[1][long_[0][0]:long_[0][1]]
            assert len(arms) > 128 and np.all(gone[arms] == 1) and np.all(trimmed[arms])
            assert trimmed[0] and gone[0] == 2 and gone[1] > 2 and not trimmed[1]
            assert r.size[0] == 1 and r.size[1] == 3 and r.outer == 1
    row_ptr, col = co.motif()
    r = co.components(row_ptr, col, co.STRONG)
    assert np.diff(row_ptr).max() > 128 and r.outer == 2 and r.size[0] > 40 and r.size[-1] == 1
    assert np.count_nonzero(r.size == 3) == 3 and np.diff(row_ptr)[-1] == 0
    assert co.components(row_ptr, col, co.WEAK).n_components == 2


# ------------------------------------------------------------------------------------- the Python layer over a double
def _arrays(csr):
    return np.asarray(csr.row_ptr, dtype=np.int64), np.asarray(csr.col, dtype=np.int64)


@pytest.fixture
def cpu_backend():
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.calls = []

    def components(csr, in_csr=None, mode='connected', want_size=True, lanes=None):
        double.calls.append(('components', mode, in_csr is not None))
        row_ptr, col = _arrays(csr)
        if mode == 'strong':
            t_ptr, t_col = _arrays(in_csr)
            assert (t_ptr.tolist(), t_col.tolist()) == tuple(a.tolist() for a in co.transpose(row_ptr, col))
        r = co.components(row_ptr, col, mode)
        return (torch.from_numpy(r.label.copy()), torch.from_numpy(r.size.copy()) if want_size else None,
                r.n_components, r.rounds)

    def reachable(csr, flag, lanes=None):
        double.calls.append(('reachable',))
        out, count, levels = co.reachable(*_arrays(csr), np.asarray(flag))
        return torch.from_numpy(out), count, levels

    double.components, double.reachable = components, reachable
    backend.use(double)
    yield double
    backend.use(None)


def _strings(G):
    return nx.relabel_nodes(G, lambda v: f'node-{v:03d}')


def _shuffled(G, seed):
    order = list(G)
    np.random.default_rng(seed).shuffle(order)
    H = G.__class__()
    H.add_nodes_from(order)
    H.add_edges_from(G.edges())
    return H


def _undirected_cases():
    G = nx.disjoint_union(nx.barabasi_albert_graph(40, 2, seed=1), nx.cycle_graph(9))
    G.add_nodes_from([49, 50])
    G.add_edge(50, 50)
    yield 'plain', G
    yield 'strings', _strings(G)
    yield 'relabelled', _shuffled(nx.relabel_nodes(G, {v: (v * 37) % 101 for v in G}), 2)
    M = nx.MultiGraph(G)
    M.add_edges_from([(0, 1), (0, 1), (45, 46), (3, 3)])
    yield 'multigraph', M
    yield 'no_edges', nx.empty_graph(5)
    yield 'n1', nx.empty_graph(1)


def _directed_cases():
    G = nx.gnm_random_graph(45, 70, seed=5, directed=True)
    G.add_nodes_from([45, 46])
    G.add_edges_from([(46, 46), (3, 3)])
    yield 'plain', G
    yield 'strings', _strings(G)
    yield 'relabelled', _shuffled(nx.relabel_nodes(G, {v: (v * 37) % 101 for v in G}), 3)
    M = nx.MultiDiGraph(G)
    M.add_edges_from([(0, 1), (0, 1), (1, 0), (7, 7)])
    yield 'multigraph', M
    yield 'dense', nx.gnm_random_graph(30, 120, seed=6, directed=True)
    yield 'no_arcs', nx.empty_graph(4, create_using=nx.DiGraph)
    yield 'n1', nx.empty_graph(1, create_using=nx.DiGraph)


def _ordered(sets):
    return sorted((set(s) for s in sets), key=min)


def _check_table(table, sets, G):
    """component = the rank by decreasing size, ties by first member in the index; component_size; the index."""
    assert list(table.columns) == ['component', 'component_size'] and list(table.index) == sorted(G)
    assert table['component'].dtype == np.int64 and table['component_size'].dtype == np.int64
    ranked = sorted(sets, key=lambda s: (-len(s), min(s)))
    for rank, s in enumerate(ranked):
        assert set(table.index[table['component'] == rank]) == s
        assert np.all(table.loc[sorted(s), 'component_size'] == len(s))
    assert table.attrs['n_components'] == len(sets)
    return ranked


@pytest.mark.parametrize('key', [k for k, _ in _undirected_cases()])
def test_undirected_public_functions(cpu_backend, key):
    import graphrole_amd as ga
    G = dict(_undirected_cases())[key]
    want = _ordered(nx.connected_components(G))
    got = ga.connected_components(G)
    assert isinstance(got, list) and got == want                # ordered by first member in the index
    assert ga.number_connected_components(G) == nx.number_connected_components(G)
    assert ga.is_connected(G) == nx.is_connected(G)
    ranked = _check_table(ga.component_table(G), want, G)
    assert ga.component_table(G, kind='connected').equals(ga.component_table(G))
    assert ga.component_table(G).attrs['rounds'] == 0
    giant = ga.largest_component(G)
    assert isinstance(giant, pd.Index) and list(giant) == sorted(ranked[0])
    for v in list(G)[:3]:
        assert ga.descendants(G, v) == nx.descendants(G, v) == ga.ancestors(G, v)


@pytest.mark.parametrize('key', [k for k, _ in _directed_cases()])
def test_directed_public_functions(cpu_backend, key):
    import graphrole_amd as ga
    G = dict(_directed_cases())[key]
    weak, strong = _ordered(nx.weakly_connected_components(G)), _ordered(nx.strongly_connected_components(G))
    assert ga.weakly_connected_components(G) == weak and ga.strongly_connected_components(G) == strong
    assert ga.number_weakly_connected_components(G) == len(weak)
    assert ga.number_strongly_connected_components(G) == len(strong)
    assert ga.is_weakly_connected(G) == nx.is_weakly_connected(G)
    assert ga.is_strongly_connected(G) == nx.is_strongly_connected(G)
    _check_table(ga.component_table(G), weak, G)                # None = weak for a directed graph
    ranked = _check_table(ga.component_table(G, kind='strong'), strong, G)
    assert ga.component_table(G, kind='weak').equals(ga.component_table(G))
    assert list(ga.largest_component(G, kind='strong')) == sorted(ranked[0])
    for v in list(G)[:4]:
        assert ga.descendants(G, v) == nx.descendants(G, v) and ga.ancestors(G, v) == nx.ancestors(G, v)
    tie = ga.bow_tie(G)
    nodes = sorted(G)
    want = _bow_tie_by_definition(G, nodes)
    assert list(tie.index) == nodes and tie.name == 'bow_tie'
    assert list(tie.cat.categories) == ['core', 'in', 'out', 'tube', 'tendril', 'other']
    assert np.array_equal(tie.cat.codes.to_numpy(), want)
    assert tie.attrs['sizes'] == {c: int((want == k).sum()) for k, c in enumerate(tie.cat.categories)}
    assert set(tie.index[tie == 'core']) == ranked[0]


def test_weak_needs_no_in_adjacency_and_strong_is_refused_without(cpu_backend):
    import graphrole_amd as ga
    from graphrole_amd import components, measures
    G = nx.gnm_random_graph(20, 40, seed=1, directed=True)
    graph = measures._adapter(G)
    out = graph._structure_csrs()[0]
    graph._structure_csrs = lambda: (out, None)
    real = measures._adapter
    try:
        measures._adapter = components._adapter = lambda _: graph
        assert ga.weakly_connected_components(G) == _ordered(nx.weakly_connected_components(G))
        assert ga.descendants(G, 0) == nx.descendants(G, 0)
        cpu_backend.calls.clear()
        for call in (lambda: ga.strongly_connected_components(G), lambda: ga.bow_tie(G), lambda: ga.ancestors(G, 0),
                     lambda: ga.component_table(G, kind='strong'), lambda: ga.is_strongly_connected(G)):
            with pytest.raises(NotImplementedError, match='has no in-adjacency for this directed graph'):
                call()
        assert cpu_backend.calls == []
    finally:
        measures._adapter = components._adapter = real


def test_rank_ties_go_to_the_first_member_in_the_index(cpu_backend):
    import graphrole_amd as ga
    # two 3-cycles and a 2-cycle; the cycle with the later labels comes first in the graph's own node order
    G = nx.DiGraph()
    nx.add_cycle(G, ['x', 'y', 'z'])
    nx.add_cycle(G, ['a', 'b', 'c'])
    nx.add_cycle(G, ['m', 'n'])
    G.add_edge('c', 'x')
    table = ga.component_table(G, kind='strong')
    assert table.loc[['a', 'b', 'c'], 'component'].tolist() == [0, 0, 0]
    assert table.loc[['x', 'y', 'z'], 'component'].tolist() == [1, 1, 1]
    assert table.loc[['m', 'n'], 'component'].tolist() == [2, 2]
    assert list(ga.largest_component(G, kind='strong')) == ['a', 'b', 'c']
    assert ga.strongly_connected_components(G) == [{'a', 'b', 'c'}, {'m', 'n'}, {'x', 'y', 'z'}]
    tie = ga.bow_tie(G)
    assert tie[['a', 'x', 'm']].tolist() == ['core', 'out', 'other'] and tie.attrs['sizes']['out'] == 3
    U = nx.Graph([(5, 6), (1, 2), (9, 9)])
    assert ga.component_table(U)['component'].to_dict() == {1: 0, 2: 0, 5: 1, 6: 1, 9: 2}
    assert list(ga.largest_component(U)) == [1, 2]


def test_every_refusal_and_the_null_graph(cpu_backend):
    import graphrole_amd as ga
    U, D = nx.path_graph(4), nx.gnm_random_graph(6, 9, seed=1, directed=True)
    cpu_backend.calls.clear()
    for name in ('connected_components', 'number_connected_components', 'is_connected'):
        with pytest.raises(NotImplementedError, match=rf'networkx does not implement nx\.{name}\(G\) for a directed graph'):
            getattr(ga, name)(D)
    for name in ('weakly_connected_components', 'strongly_connected_components', 'number_weakly_connected_components',
                 'number_strongly_connected_components', 'is_weakly_connected', 'is_strongly_connected'):
        with pytest.raises(NotImplementedError,
                           match=rf'networkx does not implement nx\.{name}\(G\) for an undirected graph'):
            getattr(ga, name)(U)
    with pytest.raises(NotImplementedError, match='for a directed graph.*to_undirected'):
        ga.component_table(D, kind='connected')
    for kind in ('weak', 'strong'):
        with pytest.raises(NotImplementedError, match='for an undirected graph.*to_directed'):
            ga.component_table(U, kind=kind)
        with pytest.raises(NotImplementedError, match='for an undirected graph'):
            ga.largest_component(U, kind=kind)
    with pytest.raises(NotImplementedError, match='bow_tie is defined for a directed graph'):
        ga.bow_tie(U)
    with pytest.raises(ValueError, match="kind must be 'connected', 'weak', 'strong' or None"):
        ga.component_table(U, kind='giant')
    for f, G, word in ((ga.descendants, D, 'digraph'), (ga.ancestors, D, 'digraph'), (ga.descendants, U, 'graph')):
        with pytest.raises(nx.NetworkXError, match=f'The node 77 is not in the {word}'):
            f(G, 77)
    with pytest.raises(TypeError, match='supported libraries'):
        ga.connected_components([1, 2])
    for f, G in ((ga.is_connected, nx.Graph()), (ga.is_weakly_connected, nx.DiGraph()),
                 (ga.is_strongly_connected, nx.DiGraph())):
        with pytest.raises(nx.NetworkXPointlessConcept, match='Connectivity is undefined for the null graph'):
            f(G)
    assert cpu_backend.calls == []                              # no refusal reaches a kernel
    # n = 0 works everywhere else
    assert ga.connected_components(nx.Graph()) == [] and ga.number_strongly_connected_components(nx.DiGraph()) == 0
    table = ga.component_table(nx.DiGraph(), kind='strong')
    assert table.shape == (0, 2) and table.attrs == {'n_components': 0, 'rounds': 0}
    assert len(ga.largest_component(nx.Graph())) == 0
    tie = ga.bow_tie(nx.DiGraph())
    assert len(tie) == 0 and tie.attrs['sizes'] == dict.fromkeys(['core', 'in', 'out', 'tube', 'tendril', 'other'], 0)


def test_catalogue_and_default_table_are_unchanged(cpu_backend):
    from graphrole_amd import measures
    assert list(measures.CATALOGUE) == [
        'degree', 'weighted_degree', 'in_degree', 'out_degree', 'clustering', 'effective_size', 'constraint', 'pagerank',
        'eigenvector', 'betweenness_centrality', 'closeness_centrality', 'harmonic_centrality',
        'biconnected_components', 'core_number', 'onion_layer', 'eccentricity']
    assert measures.OPT_IN == ('betweenness_centrality', 'closeness_centrality', 'harmonic_centrality',
                               'biconnected_components', 'core_number', 'onion_layer', 'eccentricity', 'constraint')
    assert measures.available_measures(False, False) == ['degree', 'weighted_degree', 'clustering', 'effective_size',
                                                         'pagerank', 'eigenvector']
    assert measures.available_measures(True, False) == ['degree', 'weighted_degree', 'in_degree', 'out_degree',
                                                        'pagerank', 'eigenvector']
    with pytest.raises(ValueError, match='catalogue'):
        measures.node_measures(nx.path_graph(3), ['component_size'])


# -------------------------------------------------------------------------------------------------------- static checks
def _source(name):
    return open(os.path.join(ROOT, 'graphrole_amd', 'csrc', name)).read()


def test_header_version_declarations_and_signatures():
    from graphrole_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'grx.h')).read()
    assert re.search(r'#define\s+GRX_VERSION\s+1100\b', header)
    assert 'enum { GRX_COMPONENTS_CONNECTED = 0, GRX_COMPONENTS_WEAK = 1, GRX_COMPONENTS_STRONG = 2 };' in header
    for name, args in (('grx_components_workspace_bytes', 1), ('grx_components', 19),
                       ('grx_reachable_workspace_bytes', 1), ('grx_reachable', 12)):
        decl = re.search(r'\b(?:size_t|int) ' + name + r'\(([^;]*)\);', header)
        assert decl and len(decl.group(1).split(',')) == args == len(_lib._SIGNATURES[name][1]), name
    lib = _lib.load()
    assert lib.grx_version() == 1100
    assert lib.grx_components_workspace_bytes(1000) >= 16 * 1000 and lib.grx_reachable_workspace_bytes(1000) >= 4000
    assert 'grx_components.hip' in _source('Makefile') and 'grx_unionfind.h' in _source('Makefile')


def test_the_mirrored_constants_are_the_ones_in_the_source():
    from graphrole_amd import kernels as K
    text = _source('grx_components.hip')
    for constant in ('CP_BLOCK', 'CP_GROUP', 'CP_MAX_BLOCKS', 'CP_MAX_ROW_BLOCKS', 'CP_ROUND_BATCH'):
        found = re.findall(r'\bconstexpr int ' + constant + r' = (\d+);', text)
        assert len(found) == 1 and int(found[0]) == getattr(K, constant), (constant, found)
    assert co.ROUND_BATCH == K.CP_ROUND_BATCH
    assert K.COMPONENT_MODES == {'connected': 0, 'weak': 1, 'strong': 2}
    # every capped launch of the file is one of these two shapes: the second-trip test wraps both
    calls = set(re.findall(r'grx_grid\((?:[^()]|\([^()]*\))*\)', text))
    assert calls == {'grx_grid(n, CP_BLOCK, CP_MAX_BLOCKS)', 'grx_grid(n, CP_BLOCK / CP_GROUP, CP_MAX_ROW_BLOCKS)'}
    assert int(re.search(r'constexpr int GRX_HUB_FACTOR = (\d+);', _source('grx_common.h')).group(1)) == K.HUB_FACTOR
    # one copy of the union-find
    assert 'atomicCAS(' not in _source('grx_biconnected.hip') and 'grx_uf_union' in _source('grx_unionfind.h')


def test_argument_validation_needs_no_device():
    import ctypes
    from graphrole_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    n_comp, rounds = ctypes.c_int64(-1), ctypes.c_int64(-1)

    def call(n=10, mode=2, in_row_ptr=p, in_col=p, in_lanes=8, label=p, ws_bytes=1 << 20, lanes=8):
        return lib.grx_components(n, p, p, None, 0, lanes, in_row_ptr, in_col, None, 0, in_lanes, mode, label, None,
                                  ctypes.byref(n_comp), ctypes.byref(rounds), p, ws_bytes, None)

    assert call(mode=2, in_row_ptr=None, in_col=None) == -1 and b'needs the in CSR' in lib.grx_last_error()
    assert call(mode=0) == -1 and b'no in CSR' in lib.grx_last_error()
    assert call(mode=3) == -1 and b'mode' in lib.grx_last_error()
    assert call(n=-1) == -1 and call(n=1 << 31) == -1 and call(label=None) == -1 and call(lanes=0) == -1
    assert call(ws_bytes=16) == -1 and b'workspace' in lib.grx_last_error()
    assert call(n=0) == 0 and (n_comp.value, rounds.value) == (0, 0)
    count, levels = ctypes.c_int64(-1), ctypes.c_int64(-1)

    def reach(n=10, flag=p, ws_bytes=1 << 20, lanes=8, hubs=0):
        return lib.grx_reachable(n, p, p, None, hubs, lanes, flag, ctypes.byref(count), ctypes.byref(levels), p,
                                 ws_bytes, None)

    assert reach(flag=None) == -1 and reach(lanes=0) == -1 and reach(hubs=3) == -1 and reach(n=-2) == -1
    assert reach(ws_bytes=8) == -1 and b'workspace' in lib.grx_last_error()
    assert reach(n=0) == 0 and (count.value, levels.value) == (0, 0)
