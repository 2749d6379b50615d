"""
-m "not gpu": edge betweenness centrality without a device.  tests/edge_betweenness_oracle.py against
nx.edge_betweenness_centrality on every graph kind and option (the missing n / k of a sampled run among them), then
the Python layer of graphrole_amd.edge_betweenness_centrality over a CPU double of kernels.edge_betweenness /
kernels.weighted_edge_betweenness (the oracle on the double's CSR arrays): index, sources, scale, refusals, and the
header.  The device numbers are pinned in tests/test_gpu_edge_betweenness.py.
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

from tests import edge_betweenness_oracle as eo
from tests import fake_kernels
from tests import weighted_betweenness_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loops_isolated(directed=False):
    G = nx.gnm_random_graph(120, 400, seed=7, directed=directed)
    G.add_edges_from([(3, 3), (10, 10)])
    G.add_nodes_from([500, 501])
    return G


GRAPHS = {
    'karate': nx.karate_club_graph,
    'er300': lambda: nx.gnm_random_graph(300, 1200, seed=1),
    'er300_directed': lambda: nx.gnm_random_graph(300, 1200, seed=1, directed=True),
    'ba300': lambda: nx.barabasi_albert_graph(300, 3, seed=2),
    'loops_isolated': _loops_isolated,
    'directed_loops_isolated': lambda: _loops_isolated(True),
    'n3': lambda: nx.path_graph(3),
    'n2': lambda: nx.path_graph(2),
    'n1': lambda: nx.empty_graph(1),
}

OPTIONS = {'default': dict(), 'raw': dict(normalized=False), 'sampled': dict(k=40, seed=3)}


def _close(G, got: dict, want: dict):
    want = eo.by_sorted_ends(G, want)
    assert set(got) == set(want)
    keys = list(want)
    a, b = np.array([got[e] for e in keys]), np.array([want[e] for e in keys])
    np.testing.assert_allclose(a, b, rtol=eo.RTOL, atol=0)
    assert np.array_equal(a == 0, b == 0)                       # what networkx has at exactly 0 is exactly 0


@pytest.mark.parametrize('opts', list(OPTIONS))
@pytest.mark.parametrize('key', list(GRAPHS))
def test_oracle_matches_networkx(key, opts):
    G = GRAPHS[key]()
    kw = dict(OPTIONS[opts])
    if kw.get('k', 0) > G.number_of_nodes():
        kw['k'] = G.number_of_nodes()
    _close(G, eo.edge_betweenness(G, **kw), nx.edge_betweenness_centrality(G, **kw))


def test_a_sampled_run_is_not_scaled_by_n_over_k():
    """networkx 3.4.2 does not pass k to _rescale_e: with the k = n sources in the graph's own order a "sampled" run is
    the full run, and with k < n the sums are NOT multiplied by n / k."""
    G = nx.karate_club_graph()
    assert eo.rescale_e_factor(34, True, False) == 1 / (34 * 33)
    rng = random.Random(3)
    sources = rng.sample(list(G.nodes()), 10)
    want = nx.edge_betweenness_centrality(G, k=10, seed=3)
    row_ptr, col = eo.bo.csr_of(G, sorted(G))
    u, v, val = eo.edge_values(row_ptr, col, eo.arc_sums(row_ptr, col, sources), False, 1 / (34 * 33))
    _close(G, {(int(a), int(b)): float(c) for a, b, c in zip(u, v, val)}, want)


@pytest.mark.parametrize('kind', ['ints', 'uniform'])
@pytest.mark.parametrize('key', ['karate', 'er300', 'er300_directed', 'loops_isolated'])
def test_weighted_oracle_matches_networkx(key, kind):
    G = wo.with_weights(GRAPHS[key](), kind, seed=4)
    _close(G, eo.edge_betweenness(G, weight='weight'), nx.edge_betweenness_centrality(G, weight='weight'))
    _close(G, eo.edge_betweenness(G, weight='weight', k=30, seed=3, normalized=False),
           nx.edge_betweenness_centrality(G, weight='weight', k=30, seed=3, normalized=False))


def test_weighted_oracle_with_unit_weights_is_the_unweighted_one():
    G = nx.barabasi_albert_graph(80, 3, seed=3)
    a, b = eo.edge_betweenness(G), eo.edge_betweenness(G, weight='weight')
    assert list(a) == list(b)
    np.testing.assert_allclose(list(b.values()), list(a.values()), rtol=eo.RTOL, atol=0)


def test_incident_edges_identity_on_the_oracle():
    """Undirected, every node a source, unnormalised (scale 0.5 both): the edge values at a node sum to twice its node
    betweenness plus (reach - 1) -- every path that passes through v uses two of v's edges, every path that ends at v
    one, and there are reach - 1 of the latter counted from either end, halved."""
    G = nx.barabasi_albert_graph(300, 3, seed=2)
    edges = eo.edge_betweenness(G, normalized=False)
    node = eo.bo.betweenness(G, normalized=False)
    total = dict.fromkeys(G, 0.0)
    for (a, b), c in edges.items():
        total[a] += c
        total[b] += c
    reach = len(G)                                              # connected
    for v in G:
        assert abs(total[v] - (reach - 1) - 2 * node[v]) <= eo.RTOL * G.degree(v) * total[v]


# ------------------------------------------------------------------------------------------ Python layer, CPU double
@pytest.fixture
def cpu_backend():
    import torch
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.calls = []

    def both_slots(csr, arc, directed, scale):
        row_ptr, col = np.asarray(csr.row_ptr, dtype=np.int64), np.asarray(csr.col, dtype=np.int64)
        n = len(row_ptr) - 1
        u = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
        if directed:
            return arc * scale
        key = u * n + col
        mirror = np.searchsorted(key, col * n + u)
        return np.where(u == col, arc, arc + arc[mirror]) * scale    # both arcs of an edge hold its value

    def edge_betweenness(csr_out, csr_in, sources, scale, batch=0):
        sources = np.asarray(sources, dtype=np.int64)
        double.calls.append(dict(kind='hops', sources=sources.copy(), scale=scale, out=csr_out, inn=csr_in))
        arc = eo.arc_sums(csr_out.row_ptr, csr_out.col, sources)
        return torch.from_numpy(both_slots(csr_out, arc, csr_in is not None, scale))

    def arrays(csr):
        w = np.ones(len(csr.col)) if csr.w is None else np.asarray(csr.w, dtype=np.float64)
        return np.asarray(csr.row_ptr, dtype=np.int64), np.asarray(csr.col, dtype=np.int64), w

    def weighted_edge_betweenness(csr_out, csr_in, sources, scale, batch=0):
        sources = np.asarray(sources, dtype=np.int64)
        double.calls.append(dict(kind='weight', sources=sources.copy(), scale=scale, out=csr_out, inn=csr_in))
        out = arrays(csr_out)
        inn = out if csr_in is None else arrays(csr_in)
        arc, levels = eo.weighted_arc_sums(out, inn, sources)
        return (torch.from_numpy(both_slots(csr_out, arc, csr_in is not None, scale)),
                wo.relaxation_rounds(inn, sources), levels)

    double.edge_betweenness = edge_betweenness
    double.weighted_edge_betweenness = weighted_edge_betweenness
    backend.use(double)
    yield double
    backend.use(None)


def _series(G, series, want: dict):
    want = eo.by_sorted_ends(G, want)
    assert isinstance(series, pd.Series) and series.dtype == np.float64
    assert series.name == 'edge_betweenness_centrality' and list(series.index.names) == ['u', 'v']
    assert list(series.index) == sorted(want)                  # lexicographic, u before v when undirected
    got, ref = series.to_numpy(), np.array([want[e] for e in series.index])
    np.testing.assert_allclose(got, ref, rtol=eo.RTOL, atol=0)
    assert np.array_equal(got == 0, ref == 0)


def _internal_ids(G, nodes):
    from graphrole_amd.graph.csr import InternalGraph
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    row_of = {v: i for i, v in enumerate(sorted(G.nodes))}
    return InternalGraph(NetworkxInterface(G).to_csr()).inv[[row_of[v] for v in nodes]]


@pytest.mark.parametrize('opts', list(OPTIONS))
@pytest.mark.parametrize('key', ['karate', 'loops_isolated', 'directed_loops_isolated', 'n3', 'n2'])
def test_public_function_matches_networkx(cpu_backend, key, opts):
    from graphrole_amd import edge_betweenness_centrality
    G = GRAPHS[key]()
    kw = dict(OPTIONS[opts])
    if kw.get('k', 0) > G.number_of_nodes():
        kw['k'] = G.number_of_nodes()
    got = edge_betweenness_centrality(G, **kw)
    _series(G, got, nx.edge_betweenness_centrality(G, **kw))
    (call,) = cpu_backend.calls
    n = G.number_of_nodes()
    assert call['kind'] == 'hops' and (call['inn'] is not None) == G.is_directed()
    assert call['scale'] == eo.rescale_e_factor(n, kw.get('normalized', True), G.is_directed())
    expected = list(G) if 'k' not in kw else random.Random(3).sample(list(G.nodes()), kw['k'])
    assert np.array_equal(call['sources'], _internal_ids(G, expected))
    assert got.attrs == {}


@pytest.mark.parametrize('directed', [False, True])
def test_weighted_form_and_attrs(cpu_backend, directed):
    from graphrole_amd import edge_betweenness_centrality
    G = wo.with_weights(nx.gnm_random_graph(50, 260, seed=3, directed=directed), 'ints', seed=2)
    H = type(G)()
    H.add_nodes_from(random.Random(0).sample(list(G), 50))       # graph order differs from label order
    H.add_edges_from(G.edges(data=True))
    for seed in (5, random.Random(5)):
        got = edge_betweenness_centrality(H, weight='weight', k=20, seed=seed)
        _series(H, got, nx.edge_betweenness_centrality(H, weight='weight', k=20, seed=5))
        call = cpu_backend.calls[-1]
        assert call['kind'] == 'weight' and call['scale'] == 1 / (50 * 49) and (call['inn'] is not None) == directed
        assert np.array_equal(call['sources'], _internal_ids(H, random.Random(5).sample(list(H.nodes()), 20)))
        assert set(got.attrs) == {'rounds', 'levels'} and got.attrs['levels'] >= 2 and got.attrs['rounds'] >= 3


def test_string_labels_and_csr_graph_input(cpu_backend):
    from graphrole_amd import edge_betweenness_centrality
    from graphrole_amd.graph.csr import CSRGraph
    G = nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}')
    _series(G, edge_betweenness_centrality(G), nx.edge_betweenness_centrality(G))
    B = nx.barabasi_albert_graph(60, 3, seed=8)
    src, dst = np.array(list(B.edges)).T
    _series(B, edge_betweenness_centrality(CSRGraph(60, src, dst)), nx.edge_betweenness_centrality(B))


def test_empty_graphs_return_the_empty_series_without_device_work(cpu_backend):
    from graphrole_amd import edge_betweenness_centrality
    for G in (nx.empty_graph(0), nx.empty_graph(1), nx.empty_graph(5, create_using=nx.DiGraph)):
        for weight in (None, 'weight'):
            got = edge_betweenness_centrality(G, weight=weight)
            assert len(got) == 0 and got.dtype == np.float64 and got.name == 'edge_betweenness_centrality'
            assert list(got.index.names) == ['u', 'v'] and got.index.nlevels == 2
            assert got.attrs == ({} if weight is None else dict(rounds=0, levels=0))
    assert cpu_backend.calls == []


def test_refusals_before_any_device_work(cpu_backend, monkeypatch):
    from graphrole_amd import edge_betweenness_centrality
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    G = nx.karate_club_graph()
    for multi in (nx.MultiGraph([(0, 1), (0, 1), (1, 2)]), nx.MultiDiGraph([(0, 1), (1, 0)])):
        for weight in (None, 'weight'):
            with pytest.raises(NotImplementedError, match='parallel edges'):
                edge_betweenness_centrality(multi, weight=weight)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        H = G.copy()
        H[0][1]['weight'] = bad
        with pytest.raises(ValueError, match='finite and > 0'):
            edge_betweenness_centrality(H, weight='weight')
    for bad in ('cost', 1, lambda u, v, d: 1):
        with pytest.raises(NotImplementedError, match="weight='weight'"):
            edge_betweenness_centrality(G, weight=bad)
    for k in (0, 35, 2.5, True):
        with pytest.raises(ValueError, match='k must be'):
            edge_betweenness_centrality(G, k=k)
    with pytest.raises(TypeError, match='seed'):
        edge_betweenness_centrality(G, k=3, seed=np.random.RandomState(0))
    D = wo.with_weights(nx.gnm_random_graph(30, 90, seed=2, directed=True), 'ints')
    host, out, _ = NetworkxInterface(D)._device_graph()
    monkeypatch.setattr(NetworkxInterface, '_device_graph', lambda self: (host, out, None))
    for weight in (None, 'weight'):
        with pytest.raises(NotImplementedError, match='in-adjacency'):
            edge_betweenness_centrality(D, weight=weight)
    assert cpu_backend.calls == []


def test_igraph_parallel_edges_are_refused(cpu_backend):
    from graphrole_amd import edge_betweenness_centrality
    from tests.test_igraph_adapter_cpu import _pair, _random_multigraph
    edges = _random_multigraph(np.random.default_rng(3), 40, 160, False, True, True)
    ig, _ = _pair(40, edges, False)
    with pytest.raises(NotImplementedError, match='parallel edges'):
        edge_betweenness_centrality(ig)
    assert cpu_backend.calls == []


# ---------------------------------------------------------------------------------------------------------- ABI
def test_public_names_and_catalogue():
    import graphrole_amd
    from graphrole_amd import kernels, measures
    assert graphrole_amd.edge_betweenness_centrality is measures.edge_betweenness_centrality
    assert callable(kernels.edge_betweenness) and callable(kernels.weighted_edge_betweenness)
    assert 'edge_betweenness_centrality' not in measures.CATALOGUE and len(measures.CATALOGUE) == 16
    assert 'without passing `k`' in measures.edge_betweenness_centrality.__doc__


def _header_arguments(header: str, name: str) -> int:
    declaration = re.search(r'^(?:int|size_t)\s+' + name + r'\s*\(([^;]*?)\)\s*;', header, re.S | re.M).group(1)
    return len([a for a in declaration.split(',') if a.strip()])


def test_ctypes_signatures_header_and_caps():
    from graphrole_amd import _lib
    from graphrole_amd import kernels as K
    header = open(os.path.join(ROOT, 'include', 'grx.h')).read()
    names = ('grx_edge_betweenness', 'grx_edge_betweenness_workspace_bytes', 'grx_weighted_edge_betweenness',
             'grx_weighted_edge_betweenness_workspace_bytes')
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(_lib._SIGNATURES[name][1]) == _header_arguments(header, name)
    # the arguments of the node entry points without `endpoints`
    assert len(_lib._SIGNATURES['grx_edge_betweenness'][1]) == len(_lib._SIGNATURES['grx_betweenness'][1]) - 1 == 19
    assert (len(_lib._SIGNATURES['grx_weighted_edge_betweenness'][1]) ==
            len(_lib._SIGNATURES['grx_weighted_betweenness'][1]) - 1 == 23)
    assert '#define GRX_VERSION 1100' in header
    for restated in ('edge_betweenness_centrality', '_accumulate_edges', '_rescale_e'):
        assert restated in header
    csrc = os.path.join(ROOT, 'graphrole_amd', 'csrc')
    shared = open(os.path.join(csrc, 'grx_edge_sum.h')).read()
    assert '#pragma clang fp contract(off)' in shared
    brandes = open(os.path.join(csrc, 'grx_brandes.h')).read()   # what both files include grx_edge_sum.h through
    assert '#include "grx_edge_sum.h"' in brandes and '#pragma clang fp contract(off)' in brandes
    assert 'atomicAdd(&ebc' not in brandes and 'unsafeAtomicAdd' not in brandes
    for name in ('grx_betweenness.hip', 'grx_weighted_betweenness.hip'):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "grx_brandes.h"' in text and '#pragma clang fp contract(off)' in text
        assert 'atomicAdd(&ebc' not in text and 'unsafeAtomicAdd' not in text
    makefile = open(os.path.join(csrc, 'Makefile')).read()
    assert 'grx_edge_sum.h' in makefile and 'grx_brandes.h' in makefile
    # the caps the second-trip test sizes itself by are the ones in the sources
    for text, constant in ((shared, 'EB_BLOCK'), (shared, 'EB_ROW_LANES'), (shared, 'EB_MAX_ROW_BLOCKS'),
                           (open(os.path.join(csrc, 'grx_betweenness.hip')).read(), 'BW_BLOCK'),
                           (open(os.path.join(csrc, 'grx_betweenness.hip')).read(), 'BW_MAX_ROW_BLOCKS')):
        found = re.findall(r'\b' + constant + r' = (\d+);', text)
        assert len(found) == 1 and int(found[0]) == getattr(K, constant), constant
    assert 'grx_grid(n, EB_BLOCK / EB_ROW_LANES, EB_MAX_ROW_BLOCKS)' in shared
    assert 'grx_grid(n, BW_WAVES, BW_MAX_ROW_BLOCKS)' in open(os.path.join(csrc, 'grx_betweenness.hip')).read()


def test_argument_validation_needs_no_device():
    """GRX_REQUIRE runs before any HIP call; the batch choice of the new entry points counts the kept coeff array."""
    from graphrole_amd import _lib
    lib = _lib.load()
    size, node = lib.grx_edge_betweenness_workspace_bytes, lib.grx_betweenness_workspace_bytes
    assert size(10, 64, 70) >= 28 * 64 * 10 and size(10, 64, 70) - node(10, 64, 70) >= 8 * 64 * 10
    assert size(10, 0, 70) == size(10, 128, 70) and size(10, 0, 3) == size(10, 64, 3)
    n = 700_000                                                 # 4 GiB / 20 n = 306 -> 256 lanes; / 28 n = 219 -> 192
    assert node(n, 0, 1 << 20) == node(n, 256, 1) and size(n, 0, 1 << 20) == size(n, 192, 1)
    wsize, wnode = lib.grx_weighted_edge_betweenness_workspace_bytes, lib.grx_weighted_betweenness_workspace_bytes
    assert wsize(10, 16, 70) >= 36 * 16 * 10 + 4 * 10 and wsize(10, 64, 70) - wnode(10, 64, 70) >= 8 * 64 * 10
    assert wsize(10, 0, 70) == wsize(10, 64, 70) and wsize(10, 0, 3) == wsize(10, 16, 3)
    n = 2_000_000                                               # 28 n 64 = 3.6 GB fits 4 GiB, 36 n 64 = 4.6 GB does not
    assert wnode(n, 0, 1 << 20) == wnode(n, 64, 1) and wsize(n, 0, 1 << 20) == wsize(n, 32, 1)
    p = ctypes.c_void_p(4096)                                   # never dereferenced: every call fails validation
    unweighted = lambda **kw: lib.grx_edge_betweenness(                                           # noqa: E731
        kw.get('n', 10), p, p, None, 0, kw.get('lanes', 4), None, None, None, 0, 0, kw.get('src', p), kw.get('k', 3),
        1.0, kw.get('batch', 0), kw.get('out', p), p, kw.get('ws', 1 << 30), None)
    weighted = lambda **kw: lib.grx_weighted_edge_betweenness(                                    # noqa: E731
        kw.get('n', 10), p, p, None, None, 0, kw.get('lanes', 4), None, None, None, None, 0, 0, kw.get('src', p),
        kw.get('k', 3), 1.0, kw.get('batch', 0), kw.get('out', p), None, None, p, kw.get('ws', 1 << 30), None)
    for call, name, bad_batch in ((unweighted, 'grx_edge_betweenness', 32), (weighted, 'grx_weighted_edge_betweenness', 8)):
        for kw, message in ((dict(n=0), 'out of range'), (dict(batch=bad_batch), 'batch must be'),
                            (dict(src=None), 'source list'), (dict(out=None), 'null pointer'),
                            (dict(lanes=0), 'lanes_per_row'), (dict(ws=16), 'workspace')):
            assert call(**kw) == -1, (name, kw)
            text = lib.grx_last_error().decode()
            assert text.startswith(name + ':') and message in text, (name, kw, text)
