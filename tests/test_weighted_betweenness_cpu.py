"""
-m "not gpu": betweenness centrality over shortest paths by weight without a device.
tests/weighted_betweenness_oracle.py (the numpy restatement of grx_weighted_betweenness) against
nx.betweenness_centrality(G, weight='weight', ...) on every graph kind and option; then the Python layer --
weighted_betweenness_centrality and node_measures(betweenness_weight='weight') -- over a CPU double of
kernels.weighted_betweenness (the oracle on the double's CSR arrays): the CSRs and weights passed down, the sources and
their order, the scale, the attrs, the refusals, and every table without the keyword left as it was; then the C ABI.
The device numbers are pinned in tests/test_gpu_weighted_betweenness.py.
"""
import ctypes
import os
import random
import re
import types

import networkx as nx
import numpy as np
import pytest

from tests import betweenness_oracle as bo
from tests import fake_kernels
from tests import sssp_oracle as so
from tests import weighted_betweenness_oracle as wo
from tests.test_betweenness_cpu import OPTIONS, _fresh, _internal_ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _directed_loops_isolated():
    G = nx.gnm_random_graph(120, 400, seed=7, directed=True)
    G.add_edges_from([(3, 3), (10, 10)])
    G.add_nodes_from([500, 501])
    return wo.with_weights(G, 'ints', seed=3)


def _disconnected():
    G = nx.disjoint_union(nx.barabasi_albert_graph(60, 2, seed=1), nx.cycle_graph(9))
    G.add_nodes_from([1000, 1001])
    return wo.with_weights(G, 'ints', seed=4)


GRAPHS = {
    'karate': nx.karate_club_graph,                              # its own integer weights
    'er300_ints': lambda: wo.with_weights(nx.gnm_random_graph(300, 1200, seed=1), 'ints', seed=1),
    'ba300_dyadic': lambda: wo.with_weights(nx.barabasi_albert_graph(300, 3, seed=2), 'dyadic', seed=2),
    'directed_loops_isolated': _directed_loops_isolated,
    'disconnected': _disconnected,
    'strings': lambda: wo.with_weights(nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
                                       'uniform', seed=5),
    'path40': lambda: wo.with_weights(nx.path_graph(40), 'uniform', seed=6),
    'detour': so.detour_graph,
    'uneven_ties': wo.uneven_ties_graph,
    'n1': lambda: nx.empty_graph(1),
    'n2': lambda: wo.with_weights(nx.path_graph(2), 'uniform', seed=7),
    'n3': lambda: wo.with_weights(nx.path_graph(3), 'ints', seed=8),
}
TIED = ('karate', 'er300_ints', 'ba300_dyadic', 'directed_loops_isolated', 'disconnected', 'uneven_ties')


def _close(got: dict, want: dict):
    keys = list(want)
    assert set(got) == set(keys)
    np.testing.assert_allclose([got[v] for v in keys], [want[v] for v in keys], rtol=wo.RTOL, atol=0)


# ------------------------------------------------------------------------------------------ oracle against networkx
@pytest.mark.parametrize('opts', OPTIONS, ids=[str(i) for i in range(len(OPTIONS))])
@pytest.mark.parametrize('key', list(GRAPHS))
def test_oracle_matches_networkx(key, opts):
    G = GRAPHS[key]()
    if opts.get('k', 0) > G.number_of_nodes():
        opts = dict(opts, k=G.number_of_nodes())
    info = {}
    got = wo.betweenness(G, info=info, **_fresh(opts))
    _close(got, nx.betweenness_centrality(G, weight='weight', **_fresh(opts)))
    if key in TIED and 'k' not in opts:
        assert info['max_sigma'] > 1                            # lightest paths do tie: not a tie-free input


def test_oracle_waits_for_the_deepest_predecessor():
    G = wo.uneven_ties_graph()
    labels, out, inn = wo.csr_pair(G)
    dist, _ = so.relax(*inn, [0])
    depth, sigma, _, levels = wo.single_source(wo._arcs(out, None), wo._arcs(inn, None), dist[0], 0)
    assert dist[0][1] == 2.0 and depth[1] == 2 and sigma[1] == 2.0      # 0 - 1 and 0 - 2 - 1, depth of the longer
    assert depth[2] == 1 and depth[3] == 3 and sigma[3] == 2.0 and levels == depth.max()


def test_oracle_detour_depth_against_bfs_level():
    G = so.detour_graph()
    labels, out, inn = wo.csr_pair(G)
    bc, rounds, levels = wo.betweenness_arrays(out, inn, [0], False, 1.0)
    assert levels == 4 and rounds == 5                          # node 4 is one hop away and four arcs deep
    assert bc.tolist() == [0.0, 3.0, 2.0, 1.0, 0.0]
    _, out, inn = wo.csr_pair(G, weight=None)
    assert wo.betweenness_arrays(out, inn, [0], False, 1.0)[2] == 2


def test_oracle_hub_order_and_batch_width_change_no_bits():
    G = GRAPHS['ba300_dyadic']()
    labels, out, inn = wo.csr_pair(G)
    sources = np.random.default_rng(1).permutation(300)[:70]
    plain, rounds16, levels = wo.betweenness_arrays(out, inn, sources, True, 0.5, batch=16)
    wide, rounds64, levels64 = wo.betweenness_arrays(out, inn, sources, True, 0.5, batch=64)
    assert plain.tobytes() == wide.tobytes() and levels == levels64 and rounds16 >= rounds64
    hubs, _, _ = wo.betweenness_arrays(out, inn, sources, True, 0.5, hub_degree_out=8, hub_degree_in=8)
    np.testing.assert_allclose(hubs, plain, rtol=wo.RTOL, atol=0)


def test_unit_weights_are_the_unweighted_oracle():
    G = nx.gnm_random_graph(120, 400, seed=7, directed=True)
    _close(wo.betweenness(G), bo.betweenness(G))
    _close(wo.betweenness(G, weight=None, endpoints=True), nx.betweenness_centrality(G, endpoints=True))


# ------------------------------------------------------------------------------------------ Python layer, CPU double
@pytest.fixture
def cpu_backend():
    import torch
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.calls = []
    double.unweighted = []

    def arrays(csr):
        w = np.ones(len(csr.col)) if csr.w is None else np.asarray(csr.w, dtype=np.float64)
        return np.asarray(csr.row_ptr, dtype=np.int64), np.asarray(csr.col, dtype=np.int64), w

    def weighted_betweenness(csr_out, csr_in, sources, endpoints, scale, batch=0):
        sources = np.asarray(sources, dtype=np.int64)
        double.calls.append(dict(sources=sources.copy(), endpoints=endpoints, scale=scale, out=csr_out, inn=csr_in,
                                 batch=batch))
        out = arrays(csr_out)
        bc, rounds, levels = wo.betweenness_arrays(out, out if csr_in is None else arrays(csr_in), sources, endpoints,
                                                   scale, batch)
        return torch.from_numpy(bc), rounds, levels

    def betweenness(csr_out, csr_in, sources, endpoints, scale, batch=0):
        sources = np.asarray(sources, dtype=np.int64)
        double.unweighted.append(dict(sources=sources.copy(), scale=scale))
        bc = bo.betweenness_arrays(csr_out.row_ptr, csr_out.col, sources, True, normalized=False, endpoints=endpoints)
        return torch.from_numpy(bc * scale)

    double.weighted_betweenness = weighted_betweenness
    double.betweenness = betweenness
    backend.use(double)
    yield double
    backend.use(None)


def _series(series, want: dict):
    assert series.dtype == np.float64 and list(series.index) == sorted(want)
    assert series.name == 'betweenness_centrality'
    np.testing.assert_allclose(series.to_numpy(), [want[v] for v in series.index], rtol=wo.RTOL, atol=0)


@pytest.mark.parametrize('directed', [False, True])
def test_csrs_weights_sources_scale_and_attrs(cpu_backend, directed):
    from graphrole_amd import weighted_betweenness_centrality
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    G = wo.with_weights(nx.gnm_random_graph(50, 260, seed=3, directed=directed), 'ints', seed=2)
    H = type(G)()
    H.add_nodes_from(random.Random(0).sample(list(G), 50))       # graph order differs from label order
    H.add_edges_from(G.edges(data=True))
    bc = weighted_betweenness_centrality(H)
    (call,) = cpu_backend.calls
    assert cpu_backend.unweighted == []
    _, out, tr = NetworkxInterface(H)._device_graph()
    assert np.array_equal(call['out'].row_ptr, out.row_ptr) and np.array_equal(call['out'].col, out.col)
    assert np.array_equal(call['out'].w, out.w) and set(np.unique(out.w)) <= {1.0, 2.0, 3.0, 4.0, 5.0}
    if directed:                                                # relaxation and forward pass pull over the in-adjacency
        assert np.array_equal(call['inn'].row_ptr, tr.row_ptr) and np.array_equal(call['inn'].col, tr.col)
        assert np.array_equal(call['inn'].w, tr.w)
    else:
        assert call['inn'] is None
    assert np.array_equal(call['sources'], _internal_ids(H, list(H)))
    assert call['scale'] == 1 / (49 * 48) and call['endpoints'] is False and call['batch'] == 0
    _series(bc, nx.betweenness_centrality(H, weight='weight'))
    labels, o, i = wo.csr_pair(H)
    _, rounds, levels = wo.betweenness_arrays(o, i, list(range(50)), False, 1.0)
    assert bc.attrs['levels'] == levels >= 2 and bc.attrs['rounds'] == rounds >= 3     # one batch: any source order
    assert isinstance(bc.attrs['rounds'], int) and set(bc.attrs) == {'rounds', 'levels'}


@pytest.mark.parametrize('seed_kind', ['int', 'random'])
def test_sampled_sources_follow_networkx(cpu_backend, seed_kind):
    from graphrole_amd import weighted_betweenness_centrality
    G = wo.with_weights(nx.relabel_nodes(nx.barabasi_albert_graph(80, 2, seed=5), lambda v: f'v{v}'), 'dyadic', seed=1)
    make = (lambda: 17) if seed_kind == 'int' else (lambda: random.Random(17))
    bc = weighted_betweenness_centrality(G, k=9, seed=make(), endpoints=True, normalized=False)
    expected = random.Random(17).sample(list(G.nodes()), 9)
    (call,) = cpu_backend.calls
    assert np.array_equal(call['sources'], _internal_ids(G, expected))
    assert call['scale'] == 0.5 * 80 / 9 and call['endpoints'] is True
    _series(bc, nx.betweenness_centrality(G, k=9, seed=make(), weight='weight', endpoints=True, normalized=False))


@pytest.mark.parametrize('n,directed,normalized,endpoints,k', [
    (30, False, True, False, None), (30, True, True, False, None), (30, False, False, False, None),
    (30, True, False, True, 4), (2, False, True, False, None), (1, False, True, True, None),
    (30, False, True, False, 6),
])
def test_scale_is_rescale(cpu_backend, n, directed, normalized, endpoints, k):
    from graphrole_amd import weighted_betweenness_centrality
    G = wo.with_weights(nx.gnm_random_graph(n, 2 * n, seed=1, directed=directed), 'ints')
    weighted_betweenness_centrality(G, k=k, normalized=normalized, endpoints=endpoints, seed=0)
    want = bo.rescale_factor(n, normalized, directed, k, endpoints)
    assert cpu_backend.calls[-1]['scale'] == (1.0 if want is None else want)
    assert (cpu_backend.calls[-1]['inn'] is not None) == directed


def test_weight_none_delegates_to_the_unweighted_kernel(cpu_backend):
    from graphrole_amd import betweenness_centrality, weighted_betweenness_centrality
    G = nx.karate_club_graph()
    got = weighted_betweenness_centrality(G, weight=None, k=10, seed=2)
    assert cpu_backend.calls == [] and len(cpu_backend.unweighted) == 1
    assert got.equals(betweenness_centrality(G, k=10, seed=2))
    _series(got, nx.betweenness_centrality(G, k=10, seed=2))


def test_node_measures_keyword(cpu_backend):
    from graphrole_amd import node_measures, weighted_betweenness_centrality
    G = nx.karate_club_graph()
    opts = dict(k=12, seed=5, normalized=False, endpoints=True)
    M = node_measures(G, ['weighted_degree', 'betweenness_centrality'], betweenness_weight='weight', **opts)
    assert list(M.columns) == ['weighted_degree', 'betweenness_centrality'] and len(cpu_backend.calls) == 1
    assert cpu_backend.unweighted == []
    own = weighted_betweenness_centrality(G, **opts)
    assert M['betweenness_centrality'].to_numpy().tobytes() == own.to_numpy().tobytes()
    assert M.attrs['weighted_betweenness'] == own.attrs
    _series(own, nx.betweenness_centrality(G, weight='weight', **opts))
    # the keyword touches that column only, and without it every table is what it was
    calls = len(cpu_backend.calls)
    plain = node_measures(G, ['weighted_degree', 'betweenness_centrality'], **opts)
    assert len(cpu_backend.calls) == calls and len(cpu_backend.unweighted) == 1
    assert 'weighted_betweenness' not in plain.attrs
    _series(plain['betweenness_centrality'], nx.betweenness_centrality(G, **opts))
    assert plain.equals(node_measures(G, ['weighted_degree', 'betweenness_centrality'], betweenness_weight=None, **opts))
    assert not np.array_equal(plain['betweenness_centrality'].to_numpy(), own.to_numpy())
    assert node_measures(G, ['weighted_degree'], betweenness_weight='weight').equals(node_measures(G, ['weighted_degree']))
    assert len(cpu_backend.calls) == calls


def test_missing_attribute_counts_one(cpu_backend):
    from graphrole_amd import betweenness_centrality, weighted_betweenness_centrality
    G = wo.with_weights(nx.karate_club_graph(), 'dyadic', seed=8)
    del G[0][1]['weight']
    _series(weighted_betweenness_centrality(G), nx.betweenness_centrality(G, weight='weight'))
    U = nx.karate_club_graph()
    for u, v in U.edges():
        del U[u][v]['weight']
    got = weighted_betweenness_centrality(U)                    # no attribute anywhere: hop counts
    np.testing.assert_allclose(got.to_numpy(), betweenness_centrality(U).to_numpy(), rtol=wo.RTOL, atol=0)


def test_csr_graph_input(cpu_backend):
    from graphrole_amd import weighted_betweenness_centrality
    from graphrole_amd.graph.csr import CSRGraph
    G = wo.with_weights(nx.barabasi_albert_graph(60, 3, seed=8), 'ints', seed=1)
    src, dst = np.array(list(G.edges)).T
    w = np.array([G[u][v]['weight'] for u, v in G.edges], dtype=np.float64)
    _series(weighted_betweenness_centrality(CSRGraph(60, src, dst, w)), nx.betweenness_centrality(G, weight='weight'))


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals_before_any_device_work(cpu_backend):
    from graphrole_amd import node_measures, weighted_betweenness_centrality
    from graphrole_amd.graph.csr import CSRGraph
    G = nx.karate_club_graph()
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        H = G.copy()
        H[0][1]['weight'] = bad
        with pytest.raises(ValueError, match='finite and > 0'):
            weighted_betweenness_centrality(H)
        with pytest.raises(ValueError, match='finite and > 0'):
            node_measures(H, ['betweenness_centrality'], betweenness_weight='weight')
        node_measures(H, ['weighted_degree'], betweenness_weight='weight')   # no such column: the weights are not looked at
    with pytest.raises(ValueError, match='finite and > 0'):
        weighted_betweenness_centrality(so.with_weights(nx.path_graph(30), 'mixed', seed=1))     # MIXED holds 0.0
    with pytest.raises(ValueError, match='finite and > 0'):
        weighted_betweenness_centrality(CSRGraph(3, np.array([0, 1]), np.array([1, 2]), np.array([1.0, 0.0])))
    for multi in (nx.MultiGraph([(0, 1), (0, 1), (1, 2)]), nx.MultiDiGraph([(0, 1), (1, 0)])):
        with pytest.raises(NotImplementedError, match='parallel edges'):
            weighted_betweenness_centrality(multi)
        with pytest.raises(NotImplementedError, match='parallel edges'):
            node_measures(multi, ['betweenness_centrality'], betweenness_weight='weight')
    for bad in ('cost', 1, lambda u, v, d: 1):
        with pytest.raises(NotImplementedError, match="weight='weight'"):
            weighted_betweenness_centrality(G, weight=bad)
        with pytest.raises(NotImplementedError, match="weight='weight'"):
            node_measures(G, ['betweenness_centrality'], betweenness_weight=bad)
    for k in (0, 35):
        with pytest.raises(ValueError, match='k must be'):
            weighted_betweenness_centrality(G, k=k)
    with pytest.raises(TypeError, match='seed'):
        weighted_betweenness_centrality(G, k=3, seed=np.random.RandomState(0))
    assert cpu_backend.calls == [] and cpu_backend.unweighted == []


def test_igraph_parallel_edges_are_refused(cpu_backend):
    from graphrole_amd import weighted_betweenness_centrality
    from tests.test_igraph_adapter_cpu import _pair, _random_multigraph
    edges = _random_multigraph(np.random.default_rng(3), 40, 160, False, True, True)
    ig, _ = _pair(40, edges, False)
    with pytest.raises(NotImplementedError, match='parallel edges'):
        weighted_betweenness_centrality(ig)
    assert cpu_backend.calls == []


def test_directed_graph_without_in_adjacency_raises(cpu_backend, monkeypatch):
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    from graphrole_amd.measures import measures_of
    g = NetworkxInterface(wo.with_weights(nx.gnm_random_graph(30, 90, seed=2, directed=True), 'ints'))
    host, out, _ = g._device_graph()
    monkeypatch.setattr(NetworkxInterface, '_device_graph', lambda self: (host, out, None))
    with pytest.raises(NotImplementedError, match='in-adjacency'):
        measures_of(g, ['betweenness_centrality'], betweenness_weight='weight')
    assert cpu_backend.calls == []


def test_unweighted_function_still_refuses_and_names_the_new_one(cpu_backend):
    from graphrole_amd import betweenness_centrality
    with pytest.raises(NotImplementedError, match=r"nx.betweenness_centrality\(G, weight='weight'\)") as info:
        betweenness_centrality(nx.karate_club_graph(), weight='weight')
    assert 'weighted_betweenness_centrality' in str(info.value) and 'use networkx' not in str(info.value)
    assert 'weighted_betweenness_centrality' in betweenness_centrality.__doc__
    assert cpu_backend.calls == [] and cpu_backend.unweighted == []


# ---------------------------------------------------------------------------------------------------------- ABI
def test_public_names_and_catalogue():
    import graphrole_amd
    from graphrole_amd import kernels, measures
    assert graphrole_amd.weighted_betweenness_centrality is measures.weighted_betweenness_centrality
    assert callable(kernels.weighted_betweenness)
    assert list(measures.CATALOGUE)[-1] == 'eccentricity' and len(measures.CATALOGUE) == 16
    assert 'betweenness_centrality' in measures.OPT_IN and len(measures.OPT_IN) == 8


def _header_arguments(header: str, name: str) -> int:
    declaration = re.search(r'^(?:int|size_t)\s+' + name + r'\s*\(([^;]*?)\)\s*;', header, re.S | re.M).group(1)
    return len([a for a in declaration.split(',') if a.strip()])


def test_ctypes_signatures_and_header():
    from graphrole_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'grx.h')).read()
    for name in ('grx_weighted_betweenness', 'grx_weighted_betweenness_workspace_bytes'):
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(_lib._SIGNATURES[name][1]) == _header_arguments(header, name)
    assert len(_lib._SIGNATURES['grx_weighted_betweenness'][1]) == 24
    assert len(_lib._SIGNATURES['grx_weighted_betweenness_workspace_bytes'][1]) == 3
    assert 'finite and > 0' in header                           # the contract on the weights is documented
    assert '#define GRX_VERSION 1100' in header
    source = open(os.path.join(ROOT, 'graphrole_amd', 'csrc', 'grx_weighted_betweenness.hip')).read()
    assert '#pragma clang fp contract(off)' in source and '#include "grx_relax.h"' in source
    assert '#include "grx_brandes.h"' in source
    assert '#include "grx_relax.h"' in open(os.path.join(ROOT, 'graphrole_amd', 'csrc', 'grx_sssp.hip')).read()
    assert 'grx_weighted_betweenness.hip' in open(os.path.join(ROOT, 'graphrole_amd', 'csrc', 'Makefile')).read()


def test_argument_validation_needs_no_device():
    """GRX_REQUIRE runs before any HIP call: batch, n range, source list, in-adjacency, hub lists, workspace, nulls."""
    from graphrole_amd import _lib
    lib = _lib.load()
    size = lib.grx_weighted_betweenness_workspace_bytes
    need = size(10, 16, 70)
    assert need >= 28 * 16 * 10 + 4 * 10
    assert size(10, 64, 70) >= 28 * 64 * 10 + 4 * 10 > size(10, 32, 70) > need
    assert size(10, 0, 70) == size(10, 64, 70)                  # no wider than the source list rounded up ...
    assert size(10, 0, 17) == size(10, 32, 17) and size(10, 0, 3) == need    # ... and never below 16
    assert size(1 << 22, 0, 1 << 22) == size(1 << 22, 32, 1)    # 28 n 64 bytes would be 7 GiB: above the 4 GiB budget
    p = ctypes.c_void_p(4096)                                   # never dereferenced: every call fails validation

    def call(n=10, row_ptr=p, col=p, w=p, hubs=None, n_hubs=0, lanes=8, in_row_ptr=None, in_col=None, in_w=None,
             in_hubs=None, n_in_hubs=0, in_lanes=0, sources=p, n_sources=70, endpoints=0, scale=1.0, batch=16, bc=p,
             rounds=None, levels=None, ws=p, ws_bytes=need):
        return lib.grx_weighted_betweenness(n, row_ptr, col, w, hubs, n_hubs, lanes, in_row_ptr, in_col, in_w, in_hubs,
                                            n_in_hubs, in_lanes, sources, n_sources, endpoints, scale, batch, bc,
                                            rounds, levels, ws, ws_bytes, None)

    for bad in (dict(batch=8), dict(batch=48), dict(batch=128), dict(batch=-16), dict(n=1 << 31), dict(n=0),
                dict(n_sources=-1), dict(ws_bytes=need - 1), dict(batch=64), dict(batch=0), dict(row_ptr=None),
                dict(col=None), dict(bc=None), dict(sources=None), dict(ws=None), dict(lanes=0), dict(n_hubs=2),
                dict(n_hubs=-1), dict(in_row_ptr=p, in_lanes=8), dict(in_row_ptr=p, in_col=p, in_w=p, in_lanes=0),
                dict(in_row_ptr=p, in_col=p, in_w=None, in_lanes=8),
                dict(in_row_ptr=p, in_col=p, in_w=p, in_lanes=8, n_in_hubs=3)):
        assert call(**bad) == -1, bad
        assert b'grx_weighted_betweenness' in lib.grx_last_error(), bad
