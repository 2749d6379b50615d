"""
-m gpu: grx_edge_betweenness and grx_weighted_edge_betweenness between guard bands and on poisoned memory, run exactly as
tests/test_gpu_guard_bands.py runs a scenario: A without poison, B with every allocation of kernels.py -- the per-arc
output and the workspace with level / depth, sigma, delta, the kept coeff array, the distances and the control words --
filled with 0xFF (NaN as fp64) first; every guard intact in both, A == B byte for byte, B equal to the oracle
(tests/edge_betweenness_oracle.py) within its one tolerance, both entry points among those reached.  A fault signature
ends the run there, as in that file.

The scenario is registered with tests/guard_scenarios when this module is imported, which pytest does while it collects:
that is also what tests/test_guarded_alloc_cpu.py::test_every_device_entry_point_has_a_scenario sees.

  edge_betweenness  'hub_isolated', the smallest shape that takes every kernel of the two entry points -- a star of 200
                    leaves (one hub row at 4 lanes per row, none at 32), a cycle through the leaves (several levels,
                    ties), one isolated node and one self-loop, integer weights -- and the directed dw300 of
                    tests/guard_scenarios.py, each with 70 sources: a partial last batch at every width.
"""
import functools

import numpy as np
import pytest

from tests import edge_betweenness_oracle as eo, guard_scenarios as gs, test_gpu_guard_bands as bands
from tests import weighted_betweenness_oracle as wo

pytestmark = pytest.mark.gpu

NAME = 'edge_betweenness'
COVERS = ('grx_edge_betweenness', 'grx_weighted_edge_betweenness')


@functools.lru_cache(maxsize=None)
def _graphs():
    """name -> (out CSR, in CSR or None, directed), each CSR (row_ptr, col, w)."""
    import networkx as nx
    G = nx.star_graph(200)
    G.add_edges_from((v, v % 200 + 1) for v in range(1, 201))
    G.add_edge(7, 7)
    G.add_node(201)
    G = wo.with_weights(G, 'ints', seed=3)
    _, o, _ = wo.csr_pair(G)
    _, do, di = wo.csr_pair(gs.dw300())
    return {'hub_isolated': (o, None, False), 'dw300': (do, di, True)}


def _sources(n):
    return np.random.default_rng(11).permutation(n)[:70]


def _run(K):
    out = {}
    for name, (o, i, directed) in _graphs().items():
        n, nnz = len(o[0]) - 1, len(o[1])
        sources = _sources(n)
        for L in gs.LANES:
            d_out, d_in = gs._dev_pair(K, o, i, False, L)
            assert name != 'hub_isolated' or (d_out.n_hubs == 1) == (L == 4)
            out[f'{name}/L{L}/ebc'] = gs.host(K, K.edge_betweenness(d_out, d_in, sources, 0.5, batch=64), nnz)
            w_out, w_in = gs._dev_pair(K, o, i, True, L)
            ebc, rounds, levels = K.weighted_edge_betweenness(w_out, w_in, sources, 0.25, 16)
            out[f'{name}/L{L}/webc'], out[f'{name}/L{L}/webc_info'] = gs.host(K, ebc, nnz), np.array([rounds, levels])
    return out


def _both_slots(o, arc, directed, scale):
    """The kernel leaves the value of an undirected edge in both of its arc slots."""
    n = len(o[0]) - 1
    u = np.repeat(np.arange(n, dtype=np.int64), np.diff(o[0]))
    col = np.asarray(o[1], dtype=np.int64)
    if directed:
        return arc * scale
    mirror = np.searchsorted(u * n + col, col * n + u)
    return np.where(u == col, arc, arc + arc[mirror]) * scale


def _want():
    want = {}
    for name, (o, i, directed) in _graphs().items():
        sources = _sources(len(o[0]) - 1)
        inn = o if i is None else i
        hops = _both_slots(o, eo.arc_sums(o[0], o[1], sources), directed, 0.5)
        arc, levels = eo.weighted_arc_sums(o, inn, sources)
        rounds = wo.relaxation_rounds(inn, sources, 16)
        assert np.count_nonzero(hops) > 0 and np.count_nonzero(arc) > 0 and levels > 2
        for L in gs.LANES:
            want[f'{name}/L{L}/ebc'] = (hops, (eo.RTOL, 0.0))
            want[f'{name}/L{L}/webc'] = (_both_slots(o, arc, directed, 0.25), (eo.RTOL, 0.0))
            want[f'{name}/L{L}/webc_info'] = (np.array([rounds, levels]), gs.EXACT)
    return want


if not any(s.name == NAME for s in gs.SCENARIOS):
    gs.scenario(NAME, COVERS, want=_want)(_run)


@pytest.fixture(scope='module')
def K():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from graphrole_amd import kernels
    return kernels


def test_guards_and_poison(K):
    scenario = next(s for s in gs.SCENARIOS if s.name == NAME)
    assert scenario.repeatable and scenario.want is not None and set(COVERS) <= set(scenario.covers)
    bands.test_guards_and_poison(K, NAME)
