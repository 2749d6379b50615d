"""
-m gpu: grx_triad_census between guard bands and on poisoned memory, run exactly as tests/test_gpu_guard_bands.py runs a
scenario: A without poison, B with every allocation of kernels.py -- the 16 columns, the totals, the per-arc counts and
the workspace with the neighbour classes, the two counters, the pair counts, the arc rows and the common neighbours --
filled with 0xFF first; every guard intact in both, A == B byte for byte, B equal to the oracle
(tests/triad_oracle.py).  A fault signature ends the run there, as in that file.

The scenario is registered with tests/guard_scenarios when this module is imported, which pytest does while it collects:
that is also what tests/test_guarded_alloc_cpu.py::test_every_device_entry_point_has_a_scenario sees.

  triad_census  'hub_isolated', the smallest shape that takes every kernel of the entry point -- a hub with 200 spokes
                in the classes O, I and M in turn (one hub row at 4 lanes per row, none at 32), a directed ring with
                some mutual pairs and chords through the spokes' ends (closed triads with and without the hub), a
                mutual triangle and one isolated node -- with and without the two optional outputs.
"""
import functools

import networkx as nx
import numpy as np
import pytest

from tests import guard_scenarios as gs, test_gpu_guard_bands as bands
from tests import triad_oracle as to

pytestmark = pytest.mark.gpu

NAME = 'triad_census'
COVERS = ('grx_triad_census',)


@functools.lru_cache(maxsize=None)
def _arrays():
    D = nx.DiGraph()
    for k in range(200):
        v = 1 + k
        if k % 3 != 1:
            D.add_edge(0, v)
        if k % 3 != 0:
            D.add_edge(v, 0)
        D.add_edge(v, 1 + (k + 1) % 200)
        if k % 5 == 0:
            D.add_edge(1 + (k + 1) % 200, v)
        if k % 4 == 0:
            D.add_edge(1 + (k + 2) % 200, v)
    D.add_edges_from((a, b) for a in (201, 202, 203) for b in (201, 202, 203) if a != b)       # the one 300
    D.add_edge(203, 5)
    D.add_node(204)
    _, row_ptr, col, codes = to.graph_arrays(D)
    return row_ptr, col, codes


def _run(K):
    row_ptr, col, codes = _arrays()
    n, nnz = len(row_ptr) - 1, len(col)
    out = {}
    for L in gs.LANES:
        csr = gs.with_lanes(K, K.DeviceCSR(row_ptr, col), L)
        assert (csr.n_hubs == 1) == (L == 4)
        columns, totals, arc = K.triad_census(csr, K.to_device(codes), want_totals=True, want_arc_triads=True, lanes=L)
        out[f'L{L}/columns'], out[f'L{L}/totals'] = gs.host(K, columns, None, n), gs.host(K, totals, 16)
        out[f'L{L}/common'] = gs.host(K, arc, nnz)
        out[f'L{L}/columns_only'] = gs.host(K, K.triad_census(csr, K.to_device(codes), want_totals=False, lanes=L)[0],
                                            None, n)
    return out


def _want():
    row_ptr, col, codes = _arrays()
    c = to.census(row_ptr, col, codes)
    assert np.all(c.totals > 0) and c.columns[3:, -1].sum() == 0           # every type; the isolated node
    want = {}
    for L in gs.LANES:
        want[f'L{L}/columns'] = want[f'L{L}/columns_only'] = (c.columns, gs.EXACT)
        want[f'L{L}/totals'] = (c.totals, gs.EXACT)
        want[f'L{L}/common'] = (c.common, gs.EXACT)
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
