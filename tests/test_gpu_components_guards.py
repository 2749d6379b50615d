"""
-m gpu: grx_components and grx_reachable between guard bands and on poisoned memory, run exactly as
tests/test_gpu_guard_bands.py runs a scenario: A without poison, B with every allocation of kernels.py -- the labels, the
sizes, the flags and the workspace with the colours, stamps and control words -- filled with 0xFF first; every guard
intact in both, A == B byte for byte, B equal to the oracle (tests/components_oracle.py), the entry point among those
reached.  A fault signature ends the run there, as in that file.

The two scenarios are registered with tests/guard_scenarios when this module is imported, which pytest does while it
collects: that is also what tests/test_guarded_alloc_cpu.py::test_every_device_entry_point_has_a_scenario sees.

  components/modes      connected, weak and strong, with and without d_size, with 4 and 32 lanes (the hub launch and the
                        lane-group launch), on hub cases (the hub on cycles, trimmed by its short row, and trimmed in
                        round 2 by its long out-row resp. in-row) and the motif of tests/components_oracle.py, a chain of
                        two-cycles (several outer iterations) and graphs of 1 and 63 rows -- never a multiple of the block.
  components/reachable  grx_reachable over the out- and the in-adjacency of the same graphs: no seed, every row a seed, a
                        seed on the hub.
"""
import numpy as np
import pytest

from tests import components_oracle as co, guard_scenarios as gs, test_gpu_guard_bands as bands

pytestmark = pytest.mark.gpu

NAMES = ('components/modes', 'components/reachable')
MODES = (co.CONNECTED, co.WEAK, co.STRONG)


def _graphs():
    out = {kind: co.hub_case(kind) for kind in ('scc_out', 'sink_in', 'sink_out', 'source_in')}
    out['motif'] = co.motif()
    out['chain'] = co.two_cycle_chain(5)
    out['n1'] = (np.arange(2, dtype=np.int64), np.zeros(1, dtype=np.int64))     # one row with a self-loop
    out['cycle63'] = co.cycle(63)
    return out


def _for_mode(row_ptr, col, mode):
    if mode != co.CONNECTED:
        return row_ptr, col
    src, dst = co.arcs_of(row_ptr, col)
    return co.symmetric_csr(len(row_ptr) - 1, np.stack([src, dst], axis=1))


def _run_modes(K):
    out = {}
    for name, (row_ptr, col) in _graphs().items():
        n = len(row_ptr) - 1
        for mode in MODES:
            rp, c = _for_mode(row_ptr, col, mode)
            csr = K.DeviceCSR(rp, c)
            tr = K.DeviceCSR(*co.transpose(rp, c)) if mode == co.STRONG else None
            for lanes in gs.LANES:
                tag = f'{name}/{mode}/L{lanes}'
                label, size, count, rounds = K.components(csr, tr, mode=mode, lanes=lanes)
                out[f'{tag}/label'], out[f'{tag}/size'] = gs.host(K, label, n), gs.host(K, size, n)
                out[f'{tag}/info'] = np.array([count, rounds])
                label, size, count, rounds = K.components(csr, tr, mode=mode, want_size=False, lanes=lanes)
                assert size is None
                out[f'{tag}/label_only'], out[f'{tag}/info_only'] = gs.host(K, label, n), np.array([count, rounds])
    return out


def _want_modes():
    want = {}
    for name, (row_ptr, col) in _graphs().items():
        for mode in MODES:
            r = co.components(*_for_mode(row_ptr, col, mode), mode)
            for lanes in gs.LANES:
                tag = f'{name}/{mode}/L{lanes}'
                want[f'{tag}/label'], want[f'{tag}/size'] = r.label, r.size
                want[f'{tag}/label_only'] = r.label
                want[f'{tag}/info'] = want[f'{tag}/info_only'] = np.array([r.n_components, r.rounds])
    return gs.exact(want)


def _seeds(n):
    hub = np.zeros(n, dtype=np.int32)
    hub[0] = 9
    return {'none': np.zeros(n, dtype=np.int32), 'every': np.ones(n, dtype=np.int32), 'hub': hub}


def _run_reachable(K):
    out = {}
    for name, (row_ptr, col) in _graphs().items():
        n = len(row_ptr) - 1
        for side, a in (('out', (row_ptr, col)), ('in', co.transpose(row_ptr, col))):
            csr = K.DeviceCSR(*a)
            for seeds, flag in _seeds(n).items():
                for lanes in gs.LANES:
                    tag = f'{name}/{side}/{seeds}/L{lanes}'
                    got, count, levels = K.reachable(csr, flag, lanes=lanes)
                    out[f'{tag}/flag'], out[f'{tag}/info'] = gs.host(K, got, n), np.array([count, levels])
    return out


def _want_reachable():
    want = {}
    for name, (row_ptr, col) in _graphs().items():
        n = len(row_ptr) - 1
        for side, a in (('out', (row_ptr, col)), ('in', co.transpose(row_ptr, col))):
            for seeds, flag in _seeds(n).items():
                got, count, levels = co.reachable(*a, flag)
                for lanes in gs.LANES:
                    tag = f'{name}/{side}/{seeds}/L{lanes}'
                    want[f'{tag}/flag'], want[f'{tag}/info'] = got, np.array([count, levels])
    return gs.exact(want)


if not any(s.name in NAMES for s in gs.SCENARIOS):
    gs.scenario(NAMES[0], ('grx_components',), want=_want_modes)(_run_modes)
    gs.scenario(NAMES[1], ('grx_reachable',), want=_want_reachable)(_run_reachable)


@pytest.fixture(scope='module')
def K():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from graphrole_amd import kernels
    return kernels


@pytest.mark.parametrize('name', NAMES)
def test_guards_and_poison(K, name):
    scenario = next(s for s in gs.SCENARIOS if s.name == name)
    assert scenario.repeatable and scenario.want is not None
    assert {'components/modes': 'grx_components', 'components/reachable': 'grx_reachable'}[name] in scenario.covers
    bands.test_guards_and_poison(K, name)
