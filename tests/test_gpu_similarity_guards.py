"""
-m gpu: grx_similar_rows between guard bands and on poisoned memory, run exactly as tests/test_gpu_guard_bands.py runs a
scenario: A without poison, B with every allocation of kernels.py -- outputs and the workspace with the normalised
copies and the segments' lists -- filled with 0xFF first; every guard intact in both, A == B byte for byte, B equal to
the oracle (tests/similarity_oracle.py), grx_similar_rows among the entry points reached.  A fault signature ends the
run there, as in that file.

The two scenarios are registered with tests/guard_scenarios when this module is imported, which pytest does while it
collects: that is also what tests/test_guarded_alloc_cpu.py::test_every_device_entry_point_has_a_scenario sees.

  similar_rows/short    lists that run out: 70 candidates in two segments of 64 and 6 with k = 64 (the second segment's
                        list, and the first one's where a row is left out, end in the workspace's -1 / NaN padding that
                        the merge must stop at, not read through), and 5 rows asking for 10 neighbours (n - 1 < k: the
                        result itself ends in -1 / NaN); the poison is NaN as a key and -1 as a row.
  similar_rows/plain    150 rows, c = 6, k = 10, one segment and the library's choice, a padded leading dimension.
"""
import numpy as np
import pytest

from tests import guard_scenarios as gs, similarity_oracle as so, test_gpu_guard_bands as bands

pytestmark = pytest.mark.gpu

NAMES = ('similar_rows/short', 'similar_rows/plain')


def _short_inputs():
    X, Q = so.memberships(70, 4), so.memberships(3, 4, seed=8)
    return X, Q, np.array([0, -1, 69], dtype=np.int32), so.memberships(5, 3)


def _plain_inputs():
    X = so.memberships(150, 6)
    return X, np.concatenate([X, np.full((150, 3), 1e3)], axis=1)


def _out(prefix, pair, out):
    out[prefix + '/index'], out[prefix + '/score'] = pair


def _run_short(K):
    X, Q, self_rows, tiny = _short_inputs()
    out = {}
    for metric in so.METRICS:
        got = K.similar_rows(K.to_device(X), K.to_device(Q), K.to_device(self_rows), k=64, metric=metric, segments=2)
        _out(f'{metric}/two_segments', (gs.host(K, got[0]), gs.host(K, got[1])), out)
        got = K.similar_rows(K.to_device(tiny), k=10, metric=metric, segments=3)
        _out(f'{metric}/five_rows', (gs.host(K, got[0]), gs.host(K, got[1])), out)
    return out


def _want_short():
    X, Q, self_rows, tiny = _short_inputs()
    want = {}
    for metric in so.METRICS:
        _out(f'{metric}/two_segments', so.similar_rows(X, Q, self_rows, 64, metric), want)
        _out(f'{metric}/five_rows', so.similar_rows(tiny, k=10, metric=metric), want)
    assert np.all(want['cosine/five_rows/index'][:, 4:] == -1)
    return gs.exact(want)


def _run_plain(K):
    X, padded = _plain_inputs()
    out = {}
    for metric in so.METRICS:
        for segments in (1, 0):
            got = K.similar_rows(K.to_device(X), k=10, metric=metric, segments=segments)
            _out(f'{metric}/{segments}', (gs.host(K, got[0]), gs.host(K, got[1])), out)
        got = K.similar_rows(K.to_device(padded), k=10, metric=metric, c=6)
        _out(f'{metric}/padded', (gs.host(K, got[0]), gs.host(K, got[1])), out)
    return out


def _want_plain():
    X, _ = _plain_inputs()
    want = {}
    for metric in so.METRICS:
        for what in ('1', '0', 'padded'):
            _out(f'{metric}/{what}', so.similar_rows(X, k=10, metric=metric), want)
    return gs.exact(want)


if not any(s.name in NAMES for s in gs.SCENARIOS):
    gs.scenario(NAMES[0], ('grx_similar_rows',), want=_want_short)(_run_short)
    gs.scenario(NAMES[1], ('grx_similar_rows',), want=_want_plain)(_run_plain)


@pytest.fixture(scope='module')
def K():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from graphrole_amd import kernels
    return kernels


@pytest.mark.parametrize('name', NAMES)
def test_guards_and_poison(K, name):
    scenario = next(s for s in gs.SCENARIOS if s.name == name)
    assert scenario.repeatable and scenario.want is not None and 'grx_similar_rows' in scenario.covers
    bands.test_guards_and_poison(K, name)
