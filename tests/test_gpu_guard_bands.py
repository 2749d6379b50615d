"""
-m gpu: guard bands and poisoned memory around every device entry point of graphrole_amd.kernels.

Every output, scratch buffer and workspace of the product path is a ``torch.empty`` of kernels.py, which the caching
allocator rounds up to 512 bytes, carves out of shared blocks and -- in a fresh process -- usually hands out zeroed.  A
write a few elements past an output, a ``*_workspace_bytes`` that is short by one aligned vector, or an accumulation
into an ``empty`` that should have been ``zeros`` therefore changes no value any other test reads.  Here every
allocation of kernels.py comes out of tests/guarded_alloc.py instead: exactly as long as asked for, between two 4 KiB
guards of 0xA5, and in the second run filled with 0xFF (NaN as fp64, -1 as an integer) first.  For every scenario of
tests/guard_scenarios.py:

  A  guards on, no poison: every guard intact;
  B  guards on, poison on: every guard intact;
  A == B byte for byte on the defined region of every output (every family is documented as bitwise repeatable);
  B against the family's oracle where the scenario has one (a result that is wrong under poison fails against the
     reference, not merely against another run of the same code);
  the entry points reached include the scenario's declared ``covers``.

A failure names the scenario, the allocation site in kernels.py ('function:line', helpers followed by their
callers), front or back, and the byte offsets -- most of the time that alone says which kernel overran which buffer.

Out of scope, so that nobody takes this file for more than it is:
  * memory the library allocates for itself below the ABI (grx_dev_malloc, plans, staging rings);
  * graphrole_amd/parallel.py and the multi-rank paths;
  * reads past an input: a guard cannot see a read.

Findings fixed with this file: none -- every guard stayed intact and no result depended on what the memory held.
"""
import numpy as np
import pytest

from tests import guard_scenarios as gs, guarded_alloc as ga

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from graphrole_amd import kernels
    return kernels


def _run(K, scenario, poison):
    # the draws some wrappers take from numpy's global generator (k-means seeding caches, the NMF omega of the role
    # extractor) are the same in both runs
    np.random.seed(0)
    try:
        with ga.guarded(K, poison=poison) as session:
            out = scenario.run(K)
            violations = session.check()
            calls = set(session.calls)
    except Exception as exc:
        if any(sign in str(exc) for sign in ('illegal memory access', 'Memory access fault', 'unspecified launch failure')):
            # nothing more is started on a device that has faulted
            pytest.exit(f'GPU fault in scenario {scenario.name} (poison={poison}): {exc}', returncode=3)
        raise
    assert isinstance(out, dict) and out and all(isinstance(a, np.ndarray) for a in out.values())
    return out, violations, calls


def _guards_intact(scenario, run, violations):
    assert not violations, f'scenario {scenario.name}, run {run}:\n' + '\n'.join(f'  {v}' for v in violations)


def _matches(got, want, how):
    if how == gs.EXACT:
        return got.shape == want.shape and np.array_equal(got, want, equal_nan=got.dtype.kind == 'f')
    if callable(how):
        return bool(how(got, want))
    rtol, atol = how
    return got.shape == want.shape and np.allclose(got, want, rtol=rtol, atol=atol, equal_nan=True)


@pytest.mark.parametrize('name', [s.name for s in gs.SCENARIOS])
def test_guards_and_poison(K, name):
    scenario = next(s for s in gs.SCENARIOS if s.name == name)
    a, bad_a, calls_a = _run(K, scenario, poison=False)
    _guards_intact(scenario, 'A (no poison)', bad_a)
    b, bad_b, calls_b = _run(K, scenario, poison=True)
    _guards_intact(scenario, 'B (poison)', bad_b)
    assert set(a) == set(b)
    if scenario.repeatable:
        differ = [k for k in a if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
        assert not differ, (f'scenario {name}: {len(differ)} outputs depend on what the memory held before the call '
                            f'(0xFF poison against as allocated): {differ[:12]}')
    if scenario.want is not None:
        want = scenario.want()
        assert set(want) <= set(b), sorted(set(want) - set(b))[:10]
        wrong = [k for k, (w, how) in want.items() if not _matches(b[k], np.asarray(w), how)]
        assert not wrong, f'scenario {name}: {len(wrong)} outputs of the poisoned run miss the oracle: {wrong[:12]}'
    else:
        assert scenario.repeatable, f'scenario {name} has neither an oracle nor repeatable bits'
    for calls in (calls_a, calls_b):
        missing = set(scenario.covers) - calls
        assert not missing, f'scenario {name} never reached {sorted(missing)}'


def test_the_shim_reports_a_device_write_behind_a_buffer(K):
    """One byte behind a guarded device allocation, written with grx_memset: inside the allocation this test owns
    (nothing faults), and check() names the side, the offset and the allocating line of kernels.py."""
    with ga.guarded(K, poison=True) as session:
        t = K.empty((3, 5))
        nbytes = t.numel() * t.element_size()
        assert t.is_cuda and len(session.proxy.records) == 1 and session.proxy.records[0].nbytes == nbytes
        assert np.isnan(K.to_host(t)).all()
        assert session.check() == []
        K._lib.call('grx_memset', K.c_void_p(t.data_ptr() + nbytes), 0x11, 1, K._stream())
        (v,) = session.check()
        assert v.side == 'back' and (v.first, v.last) == (nbytes, nbytes) and v.found == b'\x11'
        assert v.site.startswith('empty:') and K.empty.__code__.co_firstlineno < int(v.site.split(':')[1]) \
            <= K.empty.__code__.co_firstlineno + 2
        K._lib.call('grx_memset', K.c_void_p(t.data_ptr() - 8), 0, 8, K._stream())
        front = [v for v in session.check() if v.side == 'front']
        assert len(front) == 1 and (front[0].first, front[0].last) == (-8, -1)
        assert 'grx_memset' in session.calls
    z = K.zeros(4)                                               # the proxy is gone: plain allocations again
    assert K.torch.__name__ == 'torch' and not K.to_host(z).any()
