"""
The guard-band shim of tests/guarded_alloc.py caught in the act on host memory (no GPU): the proxy is told to guard
'cpu' allocations, the "kernel" is a numpy write through the base tensor.  Plus the static completeness condition of
tests/guard_scenarios.py: every device entry point of the ABI is covered by a scenario or is on the exclusion list
below, whose entries may only be host functions, runtime / copy helpers, the multi-process communicator, plan
management and pure size / query functions.
"""
import sys

import numpy as np
import torch

from tests import guarded_alloc as ga
from tests.guarded_alloc import GUARD


def _proxy(poison=False):
    return ga.GuardedTorch(poison=poison, guard_types=('cpu',))


def _raw(proxy, k=-1):
    """The whole base allocation (guards included) of the k-th record as a writable numpy view."""
    return proxy.records[k].base.numpy()


def _line():
    return sys._getframe(1).f_lineno


def test_clean_run_reports_nothing():
    p = _proxy()
    a = p.empty(100, dtype=torch.float64, device='cpu')
    b = p.zeros((3, 7), dtype=torch.int32, device='cpu')
    c = p.empty_like(a)
    a.numpy()[:] = 1.0
    b.numpy()[:] = 2
    c.numpy()[:] = 3.0
    assert len(p.records) == 3 and p.check() == []
    assert _raw(p, 0)[:GUARD].tolist() == [ga.GUARD_BYTE] * GUARD
    p.clear()
    assert p.records == []


def test_one_byte_overrun_is_reported_with_site_and_offset():
    p = _proxy()
    line = _line() + 1
    t = p.empty(13, dtype=torch.uint8, device='cpu')
    assert t.numel() == 13
    _raw(p)[GUARD + 13] = 0x42                                   # the first byte behind an interior that is NOT rounded up
    (v,) = p.check()
    assert v.side == 'back' and (v.first, v.last) == (13, 13) and v.found == b'\x42' and v.nbytes == 13
    assert v.site == f'test_one_byte_overrun_is_reported_with_site_and_offset:{line}'
    assert 'back guard' in str(v) and v.site in str(v) and '13..13' in str(v)


def test_one_byte_underrun_is_reported_with_site_and_offset():
    p = _proxy()
    p.empty(8, dtype=torch.int64, device='cpu')                  # a clean neighbour
    line = _line() + 1
    p.empty((4, 4), dtype=torch.float64, device='cpu')
    _raw(p)[GUARD - 1] = 0
    (v,) = p.check()
    assert v.side == 'front' and (v.first, v.last) == (-1, -1) and v.found == b'\x00'
    assert v.site == f'test_one_byte_underrun_is_reported_with_site_and_offset:{line}'


def test_one_element_past_an_orbit_block_is_reported():
    n = 37
    p = _proxy()
    line = _line() + 1
    t = p.empty((15, n), dtype=torch.float64, device='cpu')
    raw = _raw(p)
    raw[GUARD:GUARD + 8 * 15 * n].view(np.float64)[:] = 1.0     # the block itself: legal
    assert p.check() == []
    raw[GUARD + 8 * 15 * n:GUARD + 8 * (15 * n + 1)].view(np.float64)[0] = 1.0      # element [15, 0]
    (v,) = p.check()
    assert v.side == 'back' and v.nbytes == 8 * 15 * n
    assert (v.first, v.last) == (8 * 15 * n, 8 * 15 * n + 7) and v.found == np.float64(1.0).tobytes()
    assert v.site == f'test_one_element_past_an_orbit_block_is_reported:{line}'
    assert t.shape == (15, n)


def test_both_sides_and_several_allocations():
    p = _proxy()
    p.empty(5, dtype=torch.int32, device='cpu')
    p.empty(6, dtype=torch.int32, device='cpu')
    _raw(p, 0)[GUARD + 20:GUARD + 24] = 7
    _raw(p, 1)[GUARD - 4:GUARD] = 7
    _raw(p, 1)[GUARD + 24 + 100] = 7
    got = [(v.side, v.first, v.last) for v in p.check()]
    assert got == [('back', 20, 23), ('front', -4, -1), ('back', 124, 124)]


def test_poison_patterns():
    p = _proxy(poison=True)
    f = p.empty((3, 5), dtype=torch.float64, device='cpu')
    i = p.empty(7, dtype=torch.int32, device='cpu')
    q = p.empty(7, dtype=torch.int64, device='cpu')
    e = p.empty_like(f)
    assert np.isnan(f.numpy()).all() and np.isnan(e.numpy()).all()
    assert (i.numpy() == -1).all() and (q.numpy() == -1).all()
    z = p.zeros((2, 3), dtype=torch.float64, device='cpu')       # zeros stays zeros under poison
    assert not z.numpy().any()
    assert p.check() == []


def test_without_poison_the_interior_is_left_as_allocated():
    p = _proxy(poison=False)
    t = p.empty(64, dtype=torch.uint8, device='cpu')
    assert _raw(p)[GUARD:GUARD + 64].tobytes() == t.numpy().tobytes()   # the very bytes of the base, whatever they are
    assert not p._poison
    calls = []
    real = torch.Tensor.fill_
    try:                                                         # no fill touches the interior: only the two guards
        torch.Tensor.fill_ = lambda self, v: (calls.append(self.numel()), real(self, v))[1]
        p.empty(64, dtype=torch.uint8, device='cpu')
    finally:
        torch.Tensor.fill_ = real
    assert calls == [GUARD, GUARD]


def test_view_is_contiguous_with_the_requested_shape_dtype_and_stride():
    p = _proxy()
    for args, kw, shape in (((4, 5, 6), {}, (4, 5, 6)), (((4, 5),), {}, (4, 5)), ((9,), {}, (9,)), (([2, 3],), {}, (2, 3)),
                            ((torch.Size([7, 2]),), {}, (7, 2))):
        for dtype in (torch.float64, torch.int32, torch.int64, torch.uint8):
            t = p.empty(*args, dtype=dtype, device='cpu', **kw)
            want = torch.empty(shape, dtype=dtype)
            assert t.shape == want.shape and t.dtype == dtype and t.stride() == want.stride() and t.is_contiguous()
            assert t.data_ptr() % 256 == p.records[-1].base.data_ptr() % 256      # GUARD keeps the base's alignment
            assert p.records[-1].nbytes == want.numel() * want.element_size()
    src = torch.empty((6, 4), dtype=torch.float64)[:, ::2]       # empty_like of a strided tensor: contiguous, same shape
    t = p.empty_like(src)
    assert t.shape == (6, 2) and t.is_contiguous() and t.dtype == torch.float64
    assert p.check() == []


def test_zero_size_request_works():
    p = _proxy(poison=True)
    for shape in ((0,), (0, 5), (3, 0)):
        t = p.empty(shape, dtype=torch.float64, device='cpu')
        assert tuple(t.shape) == shape and t.numel() == 0 and p.records[-1].nbytes == 0
        assert p.records[-1].base.numel() == 2 * GUARD
    assert p.check() == []
    _raw(p)[GUARD] = 1                                           # the first byte behind nothing is the back guard
    (v,) = p.check()
    assert v.side == 'back' and v.first == 0


def test_pinned_and_host_requests_are_not_wrapped():
    p = ga.GuardedTorch(poison=True)                             # the default: only device allocations are guarded
    a = p.empty(10, dtype=torch.float64, device='cpu')
    b = p.empty(10, dtype=torch.float64)
    c = p.zeros((2, 2), dtype=torch.int32)
    d = p.empty_like(a)
    assert p.records == []
    assert a.untyped_storage().nbytes() == 80 and not c.numpy().any() and d.shape == a.shape and b.numel() == 10
    q = _proxy(poison=True)                                      # even a proxy that guards 'cpu' leaves pinned requests alone
    try:
        e = q.empty(16, dtype=torch.float64, pin_memory=True)
        assert e.numel() == 16
    except RuntimeError:                                         # no accelerator runtime to pin with: still not wrapped
        pass
    assert q.records == []
    assert p.float64 is torch.float64 and p.Tensor is torch.Tensor and p.from_numpy is torch.from_numpy


# ---- completeness: static -------------------------------------------------------------------------------------------

#: every entry point NO scenario covers, with the reason.  Only: host functions, runtime / event / profile / trace / copy
#: helpers, the communicator (several processes: tests/test_gpu_sharded.py), plan management, pure size / query functions.
EXCLUDED = {
    'grx_version': 'query: the ABI version',
    'grx_last_error': 'query: the message of the last failed call',
    'grx_device_info': 'query: compute units and memory of the device',
    'grx_dev_malloc': 'runtime: the library\'s own allocation, below the ABI',
    'grx_dev_free': 'runtime: the library\'s own allocation, below the ABI',
    'grx_memcpy_h2d': 'copy helper',
    'grx_memcpy_d2h': 'copy helper',
    'grx_stream_sync': 'runtime: stream synchronisation',
    'grx_download': 'copy helper: device to pageable host memory through the staging ring',
    'grx_upload': 'copy helper: host to device through the staging ring',
    'grx_upload_i64_as_i32': 'copy helper: narrowing upload through the staging ring',
    'grx_host_checksums': 'host function',
    'grx_host_uniform_choice': 'host function',
    'grx_host_whiten': 'host function',
    'grx_host_whiten_for_rank': 'host function',
    'grx_host_range_finder': 'host function',
    'grx_host_small_svd': 'host function',
    'grx_host_nndsvd_plan': 'host function',
    'grx_host_prune': 'host function',
    'grx_host_eigh': 'host function',
    'grx_host_nnls': 'host function',
    'grx_event_create': 'runtime: events',
    'grx_event_destroy': 'runtime: events',
    'grx_event_record': 'runtime: events',
    'grx_event_elapsed_ms': 'runtime: events',
    'grx_trace_marker': 'trace helper',
    'grx_profile_enable': 'profile helper',
    'grx_profile_enabled': 'profile helper',
    'grx_profile_select': 'profile helper',
    'grx_profile_reset': 'profile helper',
    'grx_profile_kernel_count': 'profile helper',
    'grx_profile_kernel_name': 'profile helper',
    'grx_profile_read': 'profile helper',
    'grx_comm_rccl_unique_id': 'communicator: several processes, tests/test_gpu_sharded.py',
    'grx_comm_create_rccl': 'communicator: several processes, tests/test_gpu_sharded.py',
    'grx_comm_create_callbacks': 'communicator: several processes, tests/test_gpu_sharded.py',
    'grx_comm_destroy': 'communicator: several processes, tests/test_gpu_sharded.py',
    'grx_comm_rank': 'communicator: several processes, tests/test_gpu_sharded.py',
    'grx_comm_world': 'communicator: several processes, tests/test_gpu_sharded.py',
    'grx_comm_all_reduce': 'communicator: several processes, tests/test_gpu_sharded.py',
    'grx_comm_exchange': 'communicator: several processes, tests/test_gpu_sharded.py',
    'grx_comm_all_gather_rows': 'communicator: several processes, tests/test_gpu_sharded.py',
    'grx_comm_columns_to_owners': 'communicator: several processes, tests/test_gpu_sharded.py',
    'grx_comm_owned_to_rows': 'communicator: several processes, tests/test_gpu_sharded.py',
    'grx_comm_timing': 'communicator: several processes, tests/test_gpu_sharded.py',
    'grx_comm_timing_read': 'communicator: several processes, tests/test_gpu_sharded.py',
    'grx_comm_timing_reset': 'communicator: several processes, tests/test_gpu_sharded.py',
    'grx_aggregate_plan_create': 'plan management (host preprocessing; its device memory is the library\'s own)',
    'grx_aggregate_plan_destroy': 'plan management',
    'grx_aggregate_plan_info': 'plan management: query',
    'grx_aggregate_plan_set_lanes': 'plan management',
    'grx_aggregate_ldr': 'pure size function',
    'grx_aggregate_ldi': 'pure size function',
    'grx_aggregate_i32_ok': 'pure query on a plan',
    'grx_packed_row_bytes': 'pure size function',
    'grx_refex_bin_batch': 'pure size function',
}

_ALLOWED_PREFIXES = ('grx_host_', 'grx_comm_', 'grx_event_', 'grx_profile_', 'grx_aggregate_plan_')
_ALLOWED_NAMES = {'grx_version', 'grx_last_error', 'grx_device_info', 'grx_dev_malloc', 'grx_dev_free', 'grx_memcpy_h2d',
                  'grx_memcpy_d2h', 'grx_stream_sync', 'grx_download', 'grx_upload', 'grx_upload_i64_as_i32',
                  'grx_trace_marker', 'grx_aggregate_ldr', 'grx_aggregate_ldi', 'grx_aggregate_i32_ok',
                  'grx_packed_row_bytes', 'grx_refex_bin_batch'}


def _is_size_function(name, signature):
    restype, argtypes = signature
    import ctypes
    return name.endswith('_workspace_bytes') and restype is ctypes.c_size_t and ctypes.c_void_p not in argtypes


def test_every_device_entry_point_has_a_scenario():
    from graphrole_amd import _lib
    from tests import guard_scenarios as gs
    signatures = _lib._SIGNATURES
    covered = set()
    for s in gs.SCENARIOS:
        assert s.covers, s.name
        covered.update(s.covers)
    sizes = {name for name, sig in signatures.items() if _is_size_function(name, sig)}
    excluded = set(EXCLUDED) | sizes
    assert all(isinstance(r, str) and r for r in EXCLUDED.values())
    for name in EXCLUDED:                                        # the list holds only the allowed categories
        assert name.startswith(_ALLOWED_PREFIXES) or name in _ALLOWED_NAMES, name
    unknown = (covered | set(EXCLUDED)) - set(signatures)
    assert not unknown, f'not in _lib._SIGNATURES: {sorted(unknown)}'
    assert not covered & excluded, f'covered AND excluded: {sorted(covered & excluded)}'
    missing = set(signatures) - covered - excluded
    assert not missing, f'entry points without a guard-band scenario: {sorted(missing)}'
    names = [s.name for s in gs.SCENARIOS]
    assert len(set(names)) == len(names)
