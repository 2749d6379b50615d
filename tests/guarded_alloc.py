"""
Guard-band allocator shim for graphrole_amd.kernels (test code only; no product file knows about it).

``GuardedTorch`` stands in for the name ``torch`` inside ``graphrole_amd.kernels``.  Everything is delegated to the
real torch except ``empty``, ``zeros`` and ``empty_like`` when the result is a device tensor: those come out of one
uint8 base tensor of GUARD + nbytes + GUARD bytes whose two guards are filled with 0xA5.  The interior is exactly
nbytes long (no rounding: the back guard starts at the first byte behind it) and is handed out as a contiguous view
of the requested dtype and shape.  With ``poison=True`` the interior is filled with 0xFF first: a NaN as fp64, -1 as
int32 / int64 -- the one pattern whose use as an index or row pointer reads just in front of the buffer, inside the
owned guard, and never leaves the allocation.  Host tensors (device='cpu', no device, pin_memory=True) pass through.

``check()`` synchronises and compares every guard with 0xA5; ``guarded(K, poison)`` installs the proxy, records the
entry points reached through ``K._lib`` and restores everything on exit.
"""
import contextlib
import os
import sys
from dataclasses import dataclass

import numpy as np
import torch as _torch

GUARD = 4096
GUARD_BYTE = 0xA5
POISON_BYTE = 0xFF
_HERE = os.path.abspath(__file__)


@dataclass
class Violation:
    site: str          # 'function:line' of the allocation
    side: str          # 'front' or 'back'
    first: int         # byte offsets of the first and last changed guard byte, relative to the interior's first byte
    last: int          # (front: negative, back: >= nbytes)
    nbytes: int
    found: bytes       # the changed stretch [first, last], at most 32 bytes of it

    def __str__(self):
        return (f'{self.side} guard of the {self.nbytes}-byte allocation at {self.site} overwritten: offsets '
                f'{self.first}..{self.last} relative to the buffer, found {self.found.hex()}')


@dataclass
class _Record:
    base: object
    nbytes: int
    site: str


def _size_of(size):
    if len(size) == 1 and not isinstance(size[0], (int, np.integer)):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


class GuardedTorch:
    """Proxy of the torch module; ``guard_types``: the device types whose allocations are guarded (the CPU self-tests
    pass ('cpu',) to exercise the very same code on host memory)."""

    def __init__(self, poison=False, guard_types=('cuda',), site_file=None):
        self._poison = bool(poison)
        self._guard_types = tuple(guard_types)
        self._site_file = None if site_file is None else os.path.abspath(site_file)
        self.records = []

    def __getattr__(self, name):
        return getattr(_torch, name)

    # ---- the three allocation calls -------------------------------------------------------------------------------
    def empty(self, *size, **kw):
        if self._guards(kw):
            return self._allocate(_size_of(size), kw, zero=False)
        return _torch.empty(*size, **kw)

    def zeros(self, *size, **kw):
        if self._guards(kw):
            return self._allocate(_size_of(size), kw, zero=True)
        return _torch.zeros(*size, **kw)

    def empty_like(self, t, **kw):
        kw.setdefault('dtype', t.dtype)
        kw.setdefault('device', t.device)
        if self._guards(kw):
            return self._allocate(tuple(t.shape), kw, zero=False)
        return _torch.empty_like(t, **kw)

    def _guards(self, kw):
        if kw.get('pin_memory') or kw.get('device') is None:
            return False
        return _torch.device(kw['device']).type in self._guard_types

    def _site(self):
        """'function:line' of the allocating frame in site_file -- followed by its callers in the same file ('zeros:150
        < triangle_counts:417'), since a helper's own line says little; without site_file: the first frame outside
        this module."""
        frame = sys._getframe(3)
        chain, fallback = [], None
        while frame is not None and len(chain) < 3:
            path = os.path.abspath(frame.f_code.co_filename)
            here = f'{frame.f_code.co_name}:{frame.f_lineno}'
            if path != _HERE:
                if self._site_file is None:
                    return here
                if path == self._site_file:
                    chain.append(here)
                elif chain:
                    break
                fallback = fallback or here
            frame = frame.f_back
        return ' < '.join(chain) or fallback or '?'

    def _allocate(self, shape, kw, zero):
        dtype = kw.get('dtype') or _torch.get_default_dtype()
        count = 1
        for s in shape:
            count *= s
        nbytes = count * _torch.empty(0, dtype=dtype).element_size()
        base = _torch.empty(GUARD + nbytes + GUARD, dtype=_torch.uint8, device=kw['device'])
        base[:GUARD].fill_(GUARD_BYTE)
        base[GUARD + nbytes:].fill_(GUARD_BYTE)
        interior = base[GUARD:GUARD + nbytes]
        if zero:
            interior.zero_()
        elif self._poison:
            interior.fill_(POISON_BYTE)
        self.records.append(_Record(base, nbytes, self._site()))
        return interior.view(dtype).view(shape)

    # ---- the check ---------------------------------------------------------------------------------------------------
    def check(self):
        """Synchronise, compare every guard with 0xA5; the list of Violations (empty: all intact)."""
        if any(r.base.is_cuda for r in self.records):
            _torch.cuda.synchronize()
        bad = []
        for r in self.records:
            host = r.base[:GUARD].cpu().numpy(), r.base[GUARD + r.nbytes:].cpu().numpy()
            for side, g, origin in (('front', host[0], -GUARD), ('back', host[1], r.nbytes)):
                hit = np.nonzero(g != GUARD_BYTE)[0]
                if len(hit):
                    first, last = int(hit[0]), int(hit[-1])
                    bad.append(Violation(r.site, side, origin + first, origin + last, r.nbytes,
                                         g[first:min(last + 1, first + 32)].tobytes()))
        return bad

    def clear(self):
        self.records.clear()


class _RecordingLib:
    """The loaded library with every grx_* function noting its name when it is called."""

    def __init__(self, lib, names):
        self._lib, self._names = lib, names

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('grx_'):
            return fn

        def recorded(*args):
            self._names.add(name)
            return fn(*args)
        return recorded


class Session:
    def __init__(self, proxy, calls):
        self.proxy, self.calls = proxy, calls

    def check(self):
        return self.proxy.check()


@contextlib.contextmanager
def guarded(K, poison=False):
    """Within the block ``K.torch`` is a GuardedTorch and ``K._lib.call`` / ``K._lib.load`` record the entry points
    they reach (``session.calls``).  The register keeps every allocation alive until the block ends."""
    lib_mod = K._lib
    proxy = GuardedTorch(poison=poison, site_file=K.__file__)
    calls = set()
    real_torch, real_call, real_load = K.torch, lib_mod.call, lib_mod.load

    def call(name, *args):
        calls.add(name)
        return real_call(name, *args)

    def load():
        return _RecordingLib(real_load(), calls)

    K.torch, lib_mod.call, lib_mod.load = proxy, call, load
    try:
        yield Session(proxy, calls)
    finally:
        K.torch, lib_mod.call, lib_mod.load = real_torch, real_call, real_load
        if any(r.base.is_cuda for r in proxy.records):
            _torch.cuda.synchronize()
        proxy.clear()
