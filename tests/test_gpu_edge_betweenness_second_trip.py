"""
The second trip of every capped grid-stride launch that edge betweenness adds, on the MI355X, in the manner of
tests/test_gpu_second_trip.py: C interleaved copies of a small motif (tests/tiled_graphs.py) with n just above 5 / 4 of
the largest cap * rows-per-workgroup among the launches of the call, one batch of the narrowest width of sources spread
over three copies.  Each test asserts from the copies of the caps in graphrole_amd/kernels.py that its launches wrap,
compares with the motif's oracle answer tiled, and asserts the bytes of the one-trip run on the motif alone, tiled.

The order in which an arc slot adds its sources depends on a source's POSITION in the caller's list, so the run on the
motif alone keeps every source of the copy at its position and puts -1 (an id that reaches nothing) at the others.
"""
import functools

import numpy as np
import pytest

from tests import edge_betweenness_oracle as eo
from tests import tiled_graphs as tg

pytestmark = pytest.mark.gpu


def _wraps(items, per_block, cap):
    return items > cap * per_block


@functools.lru_cache(maxsize=None)
def _tiled(kind, rows, inn=False):
    m = tg.motif(kind)
    C = tg.copies_for(m.n, rows + rows // 4)
    a = m.inn if inn else (m.row_ptr, m.col, m.w)
    n, row_ptr, col, w, arc_src = tg.tile(a[0], a[1], C, a[2])
    assert rows + rows // 4 < n <= rows + rows // 4 + m.n
    return m, C, n, row_ptr, col, w, arc_src


def _pair(K, kind, rows, inn=False):
    t = _tiled(kind, rows, inn)
    m = t[0]
    a = m.inn if inn else (m.row_ptr, m.col, m.w)
    big, small = K.DeviceCSR(t[3], t[4], t[5]), K.DeviceCSR(*a)
    assert big.n_hubs == t[1] * small.n_hubs > 0 and big.lanes_per_row == small.lanes_per_row
    return t, big, small


def _tiled_arcs(solve, sources, C, row_ptr_big, arc_src):
    """The per-arc answer on the tiling from ``solve(motif rows, -1 where the source is in another copy)``."""
    sources = np.asarray(sources, dtype=np.int64)
    j, c = sources // C, sources % C
    copy_of_arc = np.repeat(np.arange(len(row_ptr_big) - 1, dtype=np.int64), np.diff(row_ptr_big)) % C
    out = np.zeros(len(arc_src))
    for k in np.unique(c):
        own = solve(np.where(c == k, j, -1))
        at = copy_of_arc == k
        out[at] = own[arc_src[at]]
    return out


def _both_slots(row_ptr, col, arc, directed, scale):
    n = len(row_ptr) - 1
    u = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    col = np.asarray(col, dtype=np.int64)
    if directed:
        return arc * scale
    mirror = np.searchsorted(u * n + col, col * n + u)
    return np.where(u == col, arc, arc + arc[mirror]) * scale


@pytest.mark.parametrize('kind', ['structural', 'directed'])
def test_edge_betweenness(kind):
    from graphrole_amd import kernels as K
    directed = kind == 'directed'
    rows = K.EB_MAX_ROW_BLOCKS * (K.EB_BLOCK // K.EB_ROW_LANES)                # the largest trip of the call
    (m, C, n, row_ptr, col, _, arc_src), big, small = _pair(K, kind, rows)
    big_in = small_in = None
    if directed:
        _, big_in, small_in = _pair(K, kind, rows, inn=True)
    sources = tg.spread_sources(m.n, C, 20, seed=6)                            # one batch of 64, partial
    assert sources.max() > rows and len(set((sources % C).tolist())) == 3
    assert _wraps(n, K.EB_BLOCK // K.EB_ROW_LANES, K.EB_MAX_ROW_BLOCKS)        # eb_rows: zero, scale / combine, mirror
    assert _wraps(n, K.BW_BLOCK // 64, K.BW_MAX_ROW_BLOCKS)                    # bw_edge_kernel, forward, backward<true>

    def device(csr, csr_in, js):
        return K.to_host(K.edge_betweenness(csr, csr_in, js, 0.25, batch=64))[:csr.nnz]

    def oracle(js):
        arc = eo.arc_sums(m.row_ptr, m.col, [s for s in js if s >= 0])
        return _both_slots(m.row_ptr, m.col, arc, directed, 0.25)

    got = device(big, big_in, sources)
    want = _tiled_arcs(oracle, sources, C, row_ptr, arc_src)
    assert got.dtype == np.float64 and np.count_nonzero(want) > 0
    np.testing.assert_allclose(got, want, rtol=eo.RTOL, atol=0)
    assert np.array_equal(got == 0, want == 0)
    alone = _tiled_arcs(lambda js: device(small, small_in, js), sources, C, row_ptr, arc_src)
    assert got.tobytes() == alone.tobytes()


@pytest.mark.parametrize('kind', ['ints', 'directed'])
def test_weighted_edge_betweenness(kind):
    from graphrole_amd import kernels as K
    directed = kind == 'directed'
    batch = 16
    rows = K.WB_MAX_ROW_BLOCKS * (K.WB_BLOCK // batch)                         # the largest trip of the call
    (m, C, n, row_ptr, col, _, arc_src), big, small = _pair(K, kind, rows)
    big_in = small_in = None
    out = inn = (m.row_ptr, m.col, m.w)
    if directed:
        _, big_in, small_in = _pair(K, kind, rows, inn=True)
        inn = m.inn
    sources = tg.spread_sources(m.n, C, 13, seed=6)                            # one batch of 16, partial
    assert sources.max() > rows and len(set((sources % C).tolist())) == 3
    assert _wraps(n, K.EB_BLOCK // K.EB_ROW_LANES, K.EB_MAX_ROW_BLOCKS)        # eb_rows: zero, scale / combine, mirror
    assert _wraps(n, K.WB_BLOCK // batch, K.WB_MAX_ROW_BLOCKS)                 # wb_edge_kernel, forward, backward<true>
    assert _wraps(n, K.SP_BLOCK // batch, K.SP_MAX_ROW_BLOCKS)                 # sp_round<S>

    def device(csr, csr_in, js):
        ebc, rounds, levels = K.weighted_edge_betweenness(csr, csr_in, js, 0.25, batch)
        return K.to_host(ebc)[:csr.nnz], rounds, levels

    def oracle(js):
        arc, _ = eo.weighted_arc_sums(out, inn, [s for s in js if s >= 0])
        return _both_slots(m.row_ptr, m.col, arc, directed, 0.25)

    got, rounds, levels = device(big, big_in, sources)
    want = _tiled_arcs(oracle, sources, C, row_ptr, arc_src)
    assert np.count_nonzero(want) > 0
    np.testing.assert_allclose(got, want, rtol=eo.RTOL, atol=0)
    assert np.array_equal(got == 0, want == 0)
    alone = _tiled_arcs(lambda js: device(small, small_in, js)[0], sources, C, row_ptr, arc_src)
    assert got.tobytes() == alone.tobytes()
    _, rounds0, levels0 = device(small, small_in, sources // C)               # every batch holds the same lanes
    assert (rounds, levels) == (rounds0, levels0) and levels > 2
