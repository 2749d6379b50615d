"""
The second trip of every capped grid-stride launch of grx_triad_census, on the MI355X, in the manner of
tests/test_gpu_second_trip.py: C interleaved copies of the directed motif of tests/tiled_graphs.py, as its all-neighbour
CSR with the direction code of every slot (tests/triad_oracle.py::tiled_motif), with n just above 5 / 4 of the largest
cap * rows-per-workgroup among the launches of the call (the totals: 2 048 workgroups of 256 rows) and its arc count
past RJ_ARC_MAX_WG * arcs-per-workgroup at every lane width.  The test asserts from the copies of the caps in
graphrole_amd/kernels.py that the launches wrap, compares with the formula oracle on the tiled arrays, and compares the
connected and closed columns and the common neighbours per arc with the motif's own, tiled (the null and dyadic columns
depend on n and on the number of pairs of the whole graph), and with the one-trip run on the motif alone.
"""
import functools

import numpy as np
import pytest

from tests import tiled_graphs as tg
from tests import triad_oracle as to

pytestmark = pytest.mark.gpu


def _wraps(items, per_block, cap):
    return items > cap * per_block


@functools.lru_cache(maxsize=None)
def _tiled(rows):
    return to.tiled_motif(tg.copies_for(tg.motif('directed').n, rows + rows // 4))


def test_triad_census():
    from graphrole_amd import kernels as K
    rows = K.TD_MAX_WG * K.RJ_BLOCK                                             # the largest trip of the call
    (m_ptr, m_col, m_codes), C, (n, row_ptr, col, codes, arc_src) = _tiled(rows)
    n0, nnz = len(m_ptr) - 1, len(col)
    assert rows + rows // 4 < n <= rows + rows // 4 + n0
    big, small = K.DeviceCSR(row_ptr, col), K.DeviceCSR(m_ptr, m_col)
    assert big.n_hubs == C * small.n_hubs > 0 and big.lanes_per_row == small.lanes_per_row == 4
    d_codes, d_small_codes = K.to_device(codes), K.to_device(m_codes)
    want, motif = to.census(row_ptr, col, codes), to.census(m_ptr, m_col, m_codes)
    local = [to.T[name] for name in to.WEDGES + to.CLOSED]                      # what does not depend on n
    assert np.count_nonzero(motif.totals[local]) == 11                          # all but 030T and 030C occur there
    assert np.array_equal(want.columns[local], tg.tile_nodes(motif.columns[local], C))
    assert np.array_equal(want.common, motif.common[arc_src])
    for lanes in (32, big.lanes_per_row):
        assert _wraps(nnz, K.RJ_BLOCK, K.TD_MAX_WG)                             # td_pairs
        assert _wraps(n, K.RJ_BLOCK, K.TD_MAX_WG)                               # td_totals
        assert _wraps(n, K.RJ_BLOCK // lanes, K.RJ_ROW_MAX_WG)                  # rj_rows<L>: td_stats and td_sums
        assert _wraps(nnz, K.RJ_BLOCK // lanes, K.RJ_ARC_MAX_WG)                # rj_arc<L>: td_arc
        columns, totals, arc = K.triad_census(big, d_codes, want_totals=True, want_arc_triads=True, lanes=lanes)
        columns, totals, arc = K.to_host(columns), K.to_host(totals), K.to_host(arc)[:nnz]
        assert columns.dtype == np.int64 and columns.shape == (16, n) and arc.dtype == np.int32
        assert np.array_equal(arc, want.common), lanes
        assert np.array_equal(columns, want.columns), lanes
        assert np.array_equal(totals, want.totals), lanes
        columns0, _, arc0 = K.triad_census(small, d_small_codes, want_arc_triads=True, lanes=lanes)
        assert columns[local].tobytes() == tg.tile_nodes(K.to_host(columns0)[local], C).tobytes(), lanes
        assert arc.tobytes() == K.to_host(arc0)[:small.nnz][arc_src].tobytes(), lanes
