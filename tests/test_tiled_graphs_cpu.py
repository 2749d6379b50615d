"""
-m "not gpu": the expected values tests/test_gpu_second_trip.py compares the kernels with, proved without a kernel.  For
every oracle used there, at C = 3 and C = 5 copies, the oracle run on the tiled CSR of tests/tiled_graphs.py equals the
motif's answer tiled -- exactly where the oracle's output is integer or bit-defined, within the oracle module's own
tolerance otherwise --, the traversals from sources in the first copy, a middle copy and the last copy; the two
vectorised restatements of tiled_graphs.py give the bits of the oracles they restate; the motifs hold what they are
there for; and every launch cap the GPU tests size themselves by (the copies in graphrole_amd/kernels.py) is read back
from its source file, so that a changed cap fails here instead of silently un-wrapping a GPU test.
"""
import os
import re

import numpy as np
import pytest

from tests import biconnected_oracle as bo
from tests import eccentricity_oracle as eo
from tests import graphlet_oracle as go
from tests import neighbor_sense_oracle as nso
from tests import similarity_oracle as sim
from tests import square_clustering_oracle as sq
from tests import sssp_oracle as so
from tests import tiled_graphs as tg
from tests import truss_oracle as to
from tests import weighted_betweenness_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPIES = (3, 5)


def _source(name):
    return open(os.path.join(ROOT, 'graphrole_amd', 'csrc', name)).read()


# ------------------------------------------------------------------------------------------------------- the tiling
def test_tile_is_the_interleaved_disjoint_union():
    m = tg.motif('uniform')
    for C in COPIES:
        n, row_ptr, col, w, arc_src = tg.tile(m.row_ptr, m.col, C, m.w)
        assert n == m.n * C and len(row_ptr) == n + 1 and row_ptr[-1] == len(col) == len(m.col) * C
        rows = np.repeat(np.arange(n), np.diff(row_ptr))
        assert np.all(rows % C == col % C)                      # no arc between two copies
        assert np.all(np.diff(col)[np.diff(rows) == 0] > 0)     # ascending inside a row
        for c in (0, C - 1):                                    # copy c alone is the motif, arc for arc
            mine = rows % C == c
            assert np.array_equal(rows[mine] // C, np.repeat(np.arange(m.n), np.diff(m.row_ptr)))
            assert np.array_equal(col[mine] // C, m.col) and np.array_equal(arc_src[mine], np.arange(len(m.col)))
            assert np.array_equal(w[mine], m.w)
        if C > 1 and n:
            spans = col[row_ptr[:-1][np.diff(row_ptr) > 1] + 1] - col[row_ptr[:-1][np.diff(row_ptr) > 1]]
            assert np.all(spans >= C)                           # neighbours of a row are at least C labels apart
    assert tg.copies_for(203, 524288) == 2583 and 203 * 2583 > 524288 >= 203 * 2582
    assert tg.tile_nodes(np.array([[1, 2], [3, 4]]), 2).tolist() == [[1, 1, 2, 2], [3, 3, 4, 4]]
    assert tg.tile_ids(np.array([2, -1, 0], dtype=np.int32), 3).tolist() == [6, 7, 8, -1, -1, -1, 0, 1, 2]
    s = tg.spread_sources(m.n, 7, 20)
    assert len(s) == 20 and s[-1] == s[0] and s.max() == m.n * 7 - 1 and set((s % 7).tolist()) == {0, 3, 6}


def test_motifs_hold_what_they_are_there_for():
    from graphrole_amd import kernels as K
    for kind in ('structural', 'squares', 'long_stars', 'ints', 'dyadic', 'uniform', 'directed'):
        m = tg.motif(kind)
        deg = np.diff(m.row_ptr)
        lanes = 4                                               # what DeviceCSR picks below 12 arcs a row
        assert m.row_ptr[-1] / m.n < 12 and deg.max() > K.HUB_FACTOR * lanes, kind
        assert m.inn is None or np.diff(m.inn[0]).max() > K.HUB_FACTOR * lanes
        assert np.count_nonzero(deg == 0) >= 2, kind
        assert (m.w is None) == (kind in ('structural', 'squares')) and (m.inn is not None) == (kind == 'directed')
    m = tg.motif('structural')
    assert 200 < m.n < 300
    t = to.truss_numbers(m.row_ptr, m.col)
    assert sorted(set(t.arc_truss.tolist())) == [2, 3, 7] and t.n_levels == 3     # trees and the grid, the wheel, K7: k jumps
    assert eo.eccentricity_pass(m.row_ptr, m.col, [0])[0][0] > 8 or eo.distance_table(m.row_ptr, m.col, [0]).max() > 8
    b = bo.biconnected(m.row_ptr, m.col)
    assert b.n_components > 150 and b.count.max() > 100 and np.count_nonzero(b.parent < 0) == 3
    m = tg.motif('squares')
    wedges = sq.wedge_counts(m.row_ptr, m.col)
    Q, _, _ = sq.square_clustering(m.row_ptr, m.col)
    tiers = [wedges <= K.SQ_WAVE_MAX_WEDGES, (wedges > K.SQ_WAVE_MAX_WEDGES) & (wedges <= K.SQ_LDS_MAX_WEDGES),
             wedges > K.SQ_LDS_MAX_WEDGES]
    assert [int(t.sum()) for t in tiers[1:]] == [1, 2]
    assert all(np.all(Q[t & (wedges > 0)] > 0) for t in tiers[1:]) and np.count_nonzero(Q[tiers[0]]) > 100
    m = tg.motif('long_stars')
    deg = np.diff(m.row_ptr)
    assert deg[0] > nso.LONG_ROW and deg[-1] > nso.LONG_ROW and np.count_nonzero(deg > nso.LONG_ROW) == 2
    for kind in ('ints', 'dyadic', 'uniform'):
        m = tg.motif(kind)
        assert np.array_equal(m.w > 0, np.ones(len(m.w), dtype=bool))
        assert (kind == 'uniform') != bool(np.all(m.w * 4 == np.round(m.w * 4)))
    m = tg.motif('directed')
    assert not np.array_equal(m.row_ptr, m.inn[0]) and m.row_ptr[-1] == m.inn[0][-1]


# ------------------------------------------------------------- oracle on the tiling == the motif's oracle answer, tiled
@pytest.mark.parametrize('C', COPIES)
def test_truss_oracle_on_the_tiling(C):
    m = tg.motif('structural')
    want = to.truss_numbers(m.row_ptr, m.col)
    _, row_ptr, col, _, arc_src = tg.tile(m.row_ptr, m.col, C)
    got = to.truss_numbers(row_ptr, col)
    assert np.array_equal(got.arc_truss, want.arc_truss[arc_src])
    assert np.array_equal(got.node_truss, tg.tile_nodes(want.node_truss, C))
    assert (got.n_rounds, got.n_levels) == (want.n_rounds, want.n_levels)


@pytest.mark.parametrize('C', COPIES)
def test_graphlet_oracle_on_the_tiling(C):
    m = tg.motif('structural')
    want = go.orbits(m.row_ptr, m.col)
    _, row_ptr, col, _, arc_src = tg.tile(m.row_ptr, m.col, C)
    got = go.orbits(row_ptr, col)
    assert np.array_equal(got.orbits, tg.tile_nodes(want.orbits, C))
    assert np.array_equal(got.noninduced, tg.tile_nodes(want.noninduced, C))
    assert np.array_equal(got.arc_triangles, want.arc_triangles[arc_src])


@pytest.mark.parametrize('C', COPIES)
def test_square_clustering_oracle_on_the_tiling(C):
    m = tg.motif('squares')
    Q, P, C4 = sq.square_clustering(m.row_ptr, m.col)
    _, row_ptr, col, _, _ = tg.tile(m.row_ptr, m.col, C)
    rows = np.concatenate([np.arange(0, m.n * C, 7), np.nonzero(np.diff(row_ptr) > 50)[0]])   # a sample and every hub
    q, p, c4 = sq.square_clustering(row_ptr, col, rows)
    assert np.array_equal(q, tg.tile_nodes(Q, C)[rows]) and np.array_equal(p, tg.tile_nodes(P, C)[rows])
    assert c4.tobytes() == tg.tile_nodes(C4, C)[rows].tobytes()
    assert np.array_equal(sq.wedge_counts(row_ptr, col), tg.tile_nodes(sq.wedge_counts(m.row_ptr, m.col), C))


@pytest.mark.parametrize('C', COPIES)
def test_biconnected_oracle_on_the_tiling(C):
    m = tg.motif('structural')
    want = bo.biconnected(m.row_ptr, m.col)
    _, row_ptr, col, _, _ = tg.tile(m.row_ptr, m.col, C)
    got = bo.biconnected(row_ptr, col)
    assert np.array_equal(got.count, tg.tile_nodes(want.count, C))
    assert np.array_equal(got.parent, tg.tile_ids(want.parent, C))
    assert np.array_equal(got.label, tg.tile_ids(want.label, C))           # a label is the smallest row of its set
    assert got.n_components == C * want.n_components
    assert np.array_equal(got.level, tg.tile_nodes(want.level, C))


@pytest.mark.parametrize('kind', ['ints', 'dyadic', 'uniform', 'directed'])
@pytest.mark.parametrize('C', COPIES)
def test_weighted_distance_oracle_on_the_tiling(C, kind):
    m = tg.motif(kind)
    pull = m.inn if m.inn is not None else (m.row_ptr, m.col, m.w)
    _, row_ptr, col, w, _ = tg.tile(pull[0], pull[1], C, pull[2])
    sources = tg.spread_sources(m.n, C, 20, seed=C)
    for batch in (16, 64):
        want = tg.tiled_weighted_distances(lambda js: so.weighted_distances(*pull, js, batch), m.n, C, sources)
        got = so.weighted_distances(row_ptr, col, w, sources, batch)
        for name, g, x in zip(('reach', 'dsum', 'harmonic', 'far', 'source_ecc', 'dist'), got, want):
            assert g.dtype == x.dtype and g.tobytes() == x.tobytes(), (batch, name)
        assert got[6] == want[6], batch
    assert np.isinf(got[5]).sum() >= 20 * m.n * (C - 1)


@pytest.mark.parametrize('kind', ['dyadic', 'uniform', 'directed'])
@pytest.mark.parametrize('C', COPIES)
def test_weighted_betweenness_oracle_on_the_tiling(C, kind):
    m = tg.motif(kind)
    out = (m.row_ptr, m.col, m.w)
    inn = m.inn if m.inn is not None else out
    tiled = [tg.tile(a[0], a[1], C, a[2])[1:4] for a in (out, inn)]
    sources = tg.spread_sources(m.n, C, 20, seed=C)
    hub = 32 * 4
    for endpoints in (False, True):
        for batch in (16, 64):
            want = tg.tiled_betweenness(lambda js: wo.betweenness_arrays(out, inn, js, endpoints, 0.25, batch, hub, hub),
                                        m.n, C, sources)
            got = wo.betweenness_arrays(tiled[0], tiled[1], sources, endpoints, 0.25, batch, hub, hub)
            assert got[0].tobytes() == want[0].tobytes(), (endpoints, batch)
            assert got[1:] == want[1:], (endpoints, batch)
    assert np.count_nonzero(got[0]) > 0


@pytest.mark.parametrize('C', COPIES)
def test_eccentricity_oracle_on_the_tiling(C):
    m = tg.motif('structural')
    _, row_ptr, col, _, _ = tg.tile(m.row_ptr, m.col, C)
    first, second = tg.spread_sources(m.n, C, 70, seed=1), tg.spread_sources(m.n, C, 30, seed=2)

    def solve(js, lower, upper, want_upper=True):
        return eo.eccentricity_pass(m.row_ptr, m.col, js, lower, upper, want_upper=want_upper)

    want1 = tg.tiled_eccentricity(solve, m.n, C, first, want_upper=True)
    got1 = eo.eccentricity_pass(row_ptr, col, first, want_upper=True)
    want2 = tg.tiled_eccentricity(solve, m.n, C, second, want1[2], want1[3])
    got2 = eo.eccentricity_pass(row_ptr, col, second, got1[2], got1[3])
    plain = tg.tiled_eccentricity(lambda js, lo, up: solve(js, lo, up, False), m.n, C, first)
    for got, want in ((got1, want1), (got2, want2), (eo.eccentricity_pass(row_ptr, col, first), plain)):
        for name, g, x in zip(('source_ecc', 'reach', 'lower', 'upper'), got, want):
            assert (g is None and x is None) or (g.dtype == x.dtype and np.array_equal(g, x)), name
    assert plain[3] is None and np.any(want2[3] < want1[3])


# --------------------------------------------------------------------------- the vectorised restatements of two oracles
def test_neighbor_roles_by_row_length_has_the_bits_of_the_oracle():
    m = tg.motif('long_stars')
    n, row_ptr, col, w, _ = tg.tile(m.row_ptr, m.col, 2, m.w)
    for r in (1, 5):
        P = nso.memberships(n, r)
        for weights in (None, w):
            for mode in ('sum', 'mean'):
                want = nso.neighbor_roles(row_ptr, col, weights, P, mode)
                assert tg.neighbor_roles(row_ptr, col, weights, P, mode).tobytes() == want.tobytes(), (r, mode)
    assert np.count_nonzero(np.diff(row_ptr) > nso.LONG_ROW) == 4 and np.count_nonzero(np.diff(row_ptr) == 0) >= 4


def test_similar_rows_for_many_queries_has_the_bits_of_the_oracle():
    X, Q = sim.memberships(70, 3, seed=1), sim.memberships(300, 3, seed=2)
    for metric in sim.METRICS:
        for k in (10, 33, 80):
            want = sim.similar_rows(X, Q, None, k, metric)
            got = tg.similar_rows_many_queries(X, Q, k, metric)
            assert got[0].dtype == np.int32 and got[0].tobytes() == want[0].tobytes(), (metric, k)
            assert got[1].tobytes() == want[1].tobytes(), (metric, k)


# -------------------------------------------------------------------------------------- the caps, read from the sources
CAPS = {
    'grx_peel.h': ('PL_BLOCK', 'PL_SWEEP_MAX_WG'),
    'grx_truss.hip': ('TR_PEEL_MAX_WG',),
    'grx_graphlets.hip': ('GL_K4_MAX_WG',),
    'grx_square_clustering.hip': ('SQ_WAVE_MAX_WG', 'SQ_LDS_MAX_WG', 'SQ_DENSE_WG', 'SQ_WAVE_MAX_WEDGES',
                                  'SQ_LDS_MAX_WEDGES'),
    'grx_biconnected.hip': ('BC_BLOCK', 'BC_MAX_BLOCKS'),
    'grx_relax.h': ('SP_BLOCK', 'SP_MAX_ROW_BLOCKS'),
    'grx_sssp.hip': ('SP_MAX_BLOCKS',),
    'grx_weighted_betweenness.hip': ('WB_BLOCK', 'WB_MAX_ROW_BLOCKS', 'WB_MAX_BLOCKS'),
    'grx_betweenness.hip': ('BW_BLOCK', 'BW_MAX_ROW_BLOCKS'),
    'grx_brandes.h': ('BR_BLOCK', 'BR_MAX_BLOCKS'),
    'grx_closeness.hip': ('CL_BLOCK', 'CL_MAX_ROW_BLOCKS'),
    'grx_neighbor_sense.hip': ('NS_BLOCK', 'NS_MAX_WG', 'NS_LONG_MAX_WG', 'NS_LONG_ROW'),
    'grx_rowjoin.h': ('RJ_BLOCK', 'RJ_ROW_MAX_WG', 'RJ_ARC_MAX_WG'),
    'grx_similarity.hip': ('SIM_BLOCK',),
}

#: the launches whose items per workgroup or cap is not one of the named constants alone: the text of the launch itself
LAUNCHES = {
    'grx_peel.h': ('grx_grid(count, PL_BLOCK, PL_SWEEP_MAX_WG)',),
    'grx_truss.hip': ('grx_grid(m, RJ_BLOCK / L, TR_PEEL_MAX_WG)', 'grx_grid(n, RJ_BLOCK / L, RJ_ROW_MAX_WG)'),
    'grx_rowjoin.h': ('grx_grid(c.n, RJ_BLOCK / L, RJ_ROW_MAX_WG)', 'grx_grid(c.nnz, RJ_BLOCK / L, RJ_ARC_MAX_WG)'),
    'grx_graphlets.hip': ('grx_grid(c.nnz, RJ_BLOCK, RJ_ROW_MAX_WG)', 'grx_grid(n, RJ_BLOCK, RJ_ROW_MAX_WG)',
                          'grx_grid(n, RJ_BLOCK / L, RJ_ROW_MAX_WG)', 'grx_grid(c.nnz, RJ_BLOCK / L, RJ_ARC_MAX_WG)',
                          'grx_grid(c.nnz, RJ_BLOCK / L, GL_K4_MAX_WG)'),
    'grx_square_clustering.hip': ('grx_grid(n, RJ_BLOCK / L, RJ_ROW_MAX_WG)', 'grx_grid(n, GRX_WAVE, SQ_WAVE_MAX_WG)',
                                  'grx_grid(n, 256, SQ_LDS_MAX_WG)', 'grx_grid(n, 1024, SQ_DENSE_WG)'),
    'grx_biconnected.hip': ('grx_grid(n, BC_BLOCK, BC_MAX_BLOCKS)',),
    'grx_relax.h': ('grx_grid(n, SP_BLOCK / S, SP_MAX_ROW_BLOCKS)',),
    'grx_sssp.hip': ('grx_grid(n, SP_BLOCK, SP_MAX_BLOCKS)', 'grx_grid(n, SP_BLOCK / S, SP_MAX_BLOCKS)',
                     'grx_grid(n, GRX_WAVE, SP_MAX_BLOCKS)'),
    'grx_weighted_betweenness.hip': ('grx_grid(n, WB_BLOCK / S, WB_MAX_ROW_BLOCKS)',
                                     'grx_grid(cells, WB_BLOCK, WB_MAX_BLOCKS)',
                                     'grx_grid(n, WB_BLOCK / S, WB_MAX_BLOCKS)'),
    'grx_betweenness.hip': ('grx_grid(n, BW_WAVES, BW_MAX_ROW_BLOCKS)', 'grx_grid(cells, BW_BLOCK, BW_MAX_BLOCKS)'),
    'grx_brandes.h': ('grx_grid(n, BR_BLOCK, BR_MAX_BLOCKS)',),     # the accumulation and the scale of all four entries
    'grx_closeness.hip': ('grx_grid(n, CL_BLOCK / W, CL_MAX_ROW_BLOCKS)',    # the one level launch of the three users
                          'grx_grid(a.n, CL_BLOCK, CL_MAX_BLOCKS)'),         # grx_distance_sums' per-node rounding
    'grx_neighbor_sense.hip': ('grx_grid(A.n, NS_BLOCK / (S * CL), NS_MAX_WG)',
                               'grx_grid(A.n, NS_BLOCK, NS_LONG_MAX_WG)'),
    'grx_similarity.hip': ('grx_grid(nq * k, SIM_BLOCK, 2048)', 'grx_grid(n, SIM_BLOCK, 2048)',
                           'grx_grid(nq, SIM_BLOCK, 2048)'),
    'grx_transform.hip': ('grx_grid(n, TR_BLOCK, TR_MAX_GRID)',),
}


def test_the_mirrored_caps_are_the_ones_in_the_sources():
    from graphrole_amd import kernels as K
    for name, constants in CAPS.items():
        text = _source(name)
        for constant in constants:
            found = re.findall(r'\b' + constant + r' = (\d+)[;,]', text)
            assert len(found) == 1 and int(found[0]) == getattr(K, constant), (name, constant, found)
    common, transform = _source('grx_common.h'), _source('grx_transform.hip')
    num_cu = int(re.search(r'constexpr int GRX_NUM_CU = (\d+);', common).group(1))
    assert int(re.search(r'constexpr int GRX_WAVE = (\d+);', common).group(1)) == 64
    assert int(re.search(r'constexpr int TR_BLOCK = (\d+);', transform).group(1)) == K.TRANSFORM_BLOCK
    factor = int(re.search(r'constexpr int TR_MAX_GRID = GRX_NUM_CU \* (\d+);', transform).group(1))
    assert num_cu * factor == K.TRANSFORM_MAX_GRID
    assert K.SIM_ROW_MAX_WG == 2048                             # the literal of the three launches below
    for name, launches in LAUNCHES.items():
        text = _source(name)
        for launch in launches:
            assert launch in text, (name, launch)
    # every grx_grid of these files is one of the launches above: a new capped launch has to be listed (and wrapped)
    for name, launches in LAUNCHES.items():
        for call in re.findall(r'grx_grid\((?:[^()]|\([^()]*\))*\)', _source(name)):
            assert call in launches, (name, call)
