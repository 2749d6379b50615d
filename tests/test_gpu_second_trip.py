"""
The second trip of every capped grid-stride launch of the measures added after the 1 M full-size tests, on the MI355X.

A launch sized by grx_grid(items, per_block, cap) takes a second trip of its loop only when items > cap * per_block.
Below that a wrong stride, a barrier inside a loop whose trip count differs between lanes, a per-workgroup partial that
is overwritten instead of accumulated and LDS state that is not reset between trips cannot show.  Every test here runs
one entry point on C interleaved copies of a small motif (tests/tiled_graphs.py; n = n0 * C just above 5 / 4 of 2048 *
256 rows, so that the second trip of the launches capped at 2048 * 256 items takes a fifth of the rows, every motif row
among them, not the last few labels alone), or on a random table of 2048 * 256 + 77 rows where the operation has no
graph, and

* starts by asserting, from the copies of the caps in graphrole_amd/kernels.py (checked against the sources by
  tests/test_tiled_graphs_cpu.py), that each of its launches wraps at the lane width, batch or words it passes -- the
  assertions are the list of what is covered;
* compares every output that the measure's own kernel-against-oracle test compares, in the same way and under the same
  tolerance, with the motif's oracle answer tiled (tests/test_tiled_graphs_cpu.py proves that construction);
* asserts the bytes of the kernel's own one-trip run on the motif alone, tiled, with the same lanes / batch / words.

Not wrapped here: ms_level (the level kernel of grx_closeness.hip, run here with grx_eccentricity's bodies) with
words = 1 needs more than 8192 * 256 = 2 M rows, above the size limit of this file (2^21 rows); words = 16 wraps the
same kernels above 131 072 rows.  The other second-trip tests of the suite:
measures_oracle.GRAPHS['rows32' | 'rows4' | 'elements'], test_second_trip_of_the_grid_stride_loops in
test_gpu_clustering.py and test_gpu_structural_holes.py, aggx_oracle.LENGTHS, and the full-size tests (ReFeX, closeness,
betweenness, k-core, role rows).
"""
import functools

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

pytestmark = pytest.mark.gpu

ROWS = 2048 * 256                                               # every tiling has 5 / 4 of this many rows
EXTRA = 77                                                      # and the tables ROWS + EXTRA


def _wraps(items, per_block, cap):
    return items > cap * per_block


@functools.lru_cache(maxsize=None)
def _tiled(kind, inn=False):
    """(motif, C, n, row_ptr, col, w, arc_src) of the tiling of motif(kind) -- of its in-adjacency with `inn`."""
    m = tg.motif(kind)
    C = tg.copies_for(m.n, ROWS + ROWS // 4)
    a = m.inn if inn else (m.row_ptr, m.col, m.w)
    n, row_ptr, col, w, arc_src = tg.tile(a[0], a[1], C, a[2])
    assert ROWS + ROWS // 4 < n <= ROWS + ROWS // 4 + m.n and n < 1 << 21
    return m, C, n, row_ptr, col, w, arc_src


def _pair(K, kind, inn=False):
    """(the tiling's tuple, DeviceCSR of the tiling, DeviceCSR of the motif): the same lanes, hub rows in both."""
    t = _tiled(kind, inn)
    m = t[0]
    a = m.inn if inn else (m.row_ptr, m.col, m.w)
    big, small = K.DeviceCSR(t[3], t[4], t[5]), K.DeviceCSR(*a)
    assert big.n_hubs == t[1] * small.n_hubs > 0 and big.lanes_per_row == small.lanes_per_row
    return t, big, small


# ------------------------------------------------------------------------------------------------------------ truss
def test_truss_numbers():
    from graphrole_amd import kernels as K
    (m, C, n, row_ptr, col, _, arc_src), big, small = _pair(K, 'structural')
    nnz = len(col)
    want = to.truss_numbers(m.row_ptr, m.col)
    assert want.n_levels > 1 and want.n_rounds > 3
    for lanes in (32, big.lanes_per_row):
        assert _wraps(nnz, K.PL_BLOCK, K.PL_SWEEP_MAX_WG)                       # pl_min, pl_collect over the arcs
        assert _wraps(nnz // 2, K.RJ_BLOCK // lanes, K.TR_PEEL_MAX_WG)          # tr_peel<L>
        assert _wraps(n, K.RJ_BLOCK // lanes, K.RJ_ROW_MAX_WG)                  # rj_rows<L>: support and node truss
        assert _wraps(nnz, K.RJ_BLOCK // lanes, K.RJ_ARC_MAX_WG)                # rj_arc<L>
        arc, node, n_rounds, n_levels = K.truss_numbers(big, lanes=lanes)
        arc, node = K.to_host(arc)[:nnz], K.to_host(node)[:n]
        assert arc.dtype == np.int32 and node.dtype == np.int64
        assert np.array_equal(arc, want.arc_truss[arc_src]), lanes
        assert np.array_equal(node, tg.tile_nodes(want.node_truss, C)), lanes
        assert (n_rounds, n_levels) == (want.n_rounds, want.n_levels), lanes
        arc0, node0, rounds0, levels0 = K.truss_numbers(small, lanes=lanes)
        assert arc.tobytes() == K.to_host(arc0)[:small.nnz][arc_src].tobytes(), lanes
        assert node.tobytes() == tg.tile_nodes(K.to_host(node0)[:m.n], C).tobytes(), lanes
        assert (n_rounds, n_levels) == (rounds0, levels0), lanes


# -------------------------------------------------------------------------------------------------------- graphlets
def test_graphlet_orbits():
    from graphrole_amd import kernels as K
    (m, C, n, row_ptr, col, _, arc_src), big, small = _pair(K, 'structural')
    nnz = len(col)
    want = go.orbits(m.row_ptr, m.col)
    assert np.all(want.orbits.max(axis=1) > 0)                  # every orbit occurs in the motif
    for lanes in (32, big.lanes_per_row):
        assert _wraps(nnz, K.RJ_BLOCK, K.RJ_ROW_MAX_WG)                         # gl_mirror
        assert _wraps(n, K.RJ_BLOCK, K.RJ_ROW_MAX_WG)                           # gl_finish
        assert _wraps(n, K.RJ_BLOCK // lanes, K.RJ_ROW_MAX_WG)                  # rj_rows<L>, pass a and pass b
        assert _wraps(nnz, K.RJ_BLOCK // lanes, K.RJ_ARC_MAX_WG)                # rj_arc<L>, gl_diamond<L>
        assert _wraps(nnz, K.RJ_BLOCK // lanes, K.GL_K4_MAX_WG)                 # gl_k4<L>
        orbits, non, tri = K.graphlet_orbits(big, want_noninduced=True, want_arc_triangles=True, lanes=lanes)
        orbits, non, tri = K.to_host(orbits), K.to_host(non), K.to_host(tri)[:nnz]
        assert orbits.dtype == np.int64 and non.dtype == np.int64 and tri.dtype == np.int32
        assert orbits.shape == (15, n) and non.shape == (15, n)
        assert np.array_equal(tri, want.arc_triangles[arc_src]), lanes
        assert np.array_equal(non, tg.tile_nodes(want.noninduced, C)), lanes
        assert np.array_equal(orbits, tg.tile_nodes(want.orbits, C)), lanes
        orbits0, non0, tri0 = K.graphlet_orbits(small, want_noninduced=True, want_arc_triangles=True, lanes=lanes)
        assert orbits.tobytes() == tg.tile_nodes(K.to_host(orbits0), C).tobytes(), lanes
        assert non.tobytes() == tg.tile_nodes(K.to_host(non0), C).tobytes(), lanes
        assert tri.tobytes() == K.to_host(tri0)[:small.nnz][arc_src].tobytes(), lanes


# ------------------------------------------------------------------------------------------------ square clustering
def test_square_clustering():
    from graphrole_amd import kernels as K
    (m, C, n, row_ptr, col, _, _), big, small = _pair(K, 'squares')
    wedges = sq.wedge_counts(m.row_ptr, m.col)
    Q, P, C4 = sq.square_clustering(m.row_ptr, m.col)
    wave = (wedges > 0) & (wedges <= K.SQ_WAVE_MAX_WEDGES)
    lds = (wedges > K.SQ_WAVE_MAX_WEDGES) & (wedges <= K.SQ_LDS_MAX_WEDGES)
    dense = wedges > K.SQ_LDS_MAX_WEDGES
    # rows of every tier on squares; the dense tier has more rows than workgroups, so one workgroup counts several
    assert np.count_nonzero(Q[wave]) > 100 and np.all(Q[lds] > 0) and np.all(Q[dense] > 0)
    assert wave.sum() * C > K.SQ_WAVE_MAX_WG and lds.sum() * C > 0 and dense.sum() * C > K.SQ_DENSE_WG
    assert _wraps(n, 64, K.SQ_WAVE_MAX_WG)                                      # sq_count, wave tier
    assert _wraps(n, 256, K.SQ_LDS_MAX_WG)                                      # sq_count, LDS tier
    assert _wraps(n, 1024, K.SQ_DENSE_WG)                                       # sq_count, dense tier
    for lanes in (32, big.lanes_per_row):
        assert _wraps(n, K.RJ_BLOCK // lanes, K.RJ_ROW_MAX_WG)                  # rj_rows<L>
        c, q, p = (K.to_host(x)[:n] for x in K.square_clustering(big, want_counts=True, lanes=lanes))
        assert np.array_equal(q, tg.tile_nodes(Q, C)), (lanes, 'squares')
        assert np.array_equal(p, tg.tile_nodes(P, C)), (lanes, 'potential')
        assert c.tobytes() == tg.tile_nodes(C4, C).tobytes(), (lanes, 'square clustering')
        c0, q0, p0 = (K.to_host(x)[:m.n] for x in K.square_clustering(small, want_counts=True, lanes=lanes))
        assert q.tobytes() == tg.tile_nodes(q0, C).tobytes() and p.tobytes() == tg.tile_nodes(p0, C).tobytes()
        assert c.tobytes() == tg.tile_nodes(c0, C).tobytes(), lanes


# ------------------------------------------------------------------------------------------------------ biconnected
def _same_partition(a, b):
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)
    return len(pairs) == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1])), len(pairs)


def test_biconnected():
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    from graphrole_amd import kernels as K
    (m, C, n, row_ptr, col, _, _), big, small = _pair(K, 'structural')
    assert _wraps(n, K.BC_BLOCK, K.BC_MAX_BLOCKS)                               # every egrid kernel
    want = bo.biconnected(m.row_ptr, m.col)
    count, parent, label, n_components = K.biconnected(big)
    count, parent, label = (K.to_host(t)[:n] for t in (count, parent, label))
    assert count.dtype == np.int64 and parent.dtype == np.int32 and label.dtype == np.int32
    want_parent = tg.tile_ids(want.parent, C)
    assert np.array_equal(count, tg.tile_nodes(want.count, C))
    assert np.array_equal(parent, want_parent)                  # the same stated parent rule
    assert n_components == C * want.n_components
    # labels up to renaming: the same partition of the non-root vertices, -1 exactly for the roots
    assert np.array_equal(label < 0, want_parent < 0)
    same, classes = _same_partition(label, tg.tile_ids(want.label, C))
    assert same and classes - bool((label < 0).any()) == n_components
    # a valid BFS forest: the roots are the smallest id of each connected component, every parent one level nearer
    _, comp = connected_components(csr_matrix((np.ones(len(col)), col, row_ptr), shape=(n, n)), directed=False)
    smallest = np.full(comp.max() + 1, n)
    np.minimum.at(smallest, comp, np.arange(n))
    assert np.array_equal(np.nonzero(parent < 0)[0], np.sort(smallest))
    level, nonroot = tg.tile_nodes(want.level, C), parent >= 0
    assert np.array_equal(level[parent[nonroot]], level[nonroot] - 1)
    assert np.all(comp[parent[nonroot]] == comp[nonroot])
    # the one-trip run on the motif, tiled
    count0, parent0, label0, components0 = K.biconnected(small)
    assert count.tobytes() == tg.tile_nodes(K.to_host(count0)[:m.n], C).tobytes()
    assert parent.tobytes() == tg.tile_ids(K.to_host(parent0)[:m.n], C).tobytes()
    assert _same_partition(label, tg.tile_ids(K.to_host(label0)[:m.n], C))[0]   # whatever names the labels have
    assert n_components == C * components0
    count3, parent3, label3, n3 = K.biconnected(big, want_forest=False)
    assert parent3 is None and label3 is None and n3 == n_components
    assert K.to_host(count3)[:n].tobytes() == count.tobytes()


# ----------------------------------------------------------------------------------------------- weighted distances
WD_NAMES = ('reach', 'dsum', 'harmonic', 'far', 'source_ecc', 'dist')


@pytest.mark.parametrize('kind', ['uniform', 'directed'])
def test_weighted_distances(kind):
    from graphrole_amd import kernels as K
    directed = kind == 'directed'
    (m, C, n, row_ptr, col, w, _), big, small = _pair(K, kind, inn=directed)
    pull = m.inn if directed else (m.row_ptr, m.col, m.w)
    sources = tg.spread_sources(m.n, C, 20, seed=5)
    assert sources.max() > ROWS and len(set((sources % C).tolist())) == 3       # a source in the second trip
    assert _wraps(n, K.SP_BLOCK, K.SP_MAX_BLOCKS)                               # sp_finish

    def device(csr, rows, batch, want_matrix):
        reach, dsum, harmonic, far, ecc, dist, rounds = K.weighted_distances(csr, rows, batch, want_matrix)
        return tuple(K.to_host(t)[:csr.n] for t in (reach, dsum, harmonic, far)) + (
            K.to_host(ecc), K.to_host(dist) if want_matrix else None, rounds)

    for batch in (16, 64):
        want_matrix = batch == 16                               # 20 x n doubles
        assert len(sources) > 16 and len(sources) % 16          # batch 16: two batches, the second partial
        assert _wraps(n, K.SP_BLOCK // batch, K.SP_MAX_ROW_BLOCKS)              # sp_round<S>
        assert _wraps(n, K.SP_BLOCK // batch, K.SP_MAX_BLOCKS)                  # sp_source<S>
        assert _wraps(n, 64, K.SP_MAX_BLOCKS)                                   # sp_matrix<S>
        got = device(big, sources, batch, want_matrix)
        want = tg.tiled_weighted_distances(lambda js: so.weighted_distances(*pull, js, batch), m.n, C, sources)
        alone = tg.tiled_weighted_distances(lambda js: device(small, js, batch, want_matrix), m.n, C, sources)
        for name, g, x, a in zip(WD_NAMES, got, want, alone):
            if name == 'dist' and not want_matrix:
                assert g is None
                continue
            assert g.dtype == x.dtype and g.tobytes() == x.tobytes(), (batch, name, np.nonzero(g != x))
            assert g.tobytes() == a.tobytes(), (batch, name, 'the motif alone')
        assert got[6] == want[6] == alone[6], batch             # Jacobi rounds
        if want_matrix:
            assert got[5].shape == (20, n) and np.isinf(got[5]).sum() >= 20 * (n - m.n)
    assert got[0].max() > 0 and np.count_nonzero(got[0]) <= 3 * m.n             # three copies reached, the others not


# --------------------------------------------------------------------------------------------- weighted betweenness
@pytest.mark.parametrize('kind', ['dyadic', 'directed'])
def test_weighted_betweenness(kind):
    from graphrole_amd import kernels as K
    directed = kind == 'directed'
    (m, C, n, _, _, _, _), big, small = _pair(K, kind)
    big_in = small_in = None
    inn = out = (m.row_ptr, m.col, m.w)
    if directed:
        _, big_in, small_in = _pair(K, kind, inn=True)
        inn = m.inn
    sources = tg.spread_sources(m.n, C, 20, seed=6)
    assert sources.max() > ROWS and len(set((sources % C).tolist())) == 3
    hub_out = K.HUB_FACTOR * small.lanes_per_row
    hub_in = K.HUB_FACTOR * (small_in if directed else small).lanes_per_row
    assert _wraps(n, K.BR_BLOCK, K.BR_MAX_BLOCKS)                               # br_accumulate, br_scale

    def device(csr, csr_in, rows, endpoints, batch):
        bc, rounds, levels = K.weighted_betweenness(csr, csr_in, rows, endpoints, 0.25, batch)
        return K.to_host(bc)[:csr.n], rounds, levels

    for batch in (16, 64):
        assert _wraps(n, K.SP_BLOCK // batch, K.SP_MAX_ROW_BLOCKS)              # sp_round<S>
        assert _wraps(n, K.WB_BLOCK // batch, K.WB_MAX_ROW_BLOCKS)              # the forward and backward row kernels
        assert _wraps(n * batch, K.WB_BLOCK, K.WB_MAX_BLOCKS)                   # wb_depth_init
        assert _wraps(n, K.WB_BLOCK // batch, K.WB_MAX_BLOCKS)                  # wb_reach<S>
        for endpoints in (False, True):
            got = device(big, big_in, sources, endpoints, batch)
            want = tg.tiled_betweenness(
                lambda js: wo.betweenness_arrays(out, inn, js, endpoints, 0.25, batch, hub_out, hub_in), m.n, C, sources)
            alone = tg.tiled_betweenness(lambda js: device(small, small_in, js, endpoints, batch), m.n, C, sources)
            assert got[0].dtype == np.float64
            np.testing.assert_allclose(got[0], want[0], rtol=wo.RTOL, atol=0, err_msg=str((batch, endpoints)))
            assert got[1:] == want[1:], (batch, endpoints)      # relaxation rounds, deepest level
            assert got[0].tobytes() == alone[0].tobytes() and got[1:] == alone[1:], (batch, endpoints)
    assert np.count_nonzero(got[0]) > 0


# ----------------------------------------------------------------------------------------------------- eccentricity
def test_eccentricity_pass():
    """words = 16: ms_level<16, Body> takes 256 / 16 rows a workgroup and wraps above 131 072 rows -- without the
    bounds (no upper), with them (want_upper), and continuing from carried bounds.  words = 1 would need more than
    2 M rows and stays out."""
    from graphrole_amd import kernels as K
    (m, C, n, row_ptr, col, _, _), big, small = _pair(K, 'structural')
    words = 16
    assert _wraps(n, K.CL_BLOCK // words, K.CL_MAX_ROW_BLOCKS)                  # ms_level<W, ec_reach>, <W, ec_bounds>
    first, second = tg.spread_sources(m.n, C, 70, seed=1), tg.spread_sources(m.n, C, 30, seed=2)
    assert first.max() > ROWS and second.max() > ROWS

    def host(out, rows):
        ecc, reach, lower, upper = out
        return (K.to_host(ecc), K.to_host(reach)[:rows], K.to_host(lower)[:rows],
                None if upper is None else K.to_host(upper)[:rows])

    def oracle(want_upper):
        return lambda js, lo, up: eo.eccentricity_pass(m.row_ptr, m.col, js, lo, up, want_upper=want_upper)

    def alone(want_upper):
        def solve(js, lo, up):
            bounds = None if lo is None else (K.to_device(lo), None if up is None else K.to_device(up))
            return host(K.eccentricity_pass(small, js, words, bounds=bounds, want_upper=want_upper), m.n)
        return solve

    def same(got, want, what):
        for name, g, x in zip(('source_ecc', 'reach', 'lower', 'upper'), got, want):
            if x is None:
                assert g is None, (what, name)
                continue
            assert g.dtype == x.dtype and np.array_equal(g, x), (what, name, np.nonzero(g != x)[0][:8])

    out1 = K.eccentricity_pass(big, first, words, want_upper=True)              # accumulate = 0, both passes
    got1 = host(out1, n)
    want1 = tg.tiled_eccentricity(oracle(True), m.n, C, first, want_upper=True)
    same(got1, want1, 'first call')
    same(got1, tg.tiled_eccentricity(alone(True), m.n, C, first, want_upper=True), 'first call, the motif alone')
    got2 = host(K.eccentricity_pass(big, second, words, bounds=(out1[2], out1[3])), n)      # accumulate = 1
    same(got2, tg.tiled_eccentricity(oracle(True), m.n, C, second, want1[2], want1[3]), 'second call')
    same(got2, tg.tiled_eccentricity(alone(True), m.n, C, second, want1[2], want1[3]), 'second call, the motif alone')
    assert np.all(got2[2] >= got1[2]) and np.all(got2[3] <= got1[3]) and np.any(got2[3] < got1[3])
    got3 = host(K.eccentricity_pass(big, first, words), n)                      # no upper: no second pass
    assert got3[3] is None
    same(got3, tg.tiled_eccentricity(oracle(False), m.n, C, first), 'without upper')
    same(got3, tg.tiled_eccentricity(alone(False), m.n, C, first), 'without upper, the motif alone')


# -------------------------------------------------------------------------------------------------- neighbour roles
def test_neighbor_roles():
    """P is random memberships of all n rows, not tiled: the expected value is the oracle's summation on the tiling
    itself (tiled_graphs.neighbor_roles: its bits without a loop over the rows)."""
    from graphrole_amd import kernels as K
    m, C, n, row_ptr, col, w, _ = _tiled('long_stars')
    r = 5
    deg = np.diff(row_ptr)
    long_rows = np.nonzero(deg > K.NS_LONG_ROW)[0]
    assert K.NS_LONG_ROW == nso.LONG_ROW and len(long_rows) == 2 * C
    assert _wraps(n, K.NS_BLOCK, K.NS_LONG_MAX_WG)                              # ns_long_rows
    second_trip = K.NS_LONG_MAX_WG * K.NS_BLOCK
    assert np.count_nonzero(long_rows < second_trip) == C and np.count_nonzero(long_rows >= second_trip) == C
    lanes_offered = K.neighbor_lanes(r)
    assert max(lanes_offered) == 32 and all(_wraps(n, K.NS_BLOCK // lanes, K.NS_MAX_WG) for lanes in lanes_offered)
    csr = K.DeviceCSR(row_ptr, col, w)
    padded = nso.memberships(n, r, ld=r + 3)
    P = np.ascontiguousarray(padded[:, :r])
    Pd, Pp = K.to_device(P), K.to_device(padded)
    for weights, wd in ((None, None), (w, csr.w)):
        for mode in ('sum', 'mean'):
            what = (weights is not None, mode)
            want = tg.neighbor_roles(row_ptr, col, weights, P, mode)
            assert np.all(np.isfinite(want)) and np.all(want[:, deg == 0] == 0.0) and deg.min() == 0
            for lanes in (0,) + lanes_offered:                                  # ns_rows<S, CL> for S = 8, 1, 2, 4, 8
                got = K.to_host(K.neighbor_roles(csr, Pd, mode, wd, lanes=lanes))
                assert got.shape == want.shape and got.tobytes() == want.tobytes(), what + (lanes,)
            got = K.to_host(K.neighbor_roles(csr, Pp, mode, wd, r=r))
            assert got.tobytes() == want.tobytes(), what + ('ld = r + 3',)


# ---------------------------------------------------------------------------------------------------- similar rows
def _similar(K, got, want, what):
    index, score = (np.asarray(K.to_host(t)) for t in got)
    assert index.dtype == np.int32 and score.dtype == np.float64 and index.shape == want[0].shape, what
    assert index.tobytes() == want[0].tobytes(), (what, 'index')
    assert score.tobytes() == want[1].tobytes(), (what, 'score')


@pytest.mark.parametrize('c', [3, 7])
def test_similar_rows_many_candidates(c):
    """sim_prepare of X wraps.  Only the last 77 rows of X are prepared in the second trip, so the queries are made for
    them: two rows of X that leave themselves out (one of each trip), two rows next to rows of the second trip -- each
    has its nearest candidate there under both metrics -- and one row of its own."""
    from graphrole_amd import kernels as K
    n = ROWS + EXTRA
    assert _wraps(n, K.SIM_BLOCK, K.SIM_ROW_MAX_WG)                             # sim_prepare (X)
    X = sim.memberships(n, c, seed=1)
    own = np.array([5, n - 3])                                  # one in the first trip, one in the second
    near = (np.nonzero(np.all(X[ROWS:] > 0, axis=1))[0] + ROWS)[[0, -1]]          # no zero entry: no exact cosine tie
    Q = np.concatenate([X[own], X[near] * (1.0 + 1e-9 * np.arange(1, c + 1)), sim.memberships(1, c, seed=2)])
    self_rows = np.array([own[0], own[1], -1, -1, -1], dtype=np.int32)
    Xd, Qd, Sd = K.to_device(X), K.to_device(Q), K.to_device(self_rows)
    for metric in sim.METRICS:
        for k in (10, 33):                                      # both selection-list widths
            assert k <= K.SIM_SMALL_K or k == 33
            want = sim.similar_rows(X, Q, self_rows, k, metric)
            assert not np.any(want[0][:2] == own[:, None]) and want[0].min() >= 0
            assert want[0][2:4, 0].tolist() == near.tolist()    # the answer depends on the rows of the second trip
            for segments in (0, 3):
                got = K.similar_rows(Xd, Qd, Sd, k=k, metric=metric, segments=segments, c=c)
                _similar(K, got, want, (c, metric, k, segments))


@pytest.mark.parametrize('metric', sim.METRICS)
def test_similar_rows_many_queries(metric):
    """The converse shape: sim_prepare of Q wraps (ROWS + 77 queries against 70 candidates)."""
    from graphrole_amd import kernels as K
    nq, n, c, k = ROWS + EXTRA, 70, 3, 10
    assert _wraps(nq, K.SIM_BLOCK, K.SIM_ROW_MAX_WG)                            # sim_prepare (Q)
    X, Q = sim.memberships(n, c, seed=1), sim.memberships(nq, c, seed=2)
    want = tg.similar_rows_many_queries(X, Q, k, metric)        # similarity_oracle's bits: test_tiled_graphs_cpu.py
    _similar(K, K.similar_rows(K.to_device(X), K.to_device(Q), k=k, metric=metric, c=c), want, metric)


def test_similar_rows_fill_without_candidates():
    """n = 0: sim_fill writes -1 / NaN into nq * k > 2048 * 256 slots, and nothing behind the k columns."""
    from graphrole_amd import kernels as K
    nq, k, c = 8200, 64, 3
    assert _wraps(nq * k, K.SIM_BLOCK, K.SIM_ROW_MAX_WG)                        # sim_fill
    index = K.to_device(np.full((nq, k + 3), -7, dtype=np.int32))
    score = K.to_device(np.full((nq, k + 3), -7.0))
    K.similar_rows(K.empty((0, c)), K.to_device(sim.memberships(nq, c)), k=k, out=(index, score))
    index, score = K.to_host(index), K.to_host(score)
    assert np.all(index[:, :k] == -1) and np.isnan(score[:, :k]).all()
    assert np.all(index[:, k:] == -7) and np.all(score[:, k:] == -7.0)


# --------------------------------------------------------------------------------------------------- NMF transform
def test_nmf_transform():
    """A random table of ROWS + 77 rows, F = 5, r = 3, with the checks and the tolerance of test_gpu_transform._check:
    a fixed number of iterations with tol = 0, then the default tolerance, where the norm reduction over the wrapped
    per-workgroup partials steers the stopping rule; and the same bits twice."""
    from graphrole_amd import kernels as K
    from tests import test_gpu_transform as tt
    n, F, r = ROWS + EXTRA, 5, 3
    assert _wraps(n, K.TRANSFORM_BLOCK, K.TRANSFORM_MAX_GRID)                   # every row kernel
    X, H = tt._random_case(n, F, r, seed=11)
    W, info = tt._check(X, H, tol=0.0, max_iter=12)
    assert info.n_iter == 12
    W2, info2 = tt._check(X, H)
    assert 10 <= info2.n_iter < 200 and info2.n_iter % 10 == 0                  # stopped by the rule
    W3, info3 = tt._device_transform(X, H)
    assert W3.tobytes() == W2.tobytes() and info3.n_iter == info2.n_iter and info3.err_last == info2.err_last
