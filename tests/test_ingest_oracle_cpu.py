"""
-m "not gpu": the numpy reference of tests/ingest_oracle.py against a list-of-lists construction that shares no code
with it (small cases) and against graphrole_amd/graph/csr.py (CSRGraph + InternalGraph, every case), so that
tests/test_gpu_ingest_kernels.py, tests/test_gpu_ingest.py and the host path are pinned to the same arrays; for every
case the conditions that make it reach what it is listed for; and the workspace contract of grx_ingest /
grx_orient_*, which is checked before any launch.
"""
import ctypes

import numpy as np
import pytest

from tests import ingest_oracle as io

SMALL = [c.name for c in io.CASES if c.small]
UNDIRECTED = [c.name for c in io.CASES if not c.directed]


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and np.array_equal(a, b), what


def _same_bits(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert np.array_equal(io.bits(np.asarray(a, dtype=np.float64)), io.bits(b)), what


def test_case_list_is_what_the_gpu_file_expects():
    assert len(SMALL) >= 50 and set(io.LABEL_ORDER_CASES) <= set(UNDIRECTED)
    for c in io.CASES:
        assert c.props, c.name
        assert c.props <= set(PROPERTY_CHECKS), (c.name, c.props - set(PROPERTY_CHECKS))
    used = set().union(*(c.props for c in io.CASES))
    assert used == set(PROPERTY_CHECKS)                       # no check without a case that claims it


@pytest.mark.parametrize('name', io.CASE_NAMES)
def test_edges_are_unique_and_in_range(name):
    n, src, dst, w, directed = io.graph(name)
    assert src.shape == dst.shape and len(src) >= 1 and src.min() >= 0 and dst.min() >= 0
    assert src.max() < n and dst.max() < n and (w is None or w.shape == src.shape)
    a, b = (src, dst) if directed else (np.minimum(src, dst), np.maximum(src, dst))
    assert len(np.unique(a * n + b)) == len(src)
    assert io.case(name).directed == directed and io.case(name).small == (len(src) <= io.SMALL_EDGES)


@pytest.mark.parametrize('name', SMALL)
def test_reference_equals_the_list_of_lists_construction(name):
    n, src, dst, w, directed = io.graph(name)
    ref, lol = io.expected(name), io.list_of_lists(n, src, dst, w, directed)
    for key in ('perm', 'inv', 'row_ptr', 'col', 'agg_col', 't_row_ptr', 't_col'):
        _same(lol[key], getattr(ref, key), (name, key))
    _same_bits(lol['w'], ref.w, (name, 'w'))
    _same_bits(lol['t_w'], ref.t_w, (name, 't_w'))
    assert ref.nnz == len(lol['col']) == ref.row_ptr[-1]
    if not directed:
        o = io.expected_oriented(name)
        _same(lol['o_row_ptr'], o.row_ptr, (name, 'o_row_ptr'))
        _same(lol['o_col'], o.col, (name, 'o_col'))
        _same(np.array(lol['o_arc'], dtype=np.uint64).view(np.int64) if lol['o_arc'] else np.zeros(0, np.int64), o.arc,
              (name, 'o_arc'))


@pytest.mark.parametrize('name', io.CASE_NAMES)
def test_reference_equals_the_host_construction(name):
    from graphrole_amd.graph.csr import CSRGraph, InternalGraph
    n, src, dst, w, directed = io.graph(name)
    G = CSRGraph(n, src, dst, weights=w, directed=directed)
    host, ref = InternalGraph(G), io.expected(name)
    assert G.nnz == host.nnz == ref.nnz
    for key in ('perm', 'inv', 'row_ptr', 'col', 'agg_col', 't_row_ptr', 't_col'):
        _same(getattr(host, key), getattr(ref, key), (name, key))
    _same_bits(host.w, ref.w, (name, 'w'))
    _same_bits(host.t_w, ref.t_w, (name, 't_w'))
    if name in io.LABEL_ORDER_CASES:
        row_ptr, col, _ = io.label_order(name)
        _same(G.row_ptr, row_ptr, (name, 'label row_ptr'))
        _same(G.col, col, (name, 'label col'))


@pytest.mark.parametrize('name', UNDIRECTED)
def test_oriented_reference_is_consistent(name):
    """Every undirected non-loop edge is kept in exactly one direction, rows stay ascending, and the fields of the
    per-arc word decode to the lists they describe."""
    ref, o = io.expected(name), io.expected_oriented(name)
    n = ref.n
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ref.row_ptr))
    n_loops = int((rows == ref.col).sum())
    assert o.row_ptr[-1] == len(o.col) == len(o.arc) == (ref.nnz - n_loops) // 2
    orow = np.repeat(np.arange(n, dtype=np.int64), np.diff(o.row_ptr))
    assert np.all(np.diff(orow * n + o.col) > 0)
    arc = o.arc.view(np.uint64)
    olen = np.diff(o.row_ptr)
    assert np.array_equal((arc & np.uint64(0xFFFFFFFF)).astype(np.int64), o.row_ptr[o.col])
    assert np.array_equal(((arc >> np.uint64(32)) & np.uint64(1023)).astype(np.int64), np.minimum(olen[o.col], 1023))
    assert np.array_equal(((arc >> np.uint64(42)) & np.uint64(1023)).astype(np.int64), np.minimum(olen[orow], 1023))
    assert np.all((arc >> np.uint64(62)) == 0)


# ---- reach: each case has the property it is listed for -------------------------------------------------------------

def _deg(name):
    return np.diff(io.expected(name).row_ptr)


def _near(x, tile):
    return x % tile in (tile - 1, 0, 1)


def _slots(name):
    n, src, _, _, directed = io.graph(name)
    return len(src) if directed else 2 * len(src)


def _sentinel_share(name):
    n, src, dst, _, directed = io.graph(name)
    return 0.0 if directed else float((src == dst).sum()) / (2 * len(src))


def _reversed_share(name):
    _, src, dst, _, _ = io.graph(name)
    return float((src > dst).sum()) / len(src)


def _check_single_node(name):
    ref = io.expected(name)
    assert ref.n == 1 and ref.m == 1 and ref.nnz == 1 and ref.row_ptr.tolist() == [0, 1] and ref.col.tolist() == [0]


def _check_reversed_edge(name):
    assert _reversed_share(name) > 0


def _check_all_loops(name):
    assert _sentinel_share(name) == 0.5


def _check_loops_even_odd(name):
    _, src, dst, _, _ = io.graph(name)
    at = np.flatnonzero(src == dst)
    assert len(at) == 100 and len(src) == 200 and (at % 2 == 0).sum() >= 40 and (at % 2 == 1).sum() >= 40
    assert 0.2 < _sentinel_share(name) < 0.3


def _check_block_edge(name):
    assert _near(io.expected(name).n, 256)


def _check_scan_tile_edge(name):
    assert _near(io.expected(name).n, io.SCAN_TILE)


def _check_sort_tile_edge(name):
    assert _near(io.expected(name).n, io.SORT_TILE)


def _check_last_tile_single(name):
    assert io.expected(name).n % io.SCAN_TILE == 1


def _check_last_isolated(name):
    ref = io.expected(name)
    assert _deg(name)[-1] == 0 and ref.perm[-1] == ref.n - 1 and ref.row_ptr[-1] == ref.row_ptr[-2]


def _check_mass_ties(name):
    values, counts = np.unique(_deg(name), return_counts=True)
    assert len(values) <= 3 and counts.max() >= io.expected(name).n // 3


def _check_slots(k):
    def check(name):
        assert _slots(name) == k
    return check


def _check_identity_perm(name):
    ref = io.expected(name)
    assert np.array_equal(ref.perm, np.arange(ref.n)) and set(_deg(name).tolist()) == {8}


def _check_mass_isolated(name):
    assert (_deg(name) == 0).sum() > 250_000


def _check_rows_stride(name):
    assert io.expected(name).n > io.ORIENT_WAVE_ROWS


def _check_ballot_rows(name):
    assert {63, 64, 65, 127, 128, 129, 1000, 1001} <= set(_deg(name).tolist())


def _check_ballot_kept(name):
    assert {1, 63, 64, 65, 127, 128, 129} <= set(np.diff(io.expected_oriented(name).row_ptr).tolist())


def _check_hub_row(name):
    ref = io.expected(name)
    longest = max(int(_deg(name).max()), int(np.diff(ref.t_row_ptr).max()) if ref.directed else 0)
    assert longest >= io.HUB_BIG


def _check_hub_loop(name):
    ref = io.expected(name)
    assert _deg(name)[0] == io.HUB_BIG + 1 and ref.perm[0] == io.HUB_BIG_LABEL
    assert 0 in ref.col[ref.row_ptr[0]:ref.row_ptr[1]]                  # the loop arc of internal row 0
    assert 0 < _sentinel_share(name) < 1e-4


def _check_shuffled(name):
    assert 0.3 <= _reversed_share(name) <= 0.7


def _check_special_weights(name):
    _, _, _, w, _ = io.graph(name)
    ref = io.expected(name)
    given = set(io.bits(w).tolist()) & set(io.SPECIAL_WEIGHT_BITS.tolist())
    assert len(given) == min(len(io.SPECIAL_WEIGHT_BITS), len(w)) == len(set(io.SPECIAL_WEIGHT_BITS[:len(w)].tolist()))
    for out in (ref.w, ref.t_w) if ref.directed else (ref.w,):
        assert set(io.bits(out).tolist()) & set(io.SPECIAL_WEIGHT_BITS.tolist()) == given
        assert len(np.unique(io.bits(out))) == len(np.unique(io.bits(w)))
    if len(w) >= 100:
        with np.errstate(invalid='ignore'):
            assert not np.array_equal(io.bits(w + 0.0), io.bits(w))    # what a kernel that "adds zero" would store


def _check_finite_weights(name):
    _, _, _, w, _ = io.graph(name)
    assert np.all(np.isfinite(w)) and np.all(w * 8 == np.rint(w * 8)) and w.min() > 0 and w.sum() < 2.0 ** 40


def _check_in_hub_last(name):
    ref = io.expected(name)
    sink = io.DHUB_ORDINARY + 1
    assert ref.directed and ref.inv[sink] == ref.n - 1 == sink and _deg(name)[-1] == 0
    t_len = np.diff(ref.t_row_ptr)
    assert t_len[-1] == io.HUB_BIG == t_len.max()


def _check_out_hub_first(name):
    ref = io.expected(name)
    assert ref.inv[io.DHUB_ORDINARY] == 0 and _deg(name)[0] == io.HUB_BIG and np.diff(ref.t_row_ptr)[0] == 0


def _check_reciprocal(name):
    n, src, dst, w, _ = io.graph(name)
    fwd = dict(zip((src * n + dst).tolist(), io.bits(w).tolist()))
    pairs = [(k, (k % n) * n + k // n) for k in fwd if k // n < k % n and (k % n) * n + k // n in fwd]
    assert len(pairs) > 30000 and sum(fwd[a] != fwd[b] for a, b in pairs) > len(pairs) // 2


def _check_directed_loops(name):
    _, src, dst, _, directed = io.graph(name)
    assert directed and (src == dst).sum() > 500


def _check_saturation(name):
    lengths = set(np.diff(io.expected_oriented(name).row_ptr).tolist())
    assert {1021, 1022, 1023, 1024, 1025} <= lengths
    assert len(io.graph(name)[1]) >= 525825


def _check_scan_top_chunk(name):
    assert -(-io.expected(name).n // io.SCAN_TILE) > io.SCAN_TOP_THREADS


def _check_edge_stride(name):
    assert io.expected(name).m > io.EDGE_GRID_SPAN


def _check_arc_stride(name):
    assert io.expected(name).n > io.ARC_GRID_SPAN and not io.expected(name).directed


PROPERTY_CHECKS = {
    'single_node': _check_single_node, 'reversed_edge': _check_reversed_edge, 'all_loops': _check_all_loops,
    'loops_even_odd': _check_loops_even_odd, 'block_edge': _check_block_edge, 'scan_tile_edge': _check_scan_tile_edge,
    'sort_tile_edge': _check_sort_tile_edge, 'last_tile_single': _check_last_tile_single,
    'last_isolated': _check_last_isolated, 'mass_ties': _check_mass_ties, 'slots_4095': _check_slots(4095),
    'slots_4096': _check_slots(4096), 'slots_4097': _check_slots(4097), 'identity_perm': _check_identity_perm,
    'mass_isolated': _check_mass_isolated, 'rows_stride': _check_rows_stride, 'ballot_rows': _check_ballot_rows,
    'ballot_kept': _check_ballot_kept, 'hub_row': _check_hub_row, 'hub_loop': _check_hub_loop,
    'shuffled': _check_shuffled, 'special_weights': _check_special_weights, 'finite_weights': _check_finite_weights,
    'in_hub_last': _check_in_hub_last, 'out_hub_first': _check_out_hub_first, 'reciprocal': _check_reciprocal,
    'directed_loops': _check_directed_loops, 'saturation': _check_saturation, 'scan_top_chunk': _check_scan_top_chunk,
    'edge_stride': _check_edge_stride, 'arc_stride': _check_arc_stride,
}


@pytest.mark.parametrize('name', io.CASE_NAMES)
def test_case_reaches_what_it_is_listed_for(name):
    for prop in sorted(io.case(name).props):
        PROPERTY_CHECKS[prop](name)


def test_every_constant_has_a_case_on_both_sides():
    """Scan tile 2048 and the top chunk, sort tile 4096, the 32 768-row and 2 097 152-row strides, the 1 048 576-edge
    stride, the 64-lane ballot and the 1023 saturation: a case below (or on) and a case above each."""
    ns = {io.graph(c.name)[0] for c in io.CASES}
    ms = {len(io.graph(c.name)[1]) for c in io.CASES}
    assert {2047, 2048, 2049, 4095, 4096, 4097} <= ns
    assert {4095, 4096, 4097} <= {_slots(c.name) for c in io.CASES}
    undirected_n = {io.graph(name)[0] for name in UNDIRECTED}
    assert min(undirected_n) <= io.ORIENT_WAVE_ROWS < sorted(undirected_n)[-2] <= io.ARC_GRID_SPAN < max(undirected_n)
    assert min(ms) <= io.EDGE_GRID_SPAN < max(ms)
    assert min(-(-n // io.SCAN_TILE) for n in ns) == 1 and max(-(-n // io.SCAN_TILE) for n in ns) == 1025
    lengths = set(np.diff(io.expected_oriented('clique1026').row_ptr).tolist())
    assert io.SATURATION - 1 in lengths and io.SATURATION in lengths and io.SATURATION + 1 in lengths


def test_clique_triangles_follow_from_the_construction():
    """No edge joins two neighbours of a clique node other than the clique's own: C(1025, 2) triangles each."""
    n, src, dst, _, _ = io.graph('clique1026')
    lab = set(io.clique_labels().tolist())
    inside = np.array([int(a) in lab and int(b) in lab for a, b in zip(src.tolist(), dst.tolist())])
    assert inside.sum() == io.CLIQUE * (io.CLIQUE - 1) // 2
    touching = np.array([(int(a) in lab) != (int(b) in lab) for a, b in zip(src.tolist(), dst.tolist())])
    outer = np.where(np.isin(src[touching], io.clique_labels()), dst[touching], src[touching])
    deg = np.bincount(np.concatenate([src, dst]), minlength=n)
    assert len(outer) == len(set(outer.tolist())) > 100 and np.all(deg[outer] == 1)


# ---- workspace contract (no device: the size is checked before the stream or any pointer is used) -------------------

def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize('n, m, directed', [(1, 1, 0), (300, 2500, 0), (200, 900, 1), (2049, 4097, 1)])
def test_ingest_refuses_a_workspace_one_byte_short_before_any_launch(n, m, directed):
    from graphrole_amd import _lib
    lib = _lib.load()
    need = lib.grx_ingest_workspace_bytes(n, m, directed)
    nnz = m if directed else 2 * m
    assert need >= 8 * (2 * n + 3 * nnz)
    dummy = np.zeros(8, dtype=np.int64)                       # non-NULL host addresses: never read, never written
    args = [n, m, _p(dummy), _p(dummy), _p(dummy), directed, nnz] + [_p(dummy)] * 10
    rc = lib.grx_ingest(*args, need - 1, None)
    assert rc == -3 and b'workspace' in lib.grx_last_error()  # GRX_ERR_WORKSPACE
    assert not dummy.any()
    with pytest.raises(_lib.GrxError, match='status -3'):
        _lib.call('grx_ingest', *args, need - 1, None)
    assert lib.grx_ingest(*args[:16], None, need, None) == -1  # a NULL workspace of the right size: GRX_ERR_INVALID


@pytest.mark.parametrize('n', [1, 2048, 2049, 300000])
def test_orientation_refuses_a_workspace_one_byte_short_before_any_launch(n):
    from graphrole_amd import _lib
    lib = _lib.load()
    need = lib.grx_orient_workspace_bytes(n)
    assert need >= 4 * n + 8 * (n + 1)
    dummy = np.zeros(8, dtype=np.int64)
    assert lib.grx_orient_count(n, _p(dummy), _p(dummy), _p(dummy), _p(dummy), need - 1, None) == -3
    assert b'workspace' in lib.grx_last_error()
    assert lib.grx_orient_fill(n, _p(dummy), _p(dummy), _p(dummy), 0, None, None, _p(dummy), need - 1, None) == -3
    assert b'workspace' in lib.grx_last_error() and not dummy.any()
