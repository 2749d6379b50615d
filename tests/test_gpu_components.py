"""
-m gpu: grx_components (connected, weak, strong) and grx_reachable on the MI355X against tests/components_oracle.py --
labels, sizes, counts and the round counts of the method, exactly -- and the public functions of
graphrole_amd.components against networkx.  tests/test_components_cpu.py holds the oracle itself to networkx.
"""
import functools

import networkx as nx
import numpy as np
import pytest

from tests import components_oracle as co, tiled_graphs as tg

pytestmark = pytest.mark.gpu

MODES = (co.CONNECTED, co.WEAK, co.STRONG)
LANES = (4, 8, 16, 32)


@pytest.fixture(scope='module')
def K():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from graphrole_amd import kernels
    return kernels


def _device(K, row_ptr, col, mode, lanes=None, want_size=True, in_csr=None):
    """(label, size, n_components, rounds) of K.components as host arrays cut to n rows."""
    n = len(row_ptr) - 1
    out = K.DeviceCSR(row_ptr, col)
    tr = None
    if mode == co.STRONG:
        tr = K.DeviceCSR(*(co.transpose(row_ptr, col) if in_csr is None else in_csr))
    label, size, n_components, rounds = K.components(out, tr, mode=mode, want_size=want_size, lanes=lanes)
    label = K.to_host(label)[:n].copy()
    assert label.dtype == np.int32
    if want_size:
        size = K.to_host(size)[:n].copy()
        assert size.dtype == np.int64
    return label, size, n_components, rounds


def _same(got, want, what):
    label, size, n_components, rounds = got
    assert np.array_equal(label, want.label), (what, np.nonzero(label != want.label)[0][:8])
    assert np.array_equal(size, want.size), (what, np.nonzero(size != want.size)[0][:8])
    assert (n_components, rounds) == (want.n_components, want.rounds), what


def _reach(K, row_ptr, col, flag, lanes=None):
    n = len(row_ptr) - 1
    out, count, levels = K.reachable(K.DeviceCSR(row_ptr, col), flag, lanes=lanes)
    return K.to_host(out)[:n].copy(), count, levels


# ----------------------------------------------------------------------------------------------------- exhaustive
def test_every_digraph_on_four_nodes(K):
    n, row_ptr, col = co.all_digraphs4()
    assert n == 16384
    for mode in (co.STRONG, co.WEAK):
        _same(_device(K, row_ptr, col, mode), co.components(row_ptr, col, mode), mode)


def test_every_graph_on_five_nodes(K):
    n, row_ptr, col = co.all_graphs5()
    assert n == 5120
    _same(_device(K, row_ptr, col, co.CONNECTED), co.components(row_ptr, col, co.CONNECTED), 'connected')


# ------------------------------------------------------------------------------------------------ seeded families
def test_seeded_families(K):
    count = 0
    for seed in range(13):
        for G in co.directed_family(seed):
            _, row_ptr, col, _, _ = co.graph_csrs(G)
            for mode in (co.STRONG, co.WEAK):
                _same(_device(K, row_ptr, col, mode), co.components(row_ptr, col, mode), (seed, mode))
            count += 1
        for G in co.undirected_family(seed):
            _, row_ptr, col, _, _ = co.graph_csrs(G)
            _same(_device(K, row_ptr, col, co.CONNECTED), co.components(row_ptr, col, co.CONNECTED), (seed, 'connected'))
            count += 1
    assert count > 100


# ------------------------------------------------------------------------------------------------------- hub rows
@pytest.mark.parametrize('kind', co.HUB_CASES)
def test_hub_rows(K, kind):
    row_ptr, col = co.hub_case(kind)
    tr = co.transpose(row_ptr, col)
    longest = max(np.diff(row_ptr).max(), np.diff(tr[0]).max())
    assert K.HUB_FACTOR * 4 < longest <= K.HUB_FACTOR * 32       # a hub row with 4 lanes, a lane-group row with 32
    for mode in MODES:
        rp, c = (row_ptr, col) if mode != co.CONNECTED else _symmetric(row_ptr, col)
        want = co.components(rp, c, mode)
        for lanes in (4, 32):
            _same(_device(K, rp, c, mode, lanes=lanes), want, (kind, mode, lanes))
    flag = np.zeros(len(row_ptr) - 1, dtype=np.int32)
    flag[0] = 1                                                 # the seed is the hub
    for a in ((row_ptr, col), tr):
        want = co.reachable(*a, flag)
        for lanes in (4, 32):
            got = _reach(K, *a, flag, lanes=lanes)
            assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (kind, lanes)


def _symmetric(row_ptr, col):
    src, dst = co.arcs_of(row_ptr, col)
    return co.symmetric_csr(len(row_ptr) - 1, np.stack([src, dst], axis=1))


# ------------------------------------------------------------------------- loops that straddle the read-back batch
def test_round_loops_across_the_read_back_batch(K):
    k = 3 * K.CP_ROUND_BATCH + 5
    assert K.CP_ROUND_BATCH == co.ROUND_BATCH
    for name, (row_ptr, col) in (('cycle', co.cycle(k)), ('path', co.path(k))):
        want = co.components(row_ptr, col, co.STRONG)
        assert want.rounds > K.CP_ROUND_BATCH, name              # more than one read-back
        _same(_device(K, row_ptr, col, co.STRONG), want, name)
    assert co.components(*co.cycle(k), co.STRONG).rounds == 2 * k + 2
    up, down = co.two_cycle_chain(32), co.two_cycle_chain(32, ascending=False)
    want_up, want_down = co.components(*up, co.STRONG), co.components(*down, co.STRONG)
    assert want_up.outer == 32 and want_up.rounds >= 2 * K.CP_ROUND_BATCH and want_down.outer == 1
    _same(_device(K, *up, co.STRONG), want_up, 'ascending chain')
    _same(_device(K, *down, co.STRONG), want_down, 'descending chain')


# -------------------------------------------------------------------------------------------------- grx_reachable
def test_reachable(K):
    G = next(g for seed in range(3, 9) for g in co.directed_family(seed) if g.number_of_nodes() > 20)
    _, row_ptr, col, in_row_ptr, in_col = co.graph_csrs(G)
    n = len(row_ptr) - 1
    none, every = np.zeros(n, dtype=np.int32), np.full(n, -3, dtype=np.int32)
    some = np.zeros(n, dtype=np.int32)
    some[[2, n - 1]] = (5, 1)
    for a in ((row_ptr, col), (in_row_ptr, in_col)):
        for flag in (none, every, some):
            want = co.reachable(*a, flag)
            got = _reach(K, *a, flag)
            assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    assert _reach(K, row_ptr, col, none)[1:] == (0, 0) and _reach(K, row_ptr, col, every)[1:] == (n, 0)
    # a path deeper than one batch, from its first row and, over the transpose, from its last
    k = 3 * K.CP_ROUND_BATCH + 5
    p = co.path(k)
    first, last = np.zeros(k, dtype=np.int32), np.zeros(k, dtype=np.int32)
    first[0], last[-1] = 1, 1
    assert _reach(K, *p, first)[1:] == (k, k - 1) and _reach(K, *p, last)[1:] == (1, 0)
    got = _reach(K, *co.transpose(*p), last)
    assert got[0].all() and got[1:] == (k, k - 1)
    # seeds in two components at once: a cycle and a path side by side, interleaved
    n2, rp2, c2 = co.interleave([co.cycle(9), co.path(9)])
    flag = np.zeros(n2, dtype=np.int32)
    flag[[2 * 4, 2 * 6 + 1]] = 1                                # row 4 of the cycle, row 6 of the path
    want = co.reachable(rp2, c2, flag)
    got = _reach(K, rp2, c2, flag)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:] == (9 + 3, 8)
    # a device tensor is updated in place
    t = K.to_device(flag.copy())
    out, count, _ = K.reachable(K.DeviceCSR(rp2, c2), t)
    assert out is t and np.array_equal(K.to_host(t)[:n2], want[0]) and count == 12


# ------------------------------------------------------------------------------------------------------- sameness
def test_same_bytes_every_run_and_every_lane_width(K):
    row_ptr, col = co.motif()
    sym = _symmetric(row_ptr, col)
    for mode in MODES:
        a = sym if mode == co.CONNECTED else (row_ptr, col)
        first = _device(K, *a, mode)
        for lanes in (None,) + LANES:
            got = _device(K, *a, mode, lanes=lanes)
            assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes(), (mode, lanes)
            assert got[2:] == first[2:], (mode, lanes)
        alone = _device(K, *a, mode, want_size=False)
        assert alone[1] is None and alone[0].tobytes() == first[0].tobytes() and alone[2:] == first[2:]
    flag = np.zeros(len(row_ptr) - 1, dtype=np.int32)
    flag[[0, 7]] = 1
    first = _reach(K, row_ptr, col, flag)
    for lanes in (None,) + LANES:
        got = _reach(K, row_ptr, col, flag, lanes=lanes)
        assert got[0].tobytes() == first[0].tobytes() and got[1:] == first[1:]


def test_a_permutation_of_the_rows_gives_the_same_partition(K):
    from graphrole_amd import components as pub
    G = nx.gnm_random_graph(300, 420, seed=11, directed=True)
    _, row_ptr, col, _, _ = co.graph_csrs(G)
    n = len(row_ptr) - 1
    perm = np.random.default_rng(3).permutation(n)              # old row v becomes row perm[v]
    src, dst = co.arcs_of(row_ptr, col)
    moved = co.directed_csr(n, np.stack([perm[src], perm[dst]], axis=1))
    for mode in MODES:
        a, b = ((row_ptr, col), moved) if mode != co.CONNECTED else (_symmetric(row_ptr, col), _symmetric(*moved))
        label, size, count, _ = _device(K, *a, mode)
        label2, size2, count2, _ = _device(K, *b, mode)
        assert count == count2 and np.array_equal(size, size2[perm]), mode
        assert co.partition(label) == co.partition(label2[perm]), mode
        # the component / component_size columns: names of the classes by first member in the (old) index
        assert np.array_equal(pub._ranked(label.astype(np.int64), size)[0],
                              pub._ranked(label2[perm].astype(np.int64), size2[perm])[0]), mode


# ----------------------------------------------------------------------------------------------------- edge cases
def test_edge_cases(K):
    empty = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64))
    one = (np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int64))
    no_arcs = (np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int64))
    loops = (np.arange(6, dtype=np.int64), np.arange(5, dtype=np.int64))
    one_loop = (np.arange(2, dtype=np.int64), np.zeros(1, dtype=np.int64))
    for mode in MODES:
        label, size, count, rounds = _device(K, *empty, mode)
        assert len(label) == 0 and len(size) == 0 and (count, rounds) == (0, 0)
        for a in (one, no_arcs, loops, one_loop):
            want = co.components(*a, mode)
            assert want.n_components == len(a[0]) - 1 and want.rounds == (mode == co.STRONG)
            _same(_device(K, *a, mode), want, mode)
    assert _reach(K, *empty, np.zeros(0, dtype=np.int32))[1:] == (0, 0)
    got = _reach(K, *loops, np.array([0, 1, 0, 0, 0], dtype=np.int32))
    assert got[0].tolist() == [0, 1, 0, 0, 0] and got[1:] == (1, 0)
    with pytest.raises(ValueError, match='in-adjacency'):
        K.components(K.DeviceCSR(*one), None, mode='strong')
    with pytest.raises(ValueError, match='mode'):
        K.components(K.DeviceCSR(*one), None, mode='giant')


# ------------------------------------------------------------------------- public functions against networkx
def _public_graphs():
    yield 'gnm', nx.gnm_random_graph(200, 260, seed=1, directed=True)
    yield 'dense', nx.gnm_random_graph(60, 400, seed=2, directed=True)
    M = nx.MultiDiGraph(nx.gnm_random_graph(80, 110, seed=3, directed=True))
    M.add_edges_from([(0, 1), (0, 1), (1, 0), (5, 5)])
    yield 'multidigraph', M
    yield 'strings', nx.relabel_nodes(nx.gnm_random_graph(90, 130, seed=4, directed=True), lambda v: f'v{v:03d}')
    T = nx.DiGraph()                                            # the giant component ties in size with another
    nx.add_cycle(T, [10, 11, 12, 13])
    nx.add_cycle(T, [0, 1, 2, 3])
    T.add_edges_from([(13, 20), (20, 0), (21, 10), (3, 22), (21, 23), (24, 22), (30, 31)])
    yield 'tie', T
    yield 'no_arcs', nx.empty_graph(5, create_using=nx.DiGraph)
    yield 'scale_free', nx.DiGraph(nx.scale_free_graph(300, seed=5))
    yield 'undirected', nx.disjoint_union(nx.barabasi_albert_graph(150, 2, seed=6), nx.gnm_random_graph(80, 50, seed=7))
    U = nx.MultiGraph(nx.gnm_random_graph(70, 60, seed=8))
    U.add_edges_from([(0, 1), (0, 1), (4, 4)])
    yield 'multigraph', U
    yield 'undirected_strings', nx.relabel_nodes(nx.gnm_random_graph(60, 45, seed=9), lambda v: f'u{v:02d}')
    yield 'path', nx.path_graph(40)
    yield 'n1', nx.empty_graph(1)


def _ordered(sets):
    return sorted((set(s) for s in sets), key=min)


@pytest.mark.parametrize('key', [k for k, _ in _public_graphs()])
def test_public_functions_against_networkx(K, key):
    import graphrole_amd as ga
    from tests.test_components_cpu import _bow_tie_by_definition, _check_table
    G = dict(_public_graphs())[key]
    probes = sorted(G)[::max(len(G) // 3, 1)][:3]
    if not G.is_directed():
        want = _ordered(nx.connected_components(G))
        assert ga.connected_components(G) == want
        assert ga.number_connected_components(G) == len(want) and ga.is_connected(G) == nx.is_connected(G)
        ranked = _check_table(ga.component_table(G), want, G)
        assert list(ga.largest_component(G)) == sorted(ranked[0])
        for v in probes:
            assert ga.descendants(G, v) == nx.descendants(G, v) == ga.ancestors(G, v)
        return
    weak, strong = _ordered(nx.weakly_connected_components(G)), _ordered(nx.strongly_connected_components(G))
    assert ga.weakly_connected_components(G) == weak and ga.strongly_connected_components(G) == strong
    assert ga.number_weakly_connected_components(G) == len(weak)
    assert ga.number_strongly_connected_components(G) == len(strong)
    assert ga.is_weakly_connected(G) == nx.is_weakly_connected(G)
    assert ga.is_strongly_connected(G) == nx.is_strongly_connected(G)
    _check_table(ga.component_table(G), weak, G)
    table = ga.component_table(G, kind='strong')
    ranked = _check_table(table, strong, G)
    assert table.attrs['rounds'] >= 1
    assert list(ga.largest_component(G, kind='strong')) == sorted(ranked[0])
    for v in probes:
        assert ga.descendants(G, v) == nx.descendants(G, v) and ga.ancestors(G, v) == nx.ancestors(G, v)
    tie = ga.bow_tie(G)
    want = _bow_tie_by_definition(G, sorted(G))
    assert np.array_equal(tie.cat.codes.to_numpy(), want) and list(tie.index) == sorted(G)
    assert tie.attrs['sizes'] == {c: int((want == k).sum()) for k, c in enumerate(tie.cat.categories)}
    if key == 'tie':
        assert set(tie.index[tie == 'core']) == {0, 1, 2, 3} and tie[10] == 'in' and tie[22] == 'out'
        assert tie[21] == 'in' and tie[23] == 'tendril' and tie[24] == 'tendril' and tie[30] == 'other'


# ------------------------------------------------------------ the second trip of every capped grid-stride launch
ROWS = 2048 * 256                                               # as tests/test_gpu_second_trip.py


def _wraps(items, per_block, cap):
    return items > cap * per_block


@functools.lru_cache(maxsize=None)
def _tiled():
    row_ptr, col = co.motif()
    t_ptr, t_col = co.transpose(row_ptr, col)
    n0 = len(row_ptr) - 1
    C = tg.copies_for(n0, ROWS + ROWS // 4)
    n, big_ptr, big_col, _, _ = tg.tile(row_ptr, col, C)
    _, big_t_ptr, big_t_col, _, _ = tg.tile(t_ptr, t_col, C)
    assert ROWS + ROWS // 4 < n <= ROWS + ROWS // 4 + n0 and n < 1 << 21
    return (row_ptr, col), (t_ptr, t_col), C, n, (big_ptr, big_col), (big_t_ptr, big_t_col)


def test_second_trip_of_the_grid_stride_loops(K):
    small, small_t, C, n, big, big_t = _tiled()
    n0 = len(small[0]) - 1
    assert _wraps(n, K.CP_BLOCK, K.CP_MAX_BLOCKS)                               # every per-node launch
    assert _wraps(n, K.CP_BLOCK // K.CP_GROUP, K.CP_MAX_ROW_BLOCKS)             # st_rows, rc_rows
    assert np.diff(small[0]).max() > K.HUB_FACTOR * 4                           # hub rows, C of them
    sym0, sym = _symmetric(*small), _symmetric(*big)
    for mode in MODES:
        a0, a = (sym0, sym) if mode == co.CONNECTED else (small, big)
        in0, inn = (small_t, big_t) if mode == co.STRONG else (None, None)
        want = co.components(*a0, mode)
        label, size, count, rounds = _device(K, *a, mode, in_csr=inn)
        assert np.array_equal(label, tg.tile_ids(want.label, C)), mode
        assert np.array_equal(size, tg.tile_nodes(want.size, C)), mode
        assert (count, rounds) == (C * want.n_components, want.rounds), mode
        label0, size0, count0, rounds0 = _device(K, *a0, mode, in_csr=in0)      # the one-trip run on the motif, tiled
        assert label.tobytes() == tg.tile_ids(label0, C).tobytes() and size.tobytes() == tg.tile_nodes(size0, C).tobytes()
        assert (count, rounds) == (C * count0, rounds0), mode
    assert co.components(*small, co.STRONG).outer == 2
    flag0 = np.zeros(n0, dtype=np.int32)
    flag0[[1, n0 - 5]] = 1
    for a0, a in ((small, big), (small_t, big_t)):
        want = co.reachable(*a0, flag0)
        got = _reach(K, *a, tg.tile_nodes(flag0, C))
        assert np.array_equal(got[0], tg.tile_nodes(want[0], C)) and got[1:] == (C * want[1], want[2])
        alone = _reach(K, *a0, flag0)
        assert got[0].tobytes() == tg.tile_nodes(alone[0], C).tobytes() and got[1:] == (C * alone[1], alone[2])
