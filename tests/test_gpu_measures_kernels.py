"""
Kernel-level parity of csrc/grx_measures.hip on the MI355X: grx_pagerank and grx_eigenvector_centrality against the
long-double oracle of tests/measures_oracle.py (values to 1e-12 relative, atol 0; iteration counts exactly) over
every lane width, hub rows on and past each boundary, the grid caps and the iteration accounting of the batched
launches; grx_local_structure_measures bit-equal to the oracle's float64 restatement; the column chunks of
kernels.sense_normal_equations against long-double products.  tests/test_measures_oracle_cpu.py shows for every case
of measures_oracle.CASES that the stopping iteration cannot flip under fp64 rounding and that plain fp64 stays below
1e-13 of the oracle, so a miss here is the kernel's.
"""
import numpy as np
import pandas as pd
import pytest

from tests import measures_oracle as mo

pytestmark = pytest.mark.gpu

CASES = {c.id: c for c in mo.CASES}


@pytest.fixture(scope='module')
def K():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from graphrole_amd import kernels
    return kernels


_DEVICE = {}


def _device_csr(K, name):
    """(DeviceCSR of the in-adjacency, out-weight on the device) of a graph of measures_oracle.GRAPHS."""
    if name not in _DEVICE:
        g = mo.graph(name)
        _DEVICE[name] = (K.DeviceCSR(g.row_ptr, g.col, g.w), K.to_device(mo.out_weight(g)))
    return _DEVICE[name]


def _run(K, case, tol, max_iter):
    csr, S = _device_csr(K, case.graph)
    if case.measure == 'pagerank':
        x, it = K.pagerank(csr, S, case.alpha, tol, max_iter, lanes=case.lanes)
    else:
        x, it = K.eigenvector_centrality(csr, tol, max_iter, lanes=case.lanes)
    return K.to_host(x)[:csr.n], it


def _check(got, it, case):
    want, want_it, _ = mo.expected(case)
    dev = mo.max_rel_dev(got, want)
    print(f'{case.id}: iterations {it} (oracle {want_it}), max relative deviation {dev:.3e}')
    assert it == want_it, (case.id, it, want_it)
    assert got.dtype == np.float64
    np.testing.assert_allclose(got.astype(mo.LD), want, rtol=mo.RTOL, atol=0, err_msg=case.id)


@pytest.mark.parametrize('cid', [c.id for c in mo.CASES if c.stop_at is None])
def test_power_iteration_matches_long_double_oracle(K, cid):
    case = CASES[cid]
    g, csr = mo.graph(case.graph), _device_csr(K, case.graph)[0]
    if case.lanes is None:
        assert csr.lanes_per_row == mo.natural_lanes(g)
    got, it = _run(K, case, mo.case_tol(case), mo.MAX_ITER)
    _check(got, it, case)
    if case.graph == 'all_dangling':
        np.testing.assert_allclose(got, 1.0 / g.n, rtol=1e-15, atol=0)


def test_case_list_reaches_what_it_claims(K):
    """The shapes the case list is there for: every lane tier naturally, hub rows on and past each boundary, a
    directed in-adjacency with its own hub list, dangling and isolated rows next to hubs, both grid caps."""
    tiers = {mo.natural_lanes(mo.graph(g)) for g in ('tier4', 'tier8', 'tier16', 'tier32')}
    assert tiers == {4, 8, 16, 32}
    for name in ('tier4', 'tier8', 'tier16', 'tier32'):
        assert _device_csr(K, name)[0].n_hubs == 0
    for name in ('hubs', 'hubs_w', 'hubs_dir', 'hubs_dir_w', 'hubs_iso'):
        deg = np.diff(mo.graph(name).row_ptr)
        assert tuple(deg[:10]) == mo.BOUNDARY_HUBS + (300, 20000)
    for L in (4, 8, 16, 32):
        deg = np.diff(mo.graph('hubs').row_ptr)
        assert (deg == 32 * L).any() and (deg == 32 * L + 1).any()
    d = mo.graph('hubs_dir_w')
    out_deg = np.diff(mo.transpose(d).row_ptr)
    assert out_deg[10] >= 300 and out_deg[11] >= 20000 and np.diff(d.row_ptr)[10:12].max() < 128
    S = mo.out_weight(d)
    assert (S == 0).sum() == 10 + 40 + 5 and ((S == 0) & (np.diff(d.row_ptr) > 0)).sum() >= 30
    a = mo.graph('all_hubs')
    assert np.diff(a.row_ptr).min() > 128
    assert mo.graph('rows32').n > 2048 * 8 and mo.graph('rows4').n > 2048 * 64 and mo.graph('elements').n > 2048 * 256
    assert mo.natural_lanes(mo.graph('rows4')) == 4


@pytest.mark.parametrize('measure', ['pagerank', 'eigenvector'])
@pytest.mark.parametrize('k', [1, 7, 8, 9, 16, 17])
def test_iteration_accounting_on_and_past_a_batch(K, measure, k):
    """The oracle stops at k: max_iter = k succeeds with that count and the vector of iteration k (x[k & 1] on the
    device), max_iter = k - 1 raises with iterations == k - 1."""
    from graphrole_amd import ConvergenceError
    case = CASES[f'iters-{k}-{measure}']
    tol = mo.case_tol(case)
    assert mo.expected(case)[1] == k
    for max_iter in (k, mo.MAX_ITER):
        got, it = _run(K, case, tol, max_iter)
        _check(got, it, case)
    with pytest.raises(ConvergenceError) as info:
        _run(K, case, tol, k - 1)
    assert info.value.iterations == k - 1


@pytest.mark.parametrize('measure', ['pagerank', 'eigenvector'])
def test_max_iter_zero_raises_with_zero_iterations(K, measure):
    from graphrole_amd import ConvergenceError
    with pytest.raises(ConvergenceError) as info:
        _run(K, CASES[f'tier-tier4-{measure}'], 1e-6, 0)
    assert info.value.iterations == 0


@pytest.mark.parametrize('measure', ['pagerank', 'eigenvector'])
@pytest.mark.parametrize('graph', ['hubs_w', 'hubs_dir'])
def test_every_lane_width_repeats_bitwise(K, graph, measure):
    """Two runs of the same call give the same bytes for each L (no floating-point atomics); different L may differ
    in bits and all stay within the tolerance of the oracle."""
    for L in (4, 8, 16, 32):
        case = CASES[f'hubs-{graph}-L{L}-{measure}']
        a, it_a = _run(K, case, case.tol, mo.MAX_ITER)
        b, it_b = _run(K, case, case.tol, mo.MAX_ITER)
        assert a.tobytes() == b.tobytes() and it_a == it_b, L
        _check(a, it_a, case)


def test_forced_lanes_rebuild_the_hub_list(K):
    """lanes= narrower than the graph's own width makes more rows hubs: with the hub list of the natural width the
    kernel would read accumulators nobody wrote (the forced-* cases above).  Here: the graphs are what those cases
    need, and a width the library does not have is refused."""
    deg = np.diff(mo.graph('tier32').row_ptr)
    assert _device_csr(K, 'tier32')[0].n_hubs == 0 and (deg > 128).sum() == 0 and (deg > 64).sum() > 0
    assert _device_csr(K, 'all_hubs_w')[0].lanes_per_row == 32 and _device_csr(K, 'all_hubs_w')[0].n_hubs == 0
    with pytest.raises(ValueError, match='lanes_per_row'):
        _run(K, mo.Case('bad', 'tier4', 'pagerank', lanes=5), 1e-6, 10)


# ---- grx_local_structure_measures ------------------------------------------------------------------------------

def _synthetic_T(g, seed):
    """Triangle counts the kernel could meet: uniform in 0 .. d'(d' - 1) / 2, a fifth of them 0, 0 where d' < 2."""
    rng = np.random.default_rng(seed)
    own, _ = mo.loop_counts(g.row_ptr, g.col)
    dp = np.diff(g.row_ptr) - own
    top = np.maximum(dp * (dp - 1) // 2, 0)
    T = rng.integers(0, top + 1)
    T[rng.random(g.n) < 0.2] = 0
    return T.astype(np.uint64)


def _assert_bit_equal(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64)), \
        (what, np.flatnonzero(got[ok] != want[ok])[:5])


@pytest.mark.parametrize('loops', [False, True])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 255, 256, 257, 100003])
def test_local_structure_bit_equal_to_oracle(K, n, loops):
    g = mo.local_graph(70 + n % 50, n, loops)
    deg = np.diff(g.row_ptr)
    own, nl = mo.loop_counts(g.row_ptr, g.col)
    assert bool(own.any()) == loops
    if n >= 4:
        assert (deg == 0).any() and ((deg == 1) & (own == 0)).any()        # isolated; degree 1 with T = 0
    if loops:
        assert ((deg == 1) & (own == 1)).any()                 # only neighbour is itself
    if n > 6000:
        assert deg[0] == 5000 + int(loops)
        if loops:
            assert own[0] == 1 and 0.4 < nl[0] / 5000 < 0.6
    T = _synthetic_T(g, n)
    cl, es = K.local_structure(K.DeviceCSR(g.row_ptr, g.col), K.to_device(T.view(np.int64)), loops)
    want_cl, want_es = mo.local_measures(deg, own, T, nl)
    assert np.isfinite(want_cl).all() and np.isnan(want_es).sum() == ((deg == 0) | (deg == own)).sum()
    _assert_bit_equal(K.to_host(cl)[:n], want_cl, 'clustering')
    _assert_bit_equal(K.to_host(es)[:n], want_es, 'effective_size')


def test_triangle_counts_chain_into_local_structure_with_loops(K):
    """K.triangle_counts -> K.local_structure on the 100 003-node graph with loops; the oracle's counts come from a
    scipy sparse product on the loop-free part."""
    import scipy.sparse as sp
    n = 100003
    g = mo.local_graph(91, n, True)
    deg = np.diff(g.row_ptr)
    own, nl = mo.loop_counts(g.row_ptr, g.col)
    rows = np.repeat(np.arange(n, dtype=np.int64), deg)
    col = g.col.astype(np.int64)
    keep = rows != col
    A = sp.csr_array((np.ones(int(keep.sum()), dtype=np.int64), (rows[keep], col[keep])), shape=(n, n))
    twice = np.asarray((A @ A).multiply(A).sum(axis=1)).ravel()
    assert np.all(twice % 2 == 0) and twice.sum() > 0
    T = twice // 2
    csr = K.DeviceCSR(g.row_ptr, g.col)
    T_dev = K.triangle_counts(csr)
    assert np.array_equal(K.to_host(T_dev)[:n], T)
    cl, es = K.local_structure(csr, T_dev, True)
    want_cl, want_es = mo.local_measures(deg, own, T, nl)
    _assert_bit_equal(K.to_host(cl)[:n], want_cl, 'clustering')
    _assert_bit_equal(K.to_host(es)[:n], want_es, 'effective_size')


# ---- kernels.sense_normal_equations ----------------------------------------------------------------------------

_TABLES = {}


def _tables(n):
    """G (n x 16, non-negative like a role factor), M (n x 300, mixed sign, columns of different scales) and their
    long-double products; narrower shapes are slices of them."""
    if n not in _TABLES:
        rng = np.random.default_rng(n)
        G = rng.random((n, 16))
        M = rng.standard_normal((n, 300)) * np.exp(rng.uniform(-3, 3, size=300))
        Gl, Ml = G.astype(mo.LD), M.astype(mo.LD)
        _TABLES[n] = (G, M, Gl.T @ Gl, Gl.T @ Ml, (Ml * Ml).sum(axis=0))
    return _TABLES[n]


@pytest.mark.parametrize('n', [1, 1000, 100003])
@pytest.mark.parametrize('r', [2, 6, 16])
def test_sense_normal_equations_chunks(K, r, n):
    G16, M300, GtG_ld, GtM_ld, mm_ld = _tables(n)
    G = np.ascontiguousarray(G16[:, :r])
    gn = np.sqrt(np.diag(GtG_ld)[:r].astype(np.float64))
    mn = np.sqrt(mm_ld.astype(np.float64))
    for m in (1, 128 - r, 128 - r + 1, 300):
        M = np.ascontiguousarray(M300[:, :m])
        GtG, GtM, mm = K.sense_normal_equations(G, M)
        assert GtG.shape == (r, r) and GtM.shape == (r, m) and mm.shape == (m,)
        for got, want, scale, what in ((GtG, GtG_ld[:r, :r], np.outer(gn, gn), 'GtG'),
                                       (GtM, GtM_ld[:r, :m], np.outer(gn, mn[:m]), 'GtM'),
                                       (mm, mm_ld[:m], mn[:m] ** 2, 'mm')):
            bound = 1e-12 * scale + 1e-12 * np.abs(want.astype(np.float64))
            miss = np.abs(got.astype(mo.LD) - want).astype(np.float64) > bound
            assert not miss.any(), (what, r, m, n, np.argwhere(miss)[:5])


def test_sense_making_on_a_300_column_table_equals_its_chunks():
    from graphrole_amd import RoleExtractor
    rng = np.random.default_rng(5)
    n, r, m = 1000, 6, 300
    index = [f'v{i:04d}' for i in range(n)]
    ext = RoleExtractor(n_roles=r)
    ext.node_role_factor = pd.DataFrame(rng.random((n, r)), index=index, columns=[f'role_{i}' for i in range(r)])
    M = pd.DataFrame(rng.standard_normal((n, m)) * np.exp(rng.uniform(-3, 3, size=m)), index=index,
                     columns=[f'm{j:03d}' for j in range(m)])
    E = ext.sense_making(M).copy()
    assert E.shape == (r, m) and np.all(E.to_numpy() >= 0)
    width = 128 - r                                            # the columns one Gram pass holds next to G
    for c0 in range(0, m, width):
        part = ext.sense_making(M.iloc[:, c0:c0 + width])
        assert list(part.columns) == list(M.columns[c0:c0 + width])
        assert np.array_equal(part.to_numpy(), E.iloc[:, c0:c0 + width].to_numpy()), c0
    # the KKT conditions of test_gpu_sense.py::test_karate_end_to_end_sense_making
    Gf, Mv = ext.node_role_factor.to_numpy(), M.to_numpy()
    for j, name in enumerate(M.columns):
        e, mj = E[name].to_numpy(), Mv[:, j]
        g = Gf.T @ (Gf @ e - mj)
        eps = 1e-8 * np.sqrt(np.max(np.sum(Gf * Gf, axis=0)) * (mj @ mj))
        assert np.all(g[e == 0] >= -eps) and np.all(np.abs(g[e > 0]) <= eps), name
