"""
-m "not gpu": the Python layer of RolX sense making (graphrole_amd.node_measures, RoleExtractor.sense_making) over
a CPU double defined here -- tests/fake_kernels plus numpy versions of the measure kernels; the NNLS is the real
host code of libgrx.so (grx_host_nnls needs no device).  Argument errors, label alignment, the catalogue per graph
kind and the scope limits; the numbers themselves are pinned on the GPU (tests/test_gpu_sense.py).
"""
import types

import networkx as nx
import numpy as np
import pandas as pd
import pytest
import torch

from tests import fake_kernels


def _csr_arrays(csr):
    return np.asarray(csr.row_ptr, dtype=np.int64), np.asarray(csr.col, dtype=np.int64)


def _row_counts(csr, add_self_loop):
    row_ptr, col = _csr_arrays(csr)
    deg = np.diff(row_ptr).astype(np.float64)
    if add_self_loop:
        rows = np.repeat(np.arange(csr.n), np.diff(row_ptr))
        deg += np.bincount(rows[rows == col], minlength=csr.n)
    return torch.from_numpy(deg)


def _triangle_counts(csr):
    row_ptr, col = _csr_arrays(csr)
    nbrs = [set(col[row_ptr[v]:row_ptr[v + 1]]) - {v} for v in range(csr.n)]
    return torch.tensor([sum(len(nbrs[v] & nbrs[u]) for u in nbrs[v]) // 2 for v in range(csr.n)],
                        dtype=torch.int64)


def _local_structure(csr, T, has_loops):
    row_ptr, col = _csr_arrays(csr)
    n = csr.n
    loop = np.array([v in set(col[row_ptr[v]:row_ptr[v + 1]]) for v in range(n)], dtype=np.int64)
    cl, es = np.zeros(n), np.zeros(n)
    for v in range(n):
        d = row_ptr[v + 1] - row_ptr[v]
        dp = d - loop[v]
        t = int(T[v])
        cl[v] = 0.0 if t == 0 else 2 * t / (dp * (dp - 1))
        nl = sum(loop[u] for u in col[row_ptr[v]:row_ptr[v + 1]] if u != v)
        es[v] = np.nan if d == 0 or dp == 0 else dp - 2 * (t + nl) / dp
    return torch.from_numpy(cl), torch.from_numpy(es)


def _in_matrix(csr):
    row_ptr, col = _csr_arrays(csr)
    w = np.ones(len(col)) if csr.w is None else np.asarray(csr.w)
    rows = np.repeat(np.arange(csr.n), np.diff(row_ptr))
    A = np.zeros((csr.n, csr.n))
    np.add.at(A, (rows, col), w)
    return A                                                  # A[v, u] = weight of u -> v (pulled rows)


def _pagerank(csr_in, out_weight, alpha, tol, max_iter, lanes=None):
    from graphrole_amd import ConvergenceError
    A = _in_matrix(csr_in)
    S = out_weight.numpy()
    n = csr_in.n
    sinv = np.where(S != 0, 1.0 / np.where(S != 0, S, 1.0), 0.0)
    x = np.full(n, 1.0 / n)
    for it in range(1, max_iter + 1):
        xn = alpha * (A @ (x * sinv) + x[S == 0].sum() / n) + (1 - alpha) / n
        err, x = np.abs(xn - x).sum(), xn
        if err < n * tol:
            return torch.from_numpy(x), it
    raise ConvergenceError('not converged', iterations=max_iter)


def _eigenvector(csr_in, tol, max_iter, lanes=None):
    from graphrole_amd import ConvergenceError
    A = _in_matrix(csr_in)
    n = csr_in.n
    x = np.full(n, 1.0 / n)
    for it in range(1, max_iter + 1):
        z = x + A @ x
        xn = z / (np.linalg.norm(z) or 1.0)
        err, x = np.abs(xn - x).sum(), xn
        if err < n * tol:
            return torch.from_numpy(x), it
    raise ConvergenceError('not converged', iterations=max_iter)


def _sense_normal_equations(G, M):
    return G.T @ G, G.T @ M, np.einsum('ij,ij->j', M, M)


def _nnls(GtG, GtM, mm=None):
    from graphrole_amd import kernels  # noqa: F401 -- host-only entry point of libgrx.so
    from graphrole_amd.kernels import nnls
    return nnls(GtG, GtM, mm)


@pytest.fixture
def cpu_backend():
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.row_counts = _row_counts
    double.triangle_counts = _triangle_counts
    double.local_structure = _local_structure
    double.pagerank = _pagerank
    double.eigenvector_centrality = _eigenvector
    double.sense_normal_equations = _sense_normal_equations
    double.nnls = _nnls
    backend.use(double)
    yield double
    backend.use(None)


def test_catalogue_per_graph_kind(cpu_backend):
    from graphrole_amd import node_measures
    M = node_measures(nx.karate_club_graph())
    assert list(M.columns) == ['degree', 'weighted_degree', 'clustering', 'effective_size', 'pagerank', 'eigenvector']
    assert list(M.index) == list(range(34))
    D = nx.gnm_random_graph(40, 120, seed=1, directed=True)
    assert list(node_measures(D).columns) == ['degree', 'weighted_degree', 'in_degree', 'out_degree', 'pagerank',
                                              'eigenvector']
    MG = nx.MultiGraph([(0, 1), (0, 1), (1, 2)])
    assert list(node_measures(MG).columns) == ['degree', 'weighted_degree', 'pagerank']
    assert node_measures(MG)['degree'].tolist() == [2, 3, 1]


def test_values_and_order_through_the_double(cpu_backend):
    from graphrole_amd import node_measures
    G = nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'n{v:02d}')
    M = node_measures(G, ['pagerank', 'clustering', 'degree'])
    assert list(M.columns) == ['pagerank', 'clustering', 'degree']
    assert list(M.index) == sorted(G.nodes)
    cl = nx.clustering(G)
    assert np.array_equal(M['clustering'].to_numpy(), np.array([cl[k] for k in M.index]))
    assert M['degree'].dtype == np.int64
    pr = nx.pagerank(G)
    np.testing.assert_allclose(M['pagerank'].to_numpy(), [pr[k] for k in M.index], rtol=1e-10)
    assert M.attrs['iterations']['pagerank'] > 0


def test_argument_errors_and_scope(cpu_backend):
    from graphrole_amd import ConvergenceError, node_measures
    G = nx.karate_club_graph()
    with pytest.raises(ValueError, match='catalogue'):
        node_measures(G, ['degree', 'betweenness'])
    with pytest.raises(NotImplementedError, match='directed'):
        node_measures(G, ['in_degree'])
    D = nx.gnm_random_graph(30, 90, seed=2, directed=True)
    with pytest.raises(NotImplementedError, match='nx.clustering'):
        node_measures(D, ['clustering'])
    with pytest.raises(NotImplementedError, match='nx.effective_size'):
        node_measures(D, ['effective_size'])
    MG = nx.MultiGraph([(0, 1), (0, 1), (1, 2)])
    for name in ('clustering', 'effective_size', 'eigenvector'):
        with pytest.raises(NotImplementedError):
            node_measures(MG, [name])
    with pytest.raises(ConvergenceError) as info:
        node_measures(G, ['pagerank'], max_iter=2)
    assert info.value.iterations == 2 and isinstance(info.value, RuntimeError)
    with pytest.raises(TypeError):
        node_measures(object())


def test_effective_size_loops_and_isolated(cpu_backend):
    from graphrole_amd import node_measures
    G = nx.Graph([(0, 1), (1, 2), (2, 0), (2, 3), (3, 3), (5, 5)])
    G.add_node(4)
    es = node_measures(G, ['effective_size'])['effective_size']
    ref = nx.effective_size(G.subgraph([0, 1, 2, 3, 4]))
    for v in range(5):
        assert (np.isnan(es[v]) and np.isnan(ref[v])) or es[v] == ref[v], v
    assert np.isnan(es[5])                                     # only neighbour is itself: networkx divides by zero


def _fitted(n=12, r=3, seed=0):
    from graphrole_amd import RoleExtractor
    rng = np.random.default_rng(seed)
    ext = RoleExtractor(n_roles=r)
    index = [f'v{i}' for i in range(n)]
    ext.node_role_factor = pd.DataFrame(rng.random((n, r)), index=index, columns=[f'role_{i}' for i in range(r)])
    return ext


def test_sense_making_checks(cpu_backend):
    from graphrole_amd import RoleExtractor
    M = pd.DataFrame({'a': np.arange(12.0)}, index=[f'v{i}' for i in range(12)])
    with pytest.raises(ValueError, match='extract_role_factors'):
        RoleExtractor(n_roles=2).sense_making(M)
    ext = _fitted()
    with pytest.raises(ValueError, match='labels'):
        ext.sense_making(M.rename(index={'v0': 'other'}))
    with pytest.raises(ValueError, match='labels'):
        ext.sense_making(M.iloc[:5])
    bad = M.copy()
    bad.iloc[[1, 4], 0] = np.nan
    with pytest.raises(ValueError, match=r"'a' has 2 non-finite"):
        ext.sense_making(bad)
    with pytest.raises(ValueError, match='not numeric'):
        ext.sense_making(M.assign(s=['x'] * 12))
    with pytest.raises(NotImplementedError):
        ext.explain()


def test_sense_making_alignment_and_normalize(cpu_backend):
    import scipy.optimize
    ext = _fitted()
    G = ext.node_role_factor.to_numpy()
    rng = np.random.default_rng(1)
    M = pd.DataFrame({'x': G @ np.array([1.0, 0.0, 2.0]), 'y': rng.random(12) * 100, 'z': np.zeros(12)},
                     index=ext.node_role_factor.index)
    E = ext.sense_making(M)
    assert E is ext.role_measure_factor
    assert list(E.index) == ['role_0', 'role_1', 'role_2'] and list(E.columns) == ['x', 'y', 'z']
    np.testing.assert_allclose(E['x'].to_numpy(), [1.0, 0.0, 2.0], atol=1e-9)
    assert np.array_equal(E['z'].to_numpy(), np.zeros(3))
    ref, _ = scipy.optimize.nnls(G, M['y'].to_numpy())
    np.testing.assert_allclose(E['y'].to_numpy(), ref, rtol=1e-8, atol=1e-10)
    shuffled = M.iloc[::-1]
    assert ext.sense_making(shuffled).equals(E)
    En = ext.sense_making(M, normalize=True)
    np.testing.assert_allclose(En['x'].to_numpy(), E['x'].to_numpy() / M['x'].mean(), rtol=1e-9, atol=1e-12)
    assert np.array_equal(En['z'].to_numpy(), np.zeros(3))
