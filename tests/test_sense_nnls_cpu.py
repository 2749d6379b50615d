"""
-m "not gpu": grx_host_nnls (host C++ in libgrx.so, no device) against scipy.optimize.nnls on random problems --
full-rank, rank-deficient and zero-column role factors, r = 1 .. 32 roles, up to 200 measures.  The normal equations
are formed here in numpy; on the product path one grx_gram pass over [G | M] forms them.
"""
import ctypes

import numpy as np
import pytest

scipy_optimize = pytest.importorskip('scipy.optimize')


def _nnls(GtG, GtM, mm=None):
    from graphrole_amd import _lib
    lib = _lib.load()
    GtG = np.ascontiguousarray(GtG, dtype=np.float64)
    GtM = np.ascontiguousarray(GtM, dtype=np.float64)
    r, m = GtM.shape
    E = np.zeros((r, m))
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    mm = None if mm is None else np.ascontiguousarray(mm, dtype=np.float64)
    rc = lib.grx_host_nnls(r, m, ptr(GtG), ptr(GtM), ptr(mm), ptr(E))
    assert rc == 0, lib.grx_last_error()
    return E


def _problem(seed):
    rng = np.random.default_rng(seed)
    r = int(rng.integers(1, 33))
    m = int(rng.integers(1, 201))
    n = int(rng.integers(max(r, 2), 400))
    kind = seed % 4
    G = rng.random((n, r))
    if kind == 1 and r > 1:                                   # rank-deficient: columns built from fewer directions
        k = int(rng.integers(1, r))
        G = rng.random((n, k)) @ rng.random((k, r))
    if kind == 2:                                             # all-zero role columns
        G[:, rng.random(r) < 0.3] = 0.0
    if kind == 3 and r > 1:                                   # duplicated columns and a sparse, quantised factor
        G = np.round(G * 4) / 4 * (rng.random((n, r)) < 0.5)
        G[:, -1] = G[:, 0]
    M = rng.random((n, m)) * rng.choice([1.0, 10.0, 1e3], size=m)
    M[:, rng.random(m) < 0.1] = 0.0
    M[:, -1] = G @ rng.random(r)                              # a measure inside the cone of the roles
    return G, M


@pytest.mark.parametrize('seed', range(60))
def test_nnls_matches_scipy(seed):
    G, M = _problem(seed)
    GtG, GtM, mm = G.T @ G, G.T @ M, np.einsum('ij,ij->j', M, M)
    E = _nnls(GtG, GtM, mm)
    assert E.shape == GtM.shape
    assert np.all(E >= 0)
    for j in range(M.shape[1]):
        m = M[:, j]
        e = E[:, j]
        scale = float(m @ m)
        # KKT: gradient g = G^T (G e - m) >= -eps where e = 0, |g| <= eps where e > 0
        g = GtG @ e - GtM[:, j]
        eps = 1e-8 * max(np.sqrt(np.diag(GtG).max() * scale), 1e-300)
        assert np.all(g[e == 0] >= -eps), (j, g[e == 0].min(), eps)
        assert np.all(np.abs(g[e > 0]) <= eps), (j, np.abs(g[e > 0]).max(), eps)
        x_ref, _ = scipy_optimize.nnls(G, m, maxiter=50 * G.shape[1])
        obj = float(np.sum((G @ e - m) ** 2))
        obj_ref = float(np.sum((G @ x_ref - m) ** 2))
        # objectives relative to ||m||^2, the objective at e = 0 (a measure inside the cone has objective ~0)
        assert obj <= obj_ref + 1e-10 * max(scale, 1e-300), (j, obj, obj_ref, scale)
        assert abs(obj - obj_ref) <= 1e-10 * max(scale, 1e-300), (j, obj, obj_ref, scale)


def test_zero_and_degenerate_inputs():
    E = _nnls(np.zeros((3, 3)), np.zeros((3, 2)))
    assert np.array_equal(E, np.zeros((3, 2)))
    # G = [g, g]: one of the two equal roles carries the measure
    g = np.array([1.0, 2.0, 3.0])
    G = np.stack([g, g], axis=1)
    E = _nnls(G.T @ G, G.T @ (2 * g)[:, None])
    assert np.isclose(E.sum(), 2.0) and np.all(E >= 0)
    # a measure pointing away from every role: E = 0
    E = _nnls(np.eye(2), np.array([[-1.0], [-3.0]]))
    assert np.array_equal(E, np.zeros((2, 1)))


def test_argument_checks():
    from graphrole_amd import _lib
    lib = _lib.load()
    assert lib.grx_host_nnls(0, 1, None, None, None, None) == -1
    assert lib.grx_host_nnls(33, 1, None, None, None, None) == -1
    assert b'grx_host_nnls' in lib.grx_last_error()
