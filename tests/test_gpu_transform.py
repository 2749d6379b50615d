"""
-m gpu: grx_nmf_transform (csrc/grx_transform.hip) through graphrole_amd.kernels against sklearn's recorded
``NMF(solver='mu').transform`` outputs (tests/golden/transform_*.npz, tools/make_golden_transform.py) and against the
numpy restatement tests/transform_oracle.py: equal iteration counts, memberships within FACTOR_RTOL = 1e-8 (largest
difference over largest entry -- the bound the fitted factors are held to, tests/test_gpu_rolx.py).

Shapes: every rank at which the block kernel is another instantiation class (1, 2, 3, 6; 17 and 32 take the two-launch
projection), row counts around the wavefront (1, 63, 65) and over several workgroups (700), leading dimensions above n
with NaN in the padding, n < F, F above the single-launch limit of the fit, zero rows, a dead role, an exactly
factorisable table (direct residual branch), a short last block, tol = 0, an all-zero table.
"""
import numpy as np
import pytest

from tests import transform_oracle, util

pytestmark = pytest.mark.gpu

FACTOR_RTOL = 1e-8
#: a stopping decision of the oracle must be at least this far (relative to tol) from tol for an input to be usable:
#: the device's error differs from numpy's by rounding (~1e-13 relative), five orders below this
MIN_MARGIN = 1e-6


def _device_transform(X, H, tol=1e-4, max_iter=200, pad=5):
    """(W n x r host, NmfInfo) of grx_nmf_transform on X with ldx = ldw = n + pad, NaN behind the valid rows of X and a
    sentinel behind those of W (which must survive)."""
    from graphrole_amd import kernels as K
    n, F = X.shape
    r = H.shape[0]
    Xp = np.full((F, n + pad), np.nan)
    Xp[:, :n] = X.T
    Wp = np.full((r, n + pad), -7.0)
    Xd, Wd = K.to_device(Xp), K.to_device(Wp)
    Wd, info = K.nmf_transform(Xd, n, H, tol, max_iter, out=Wd)
    Wh = K.to_host(Wd)
    assert (Wh[:, n:] == -7.0).all(), 'rows behind n were written'
    return np.ascontiguousarray(Wh[:, :n].T), info


def _check(X, H, tol=1e-4, max_iter=200, expect=None):
    Wo, it, oinfo = transform_oracle.transform(X, H, tol, max_iter)
    assert oinfo['margin'] > MIN_MARGIN, f'unusable input: a stopping decision within {oinfo["margin"]:.2e} of tol'
    W, info = _device_transform(X, H, tol, max_iter)
    err = transform_oracle.relmax(W, Wo)
    print(f'n={X.shape[0]} F={X.shape[1]} r={H.shape[0]} n_iter={info.n_iter} direct={info.direct_residuals} relmax={err:.3e}')
    assert info.n_iter == it
    assert (W >= 0).all()
    assert err < FACTOR_RTOL, err
    if expect is not None:
        assert transform_oracle.relmax(W, expect) < FACTOR_RTOL
    assert abs(info.x_sq_norm - float((X * X).sum())) <= 1e-12 * max(float((X * X).sum()), 1e-300)
    if it:
        assert abs(info.err_init - oinfo['err_init']) <= 1e-9 * oinfo['err_init']
    return W, info


@pytest.mark.parametrize('name', util.NMF_CASES)
@pytest.mark.parametrize('tag', ['same', 'second'])
def test_transform_matches_sklearn_golden(name, tag):
    g = util.load_nmf(name)
    t = np.load(util.golden_path(f'transform_{name}.npz'))
    X = g['X'] if tag == 'same' else t['X2']
    _, info = _check(X, g['H'], expect=t[f'W_{tag}'])
    assert info.n_iter == int(t[f'n_iter_{tag}'])
    if tag == 'second':
        W, _ = _device_transform(X, g['H'])
        assert (W[::7] == 0).all(), 'a zero row of X gives a zero row of W'


def _random_case(n, F, r, seed):
    rng = np.random.default_rng(seed)
    H = rng.uniform(0.0, 2.0, size=(r, F)) * (rng.uniform(size=(r, F)) < 0.6)
    X = rng.gamma(1.0, 1.0, size=(n, r)) @ H + rng.uniform(0.0, 0.3, size=(n, F))
    return X, H


@pytest.mark.parametrize('r', [1, 2, 3, 6, 17, 32])
@pytest.mark.parametrize('n', [1, 63, 65, 700])
def test_transform_shapes(n, r):
    X, H = _random_case(n, 40 if r > 6 else 11, r, seed=100 * r + n)
    _check(X, H)


def test_transform_wide_table():
    """F = 130 is above the 120 columns the fit's single-launch passes take"""
    X, H = _random_case(200, 130, 6, seed=5)
    _check(X, H)


def test_transform_dead_role():
    g = util.load_nmf('er2000_r6')
    H = g['H'].copy()
    H[2] = 0.0
    W, _ = _check(g['X'], H)
    assert (W[:, 2] == 0).all()


def test_transform_exact_rank_one_takes_the_direct_residual():
    rng = np.random.default_rng(9)
    w, h = rng.uniform(0.5, 3.0, size=(300, 1)), rng.uniform(0.5, 2.0, size=(1, 9))
    _, info = _check(w @ h, h, expect=w)
    assert info.direct_residuals > 0
    assert info.err_last <= 1e-7 * info.err_init


def test_transform_short_last_block_and_tol_zero():
    g = util.load_nmf('dw200_r5')                             # 130 iterations with the defaults
    _, info = _check(g['X'], g['H'], max_iter=25)
    assert info.n_iter == 25
    _, info = _check(g['X'], g['H'], tol=0.0, max_iter=30)
    assert info.n_iter == 30
    g = util.load_nmf('rand3000x9_r2')                        # stops at 20 with the defaults: not with tol = 0
    _, info = _check(g['X'], g['H'], tol=0.0, max_iter=30)
    assert info.n_iter == 30


def test_transform_all_zero_table_and_no_rows():
    from graphrole_amd import kernels as K
    H = util.load_nmf('karate_r4')['H']
    W, info = _device_transform(np.zeros((50, H.shape[1])), H, max_iter=40)
    assert (W == 0).all() and info.n_iter == 40               # sklearn's 0 / 0 comparison never stops
    Wo, it, _ = transform_oracle.transform(np.zeros((50, H.shape[1])), H, max_iter=40)
    assert it == 40 and (Wo == 0).all()
    Wd, info = K.nmf_transform(K.zeros((H.shape[1], 1)), 0, H)
    assert info.n_iter == 0


def test_transform_is_bitwise_reproducible():
    g = util.load_nmf('ba2000_r6')
    a, ia = _device_transform(g['X'], g['H'])
    b, ib = _device_transform(g['X'], g['H'])
    assert ia.n_iter == ib.n_iter and ia.err_last == ib.err_last
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
