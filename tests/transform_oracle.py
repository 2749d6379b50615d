"""
numpy restatement of ``sklearn.decomposition.NMF(solver='mu').transform(X)`` for the Frobenius loss, i.e.
``_fit_transform(X, H=components_, update_H=False)`` (sklearn 1.7.2, decomposition/_nmf.py): the memberships of the rows
of a new table under a FIXED role x feature factor.  No reference code; checked against sklearn itself by
tools/make_golden_transform.py (same n_iter, |dW| / max|W| <= 5.5e-14 on the recorded cases) and against the recorded
outputs by tests/test_transfer_cpu.py.
"""
import numpy as np

from oracle.rolx import EPSILON, frobenius_error


def transform(X, H, tol=1e-4, max_iter=200):
    """(W, n_iter, info) with info = dict(err_init, err_last, margin): margin is the smallest |ratio - tol| / tol over
    the stopping decisions taken -- how far device rounding is from flipping an iteration count."""
    X = np.asarray(X, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64)
    n, r = X.shape[0], H.shape[0]
    W = np.full((n, r), np.sqrt(X.mean() / r)) if n else np.zeros((0, r))     # _check_w_h, update_H=False
    info = dict(err_init=0.0, err_last=0.0, margin=np.inf)
    if n == 0:
        return W, 0, info
    XHt = X @ H.T                                             # _multiplicative_update_w: formed once
    HHt = H @ H.T
    err_init = frobenius_error(X, W, H)                       # _fit_multiplicative_update: error_at_init
    prev = err_init
    info['err_init'] = info['err_last'] = err_init
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        denom = W @ HHt
        denom[denom == 0] = EPSILON
        W *= XHt / denom
        if tol > 0 and n_iter % 10 == 0:
            err = frobenius_error(X, W, H)
            info['err_last'] = err
            with np.errstate(invalid='ignore', divide='ignore'):
                ratio = np.float64(prev - err) / np.float64(err_init)        # 0 / 0 is nan, as in sklearn
            if np.isfinite(ratio):
                info['margin'] = min(info['margin'], abs(ratio - tol) / tol)
            if ratio < tol:
                break
            prev = err
    return W, n_iter, info


def relmax(a, b):
    """largest difference over largest entry (the metric of tests/test_gpu_rolx.py)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = np.abs(b).max() if b.size else 0.0
    return float(np.abs(a - b).max() / scale) if b.size and scale > 0 else (float(np.abs(a - b).max()) if b.size else 0.0)


def second_table(X, seed):
    """A second table 'of the same kind' as X for the transfer fixtures: rows resampled with replacement, every entry
    scaled by a factor in [0.8, 1.25], and every 7th row zero."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, X.shape[0], size=X.shape[0])
    Y = X[rows] * rng.uniform(0.8, 1.25, size=X.shape)
    Y[::7] = 0.0
    return Y
