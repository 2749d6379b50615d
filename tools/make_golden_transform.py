#!/usr/bin/env python3
"""
tools/make_golden_transform.py -- role-transfer fixtures (tests/golden/transform_<case>.npz) by RUNNING scikit-learn's
``NMF(solver='mu').transform`` on a CPU host, for every fitted factor pair of tests/golden/nmf_<case>.npz:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_transform.py

Per case: the second table (tests/transform_oracle.py::second_table of the fitted table: resampled rows, rescaled
entries, every 7th row zero), sklearn's transform output for the fitted table itself and for the second table under the
recorded role x feature factor H, and both iteration counts.  The numpy restatement tests/transform_oracle.py is
checked against sklearn on the way (same n_iter; the largest difference and the closest any stopping decision comes to
tol are printed).  The fixtures are data; sklearn is imported here and only here.
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
warnings.simplefilter('ignore')

from sklearn.decomposition import NMF                                     # noqa: E402

from tests import transform_oracle, util                                 # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
SEED = 11


def sklearn_transform(X, H, tol=1e-4, max_iter=200):
    """(W, n_iter) of NMF(solver='mu').transform(X) with components_ = H (transform itself drops n_iter, so the call
    it makes is repeated here and compared)."""
    r, F = H.shape
    model = NMF(n_components=r, solver='mu', init='nndsvda', tol=tol, max_iter=max_iter)
    model.components_ = H.copy()
    model.n_components_ = r
    model.n_features_in_ = F
    W = model.transform(X)
    W2, _, n_iter = model._fit_transform(X, H=model.components_, update_H=False)
    assert np.array_equal(W, W2)
    return W, int(n_iter)


def main():
    import sklearn
    worst, closest = 0.0, np.inf
    for case in util.NMF_CASES:
        g = util.load_nmf(case)
        X, H = g['X'], g['H']
        X2 = transform_oracle.second_table(X, SEED)
        out = {}
        for tag, table in (('same', X), ('second', X2)):
            W, n_iter = sklearn_transform(table, H)
            Wo, it, info = transform_oracle.transform(table, H)
            assert it == n_iter, (case, tag, it, n_iter)
            worst = max(worst, transform_oracle.relmax(Wo, W))
            closest = min(closest, info['margin'])
            out[f'W_{tag}'], out[f'n_iter_{tag}'] = W, n_iter
            print(f'{case:16s} {tag:6s} n_iter {n_iter:3d}  oracle vs sklearn {transform_oracle.relmax(Wo, W):.2e}  '
                  f'margin {info["margin"]:.3g}')
        path = os.path.join(OUT, f'transform_{case}.npz')
        np.savez_compressed(path, X2=X2, seed=SEED, sklearn_version=sklearn.__version__, **out)
        print(f'  -> {os.path.relpath(path, ROOT)} {os.path.getsize(path)} bytes')
    print(f'largest |dW| / max|W| oracle vs sklearn: {worst:.2e}; closest stopping decision: {closest:.3g} of tol')


if __name__ == '__main__':
    main()
