"""
-m gpu: role transfer end to end -- roles fitted on one graph (ba300, numpy seeded as tests/golden/roles_ba300.npz
states), its feature columns replayed on another (er300), ``RoleExtractor.transform`` / ``transform_roles`` on that
table -- against the numpy restatement of sklearn's ``NMF(solver='mu').transform`` (tests/transform_oracle.py) applied
to the ORACLE's replayed table (tests/replay_oracle.py) and the fitted ``role_feature_factor``, within FACTOR_RTOL.
"""
import numpy as np
import pandas as pd
import pytest

from tests import replay_oracle, transform_oracle, util
from tests.test_gpu_refex import _graph_for

pytestmark = pytest.mark.gpu

FACTOR_RTOL = 1e-8


@pytest.fixture(scope='module')
def transfer():
    from graphrole_amd import RecursiveFeatureExtractor, RoleExtractor
    ga, gb = util.load_refex('ba300'), util.load_refex('er300')
    Ga, kwa = _graph_for('ba300', ga)
    Gb, kwb = _graph_for('er300', gb)
    features = RecursiveFeatureExtractor(Ga, **kwa).extract_features()
    np.random.seed(int(util.load_roles('ba300')['seed']))
    rx = RoleExtractor(n_roles=3)
    rx.extract_role_factors(features)
    fitted = (rx.node_role_factor.copy(), rx.role_feature_factor.copy())
    features_b = RecursiveFeatureExtractor(Gb, **kwb).replay_features(features.columns)
    og = util.oracle_graph_from_golden(gb)
    names0, cols0 = util.typed_gen0(gb)
    ref = replay_oracle.replay(og, names0, cols0, list(features.columns))
    Xo = np.column_stack([ref[c].astype(np.float64) for c in features.columns])
    Wo, n_iter, info = transform_oracle.transform(Xo, fitted[1].to_numpy())
    assert info['margin'] > 1e-6, 'unusable input: a stopping decision at tol'
    return rx, fitted, features, features_b, Wo, n_iter


def test_transform_matches_the_oracle(transfer):
    rx, fitted, features, features_b, Wo, n_iter = transfer
    W = rx.transform(features_b)
    assert list(W.index) == list(features_b.index) and list(W.columns) == ['role_0', 'role_1', 'role_2']
    assert W.attrs['n_iter'] == n_iter
    err = transform_oracle.relmax(W.to_numpy(), Wo)
    print(f'transfer ba300 -> er300: n_iter {n_iter}, relmax {err:.3e}')
    assert err < FACTOR_RTOL
    # nothing fitted moved
    assert rx.node_role_factor.equals(fitted[0]) and rx.role_feature_factor.equals(fitted[1])


def test_column_order_and_the_handoff_do_not_matter(transfer):
    from graphrole_amd import kernels as K
    from graphrole_amd.features import handoff
    rx, _, features, features_b, _, _ = transfer
    assert handoff.lookup(K, features_b) is not None, 'the replayed frame is registered for the device hand-off'
    W = rx.transform(features_b)
    copy = features_b.copy()
    assert handoff.lookup(K, copy) is None
    assert np.array_equal(rx.transform(copy).to_numpy().view(np.int64), W.to_numpy().view(np.int64))
    shuffled = features_b[list(features_b.columns[::-1])]
    Ws = rx.transform(shuffled)
    assert np.array_equal(Ws.to_numpy().view(np.int64), W.to_numpy().view(np.int64))
    assert Ws.attrs['n_iter'] == W.attrs['n_iter']


def test_transform_roles_is_the_first_maximum(transfer):
    rx, fitted, _, features_b, _, _ = transfer
    W = rx.transform(features_b)
    roles = rx.transform_roles(features_b)
    assert list(roles) == list(features_b.index)
    assert roles == W.idxmax(axis=1).to_dict()
    assert rx.node_role_factor.equals(fitted[0]) and rx.role_feature_factor.equals(fitted[1])
    # transforming the table of the fit itself is allowed too (not the fitted memberships: H is the encoded factor)
    assert rx.transform(transfer[2]).shape == fitted[0].shape


def test_input_checks_on_the_device(transfer):
    rx, _, _, features_b, _, _ = transfer
    bad = features_b.astype(np.float64)
    bad.iloc[3, 1] = np.nan
    with pytest.raises(ValueError, match='NaN'):
        rx.transform(bad)
    bad.iloc[3, 1] = -1.0
    with pytest.raises(ValueError, match='Negative'):
        rx.transform(bad)
    assert rx.transform(features_b, max_iter=15).attrs['n_iter'] == 15
    assert rx.transform(features_b, tol=0.0, max_iter=30).attrs['n_iter'] == 30
