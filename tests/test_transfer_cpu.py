"""
-m "not gpu": role transfer without a device -- the name parser of ``replay_features``, every refusal of
``RecursiveFeatureExtractor.replay_features`` and ``RoleExtractor.transform`` that is raised before device work,
the argument validation of grx_nmf_transform (no HIP call), the numpy restatement tests/transform_oracle.py against
sklearn's recorded outputs, and the Python layers of both over the CPU double tests/fake_kernels (+ the oracle as
``nmf_transform``).  The numbers of the device path are pinned in tests/test_gpu_transform.py, test_gpu_replay.py and
test_gpu_transfer.py.
"""
import ctypes
import types

import networkx as nx
import numpy as np
import pandas as pd
import pytest
import torch

from tests import fake_kernels, replay_oracle, transform_oracle, util


# ------------------------------------------------------------------------------------------------ name parser
@pytest.mark.parametrize('name,gen0,expected', replay_oracle.PARSER_CASES)
def test_parse_feature_name(name, gen0, expected):
    from graphrole_amd.features.extract import parse_feature_name
    assert parse_feature_name(name, gen0) == expected
    assert replay_oracle.parse(name, gen0) == expected


def test_parser_round_trips_every_recorded_candidate_name():
    from graphrole_amd.features.extract import parse_feature_name
    for case in ['ba300', 'dw200_attrs', 'directed120', 'ba300_stdvar']:
        g = util.load_refex(case)
        gen0 = g.js('gen0_names')
        for gen in range(int(g['n_generations_recorded'])):
            for name in g.js(f'g{gen}_cand_names'):
                base, chain = parse_feature_name(name, gen0)
                assert base in gen0 and len(chain) == gen
                assert base + ''.join(f'({a})' for a in chain) == name


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize('name', util.NMF_CASES)
def test_transform_oracle_matches_sklearn_golden(name):
    g = util.load_nmf(name)
    t = np.load(util.golden_path(f'transform_{name}.npz'))
    for tag, X in (('same', g['X']), ('second', t['X2'])):
        W, n_iter, info = transform_oracle.transform(X, g['H'])
        assert n_iter == int(t[f'n_iter_{tag}'])
        assert transform_oracle.relmax(W, t[f'W_{tag}']) < 1e-12
        assert info['margin'] > 1e-3                          # no stopping decision near tol: n_iter is robust
    assert np.array_equal(t['X2'], transform_oracle.second_table(g['X'], int(t['seed'])))
    assert (t['X2'][::7] == 0).all() and (t['W_second'][::7] == 0).all()


def test_transform_oracle_edge_cases():
    H = util.load_nmf('karate_r4')['H']
    W, n_iter, _ = transform_oracle.transform(np.zeros((5, H.shape[1])), H, max_iter=30)
    assert n_iter == 30 and (W == 0).all()
    W, n_iter, _ = transform_oracle.transform(np.zeros((0, H.shape[1])), H)
    assert n_iter == 0 and W.shape == (0, 4)
    X = util.load_nmf('karate_r4')['X']
    assert transform_oracle.transform(X, H, max_iter=25)[1] == 25
    assert transform_oracle.transform(X, H, tol=0.0, max_iter=30)[1] == 30


# ------------------------------------------------------------------------------------------------ the ABI
def test_nmf_transform_argument_validation_needs_no_device():
    from graphrole_amd import _lib
    lib = _lib.load()
    info = _lib.NmfInfo()
    tol = ctypes.c_double(1e-4)
    H = np.ones((3, 5))
    hp = H.ctypes.data_as(ctypes.c_void_p)

    def call(n=10, F=5, r=3, X=None, ldx=10, h=hp, tol=tol, max_iter=200, W=None, ldw=10, info=ctypes.byref(info)):
        return lib.grx_nmf_transform(n, F, r, X, ldx, h, tol, max_iter, W, ldw, info, None, 0, None)

    assert call(F=500) == -4 and b'compiled limits' in lib.grx_last_error()          # GRX_ERR_UNSUPPORTED
    assert call(r=33) == -4 and call(r=0) == -4 and call(F=0) == -4
    assert call(r=17, F=470) == -4                                                   # r + F <= 480 above 16 roles
    assert call(n=-1) == -1
    assert call(ldx=9) == -1 and b'leading dimension' in lib.grx_last_error()
    assert call(ldw=9) == -1
    assert call(max_iter=-1) == -1
    assert call(tol=ctypes.c_double(-1.0)) == -1
    assert call(info=None) == -1
    assert call() == -1 and b'NULL' in lib.grx_last_error()                          # n > 0 and no table
    info.n_iter = 99
    assert call(n=0, ldx=0, ldw=0) == 0 and info.n_iter == 0                         # no rows: returns at once
    with pytest.raises(ValueError):
        _lib.call('grx_nmf_transform', 10, 5, 3, None, 9, hp, tol, 200, None, 10, ctypes.byref(info), None, 0, None)
    a, b = lib.grx_nmf_transform_workspace_bytes(1_000_000, 20, 6), lib.grx_nmf_transform_workspace_bytes(2_000_000, 20, 6)
    assert 6 * 8 * 1_000_000 < a < b


# ------------------------------------------------------------------------------------------------ Python layers
def _nmf_transform(X, n, H, tol=1e-4, max_iter=200, out=None):
    W, n_iter, info = transform_oracle.transform(X.numpy()[:, :n].T, H, tol, max_iter)
    return torch.from_numpy(np.ascontiguousarray(W.T)), types.SimpleNamespace(n_iter=n_iter, **info)


@pytest.fixture
def cpu_double():
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.nmf_transform = _nmf_transform
    backend.use(double)
    yield double
    backend.use(None)


def _fitted(columns, r=3, index=range(6)):
    from graphrole_amd import RoleExtractor
    rx = RoleExtractor(n_roles=r)
    roles = [f'role_{i}' for i in range(r)]
    rng = np.random.default_rng(0)
    rx.node_role_factor = pd.DataFrame(rng.uniform(size=(len(index), r)), index=list(index), columns=roles)
    rx.role_feature_factor = pd.DataFrame(rng.uniform(size=(r, len(columns))), index=roles, columns=list(columns))
    return rx


def test_transform_refusals_before_device_work():
    """none of these reaches the backend: there is no device here and no double installed"""
    from graphrole_amd import RoleExtractor
    X = pd.DataFrame(np.ones((4, 3)), columns=['a', 'b', 'c'])
    with pytest.raises(ValueError, match='fitted roles'):
        RoleExtractor(n_roles=2).transform(X)
    rx = _fitted(['a', 'b', 'c'])
    with pytest.raises(ValueError, match='DataFrame'):
        rx.transform(X.to_numpy())
    with pytest.raises(ValueError, match=r"missing \['c'\].*unexpected \['d'\]"):
        rx.transform(X.rename(columns={'c': 'd'}))
    with pytest.raises(ValueError, match=r"missing \[\].*unexpected \['z'\]"):
        rx.transform(X.assign(z=1.0))
    with pytest.raises(ValueError, match=r"missing \['b'\]"):
        rx.transform(X.drop(columns='b'))
    with pytest.raises(ValueError, match='duplicate'):
        rx.transform(pd.concat([X, X[['a']]], axis=1))
    with pytest.raises(ValueError, match='fitted roles'):
        RoleExtractor(n_roles=2).transform_roles(X)
    dist = _fitted(['a', 'b', 'c'])
    dist.distributed = True
    with pytest.raises(NotImplementedError, match='sharded'):
        dist.transform(X)
    bad = _fitted(['a', 'b', 'c'])
    bad.role_feature_factor.iloc[0, 0] = -1.0
    with pytest.raises(ValueError, match='non-negative'):
        bad.transform(X)


def test_transform_python_layer_over_the_double(cpu_double):
    rng = np.random.default_rng(4)
    rx = _fitted(['a', 'b', 'c', 'd'], r=3, index=range(40))
    X = pd.DataFrame(rng.uniform(size=(25, 4)), index=[f'n{i}' for i in range(25)], columns=['a', 'b', 'c', 'd'])
    before = (rx.node_role_factor.copy(), rx.role_feature_factor.copy())
    W = rx.transform(X)
    Wo, it, _ = transform_oracle.transform(X.to_numpy(), rx.role_feature_factor.to_numpy())
    assert list(W.index) == list(X.index) and list(W.columns) == ['role_0', 'role_1', 'role_2']
    assert W.attrs['n_iter'] == it and np.array_equal(W.to_numpy(), Wo)
    # columns are matched by label: any order gives the same table
    assert rx.transform(X[['d', 'b', 'a', 'c']]).equals(W)
    roles = rx.transform_roles(X)
    assert roles == W.idxmax(axis=1).to_dict()
    # H is the CURRENT content of role_feature_factor
    rx.role_feature_factor.iloc[1] = 0.0
    assert (rx.transform(X)['role_1'] == 0).all()
    rx.role_feature_factor = before[1].copy()
    assert rx.node_role_factor.equals(before[0]) and rx.transform(X).equals(W)
    assert rx.transform(X, max_iter=7).attrs['n_iter'] == 7
    # the fit's input check (the NaN check is the device pass of factor.device_matrix: tests/test_gpu_transfer.py)
    with pytest.raises(ValueError, match='Negative'):
        rx.transform(X - 1.0)
    empty = rx.transform(X.iloc[:0])
    assert empty.shape == (0, 3) and empty.attrs['n_iter'] == 0 and rx.transform_roles(X.iloc[:0]) == {}


def _attr_graph():
    G = nx.barabasi_albert_graph(30, 2, seed=1)
    for v in G.nodes:
        G.nodes[v]['f(x)'] = float(v % 5)
    return G


def test_replay_refusals_before_device_work():
    """no double installed: anything that reached the backend would raise GrxError('no CPU fallback')"""
    from graphrole_amd import RecursiveFeatureExtractor, backend
    backend.use(None)
    G = _attr_graph()
    fe = RecursiveFeatureExtractor(G, attributes=True)
    assert fe.graph.neighborhood_feature_names() == ['degree', 'attribute_f(x)', 'internal_edges', 'external_edges']
    with pytest.raises(ValueError) as e:
        fe.replay_features(['degree(sum)', 'bogus(sum)', 'in_degree', 'attribute_f(sum)', 'attribute_f(x)(mean)'])
    assert "['bogus(sum)', 'in_degree', 'attribute_f(sum)']" in str(e.value)
    with pytest.raises(NotImplementedError, match=r"\['sem'\]"):
        fe.replay_features(['degree(sum)', 'degree(sem)'])
    with pytest.raises(NotImplementedError, match='spread'):
        fe.replay_features(['degree(spread)(sum)'])
    with pytest.raises(NotImplementedError, match='sem'):
        RecursiveFeatureExtractor(G, aggs=['sum', 'sem']).replay_features(['degree(sum)'])
    with pytest.raises(NotImplementedError, match='distributed'):
        RecursiveFeatureExtractor(G, distributed=True).replay_features(['degree'])
    empty = fe.replay_features([])
    assert empty.shape == (30, 0) and list(empty.index) == sorted(G.nodes)
    assert RecursiveFeatureExtractor(nx.DiGraph(G)).graph.neighborhood_feature_names() == \
        ['in_degree', 'out_degree', 'total_degree', 'internal_edges', 'external_edges']


def test_replay_python_layer_over_the_double(cpu_double):
    """the chain logic (needed parents only, request order, dtypes, untouched state) on the CPU double"""
    from graphrole_amd import RecursiveFeatureExtractor
    from tests.test_gpu_refex import _graph_for
    g = util.load_refex('ba300')
    G, kwargs = _graph_for('ba300', g)
    fe = RecursiveFeatureExtractor(G, native_loop=False, **kwargs)
    F = fe.extract_features()
    state = (list(fe._work), dict(fe._dtypes), {k: list(v) for k, v in fe._final_names.items()}, fe.generation_count)
    R = fe.replay_features(F.columns)
    assert R.equals(F) and [str(t) for t in R.dtypes] == g.js('final_dtypes')
    assert (list(fe._work), dict(fe._dtypes), {k: list(v) for k, v in fe._final_names.items()}, fe.generation_count) == state
    assert fe.extract_features().equals(F)
    # candidates the pruner dropped, in another order, generation 0 included
    names = g.js('g2_cand_names')[::-1] + ['degree'] + g.js('g1_cand_names')[:2]
    R = RecursiveFeatureExtractor(G, **kwargs).replay_features(names)
    assert list(R.columns) == names
    want = dict(zip(g.js('g2_cand_names'), g['g2_cand_values'].T))
    want.update(zip(g.js('g1_cand_names'), g['g1_cand_values'].T), degree=g['gen0_values'][:, 0])
    for nm in names:
        np.testing.assert_allclose(R[nm].to_numpy(dtype=np.float64), want[nm], rtol=1e-12, err_msg=nm)
    assert R['degree'].dtype == np.int64 and R[names[0]].dtype == np.float64
    # an attribute name with parentheses, and the oracle chain
    A = _attr_graph()
    fa = RecursiveFeatureExtractor(A, attributes=True, aggs=['sum', 'max'])
    cols = ['attribute_f(x)(sum)(max)', 'attribute_f(x)', 'degree(max)']
    R = fa.replay_features(cols)
    from oracle import refex
    og = refex.graph_from_networkx(A, attributes=True)
    names0, block0 = refex.neighborhood_features(og)
    gen0 = [block0[:, j].astype(np.int64) if nm != 'attribute_f(x)' else block0[:, j] for j, nm in enumerate(names0)]
    ref = replay_oracle.replay(og, names0, gen0, cols, aggs=['sum', 'max'])
    for nm in cols:
        assert R[nm].dtype == ref[nm].dtype and np.array_equal(R[nm].to_numpy(), ref[nm]), nm
