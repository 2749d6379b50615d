"""
-m "not gpu": structural similarity on the CPU.  The oracle of the kernel's arithmetic and order
(tests/similarity_oracle.py) against its long-double authority within the derived bound, and the Python layer --
graphrole_amd.nearest_nodes, RoleExtractor.similar_nodes -- over a CPU double defined here: tests/fake_kernels plus a
numpy ``similar_rows`` (the oracle).  The device kernel itself is pinned on the GPU (tests/test_gpu_similarity.py).
"""
import os
import re
import types

import numpy as np
import pandas as pd
import pytest
import torch

from tests import fake_kernels, similarity_oracle as so


# ------------------------------------------------------------------------------------------------- the CPU double
def _similar_rows(X, Q=None, self_rows=None, k=10, metric='cosine', segments=0, c=None, out=None):
    Xh = X.numpy()
    index, score = so.similar_rows(Xh if c is None else Xh[:, :c], None if Q is None else Q.numpy()[:, :c],
                                   None if self_rows is None else self_rows.numpy(), k, metric)
    return torch.from_numpy(index), torch.from_numpy(score)


class _Forbidden:
    """A backend no refusal may reach."""

    def __getattr__(self, name):
        raise AssertionError(f'device work before the refusal: kernels.{name}')


@pytest.fixture
def cpu_backend():
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.similar_rows = _similar_rows
    backend.use(double)
    yield double
    backend.use(None)


@pytest.fixture
def no_backend():
    from graphrole_amd import backend
    backend.use(_Forbidden())
    yield
    backend.use(None)


def _table(n=40, c=4, seed=0, prefix='n'):
    return pd.DataFrame(so.memberships(n, c, seed), index=[f'{prefix}{i:02d}' for i in range(n)],
                        columns=[f'role_{j}' for j in range(c)])


# --------------------------------------------------------------------------------- the oracle against the authority
CASES = so.cases()


@pytest.mark.parametrize('metric', so.METRICS)
@pytest.mark.parametrize('name', list(CASES))
def test_oracle_within_derived_bound_of_the_authority(name, metric):
    case = CASES[name]
    X, k = case['X'], case['k']
    Q = X if case['Q'] is None else case['Q']
    self_rows = np.arange(len(X)) if case['Q'] is None else np.full(len(Q), -1)
    index, score = so.similar_rows(X, case['Q'], case['self_rows'], k, metric)
    exact, bound = so.authority(Q, X, metric)
    sign = so.nearer(metric)
    assert index.shape == (len(Q), k) and (index >= 0).all()          # every case has k admissible candidates
    for q in range(len(Q)):
        got = index[q]
        assert len(set(got.tolist())) == k and self_rows[q] not in got
        assert np.all(np.abs(score[q] - exact[q, got]) <= bound[q, got]), (name, metric, q)
        left = np.setdiff1d(np.arange(len(X)), np.append(got, self_rows[q]))
        if len(left):
            kth = got[-1]
            room = 2 * np.maximum(bound[q, left], bound[q, kth])
            assert np.all(sign * (exact[q, left] - exact[q, kth]) <= room), (name, metric, q)
        # the strict order inside the list: score nearer first, then the smaller row
        s = sign * score[q]
        assert np.all((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (got[:-1] < got[1:]))), (name, metric, q)


def test_exact_cases_by_hand():
    # one-hot rows: every cosine is exactly 0 or 1, every distance 0 or sqrt(2); the row index alone orders the ties
    X = np.eye(3)[[0, 1, 0, 2, 0, 1]]
    index, score = so.similar_rows(X, k=3, metric='cosine')
    assert index.tolist() == [[2, 4, 1], [5, 0, 2], [0, 4, 1], [0, 1, 2], [0, 2, 1], [1, 0, 2]]
    assert score.tolist() == [[1, 1, 0], [1, 0, 0], [1, 1, 0], [0, 0, 0], [1, 1, 0], [1, 0, 0]]
    index, score = so.similar_rows(X, k=2, metric='euclidean')
    assert index[0].tolist() == [2, 4] and score[0].tolist() == [0.0, 0.0] and score[3].tolist() == [np.sqrt(2.0)] * 2
    # a column of ones: every cosine is exactly 1; short lists end in -1 / NaN; -1 in self_rows leaves nothing out
    index, score = so.similar_rows(np.ones((3, 1)), np.ones((2, 1)), np.array([-1, 1]), k=4)
    assert index.tolist() == [[0, 1, 2, -1], [0, 2, -1, -1]]
    assert score[0, :3].tolist() == [1.0] * 3 and np.isnan(score[0, 3]) and np.isnan(score[1, 2:]).all()
    # a zero row scores 0 with everything and symmetric pairs have equal bits
    X = so.memberships(30, 5)
    X[3] = 0.0
    for metric in so.METRICS:
        K = so.keys(X, X, metric)
        assert np.array_equal(K, K.T)
    assert np.all(so.keys(X, X, 'cosine')[3] == 0.0)


def test_adversarial_orders_are_what_they_claim():
    for name, inserted_after_k in (('rising', True), ('falling', False)):
        case = CASES[name]
        for metric in so.METRICS:
            key = so.keys(case['Q'], case['X'], metric)[0]
            assert np.all(np.diff(key) < 0) if inserted_after_k else np.all(np.diff(key) > 0)


# ------------------------------------------------------------------------------------------------ the host path
def test_labels_single_node_and_iterables(cpu_backend):
    from graphrole_amd import nearest_nodes
    T = _table()
    neighbors, scores = nearest_nodes(T, k=5)
    want_index, want_score = so.similar_rows(T.to_numpy(), k=5)
    assert list(neighbors.index) == list(T.index) and list(neighbors.columns) == list(range(5))
    assert neighbors.to_numpy().tolist() == np.asarray(T.index)[want_index].tolist()
    assert scores.to_numpy().tobytes() == want_score.tobytes() and all(dt == np.float64 for dt in scores.dtypes)
    for frame in (neighbors, scores):
        assert frame.attrs == {'metric': 'cosine', 'k': 5}
    one = nearest_nodes(T, 'n07', k=5)
    assert isinstance(one, pd.Series) and one.name == 'cosine' and one.dtype == np.float64
    assert list(one.index) == neighbors.loc['n07'].tolist() and one.to_numpy().tolist() == scores.loc['n07'].tolist()
    some_n, some_s = nearest_nodes(T, ['n07', 'n00', 'n39'], k=5, metric='euclidean')
    all_n, all_s = nearest_nodes(T, k=5, metric='euclidean')
    assert list(some_n.index) == ['n07', 'n00', 'n39'] and some_s.attrs['metric'] == 'euclidean'
    assert some_n.equals(all_n.loc[['n07', 'n00', 'n39']]) and some_s.equals(all_s.loc[['n07', 'n00', 'n39']])
    assert 'n07' not in some_n.loc['n07'].tolist()
    # integer labels keep their dtype; a tuple of labels is an iterable, not a label
    I = pd.DataFrame(T.to_numpy(), index=np.arange(100, 140), columns=T.columns)
    n_i, _ = nearest_nodes(I, (100, 101), k=3)
    assert n_i.to_numpy().dtype.kind == 'i' and n_i.to_numpy().tolist() == (want_index[:2, :3] + 100).tolist()


def test_include_self_and_duplicates(cpu_backend):
    from graphrole_amd import nearest_nodes
    T = _table()
    T.loc['n05'] = T.loc['n02']                                 # a duplicate row is a legitimate neighbour
    with_self_n, with_self_s = nearest_nodes(T, k=3, include_self=True)
    assert with_self_s[0].tolist() == pytest.approx([1.0] * len(T), abs=1e-15)
    assert with_self_n.loc['n02'].tolist()[:2] == ['n02', 'n05'] and with_self_n.loc['n05'].tolist()[:2] == ['n02', 'n05']
    without_n, without_s = nearest_nodes(T, k=3)
    assert all(label not in row.tolist() for label, row in without_n.iterrows())
    assert without_n.loc['n02', 0] == 'n05' and without_n.loc['n05', 0] == 'n02'
    assert without_s.loc['n02', 0] == with_self_s.loc['n02', 0]
    d = nearest_nodes(T, 'n02', k=2, metric='euclidean')
    assert d.index[0] == 'n05' and d.iloc[0] == 0.0


def test_candidates_are_matched_by_label(cpu_backend):
    from graphrole_amd import nearest_nodes
    A, B = _table(12, 4, seed=1, prefix='a'), _table(30, 4, seed=2, prefix='b')
    shuffled = B.iloc[np.random.default_rng(0).permutation(30)][list(B.columns[::-1])]
    neighbors, scores = nearest_nodes(A, ['a03', 'a00'], k=4, candidates=shuffled)
    want_index, want_score = so.similar_rows(shuffled[list(A.columns)].to_numpy(), A.loc[['a03', 'a00']].to_numpy(),
                                             np.full(2, -1), k=4)
    assert neighbors.to_numpy().tolist() == np.asarray(shuffled.index)[want_index].tolist()
    assert scores.to_numpy().tobytes() == want_score.tobytes()
    # the same neighbours whatever the row order of the candidates (no ties in this table)
    plain, plain_scores = nearest_nodes(A, ['a03', 'a00'], k=4, candidates=B)
    assert plain.equals(neighbors) and plain_scores.equals(scores)
    # nothing is left out as self: a table searched in itself through `candidates` finds every row first
    own, _ = nearest_nodes(A, k=1, candidates=A)
    assert own[0].tolist() == list(A.index)
    assert nearest_nodes(A, 'a03', k=30, candidates=B).shape == (30,)


def test_empty_tables_give_empty_frames(cpu_backend):
    from graphrole_amd import nearest_nodes
    empty = pd.DataFrame(np.zeros((0, 3)), columns=['a', 'b', 'c'])
    neighbors, scores = nearest_nodes(empty, k=10)
    assert neighbors.shape == (0, 10) and scores.shape == (0, 10) and scores.attrs == {'metric': 'cosine', 'k': 10}
    neighbors, scores = nearest_nodes(_table(), [], k=3)
    assert neighbors.shape == (0, 3) and scores.shape == (0, 3)


def test_role_extractor_similar_nodes(cpu_backend):
    from graphrole_amd import RoleExtractor
    rx = RoleExtractor(n_roles=4)
    with pytest.raises(ValueError, match='fitted roles'):
        rx.similar_nodes()
    T = _table()
    rx.node_role_factor = T.copy()
    rx.role_feature_factor = pd.DataFrame(np.ones((4, 2)), index=T.columns, columns=['f0', 'f1'])
    before = {name: None if value is None else value.copy() for name, value in vars(rx).items()
              if isinstance(value, pd.DataFrame) or value is None}
    neighbors, scores = rx.similar_nodes(k=6)
    want_index, want_score = so.similar_rows(T.to_numpy(), k=6)
    assert neighbors.to_numpy().tolist() == np.asarray(T.index)[want_index].tolist()
    assert scores.to_numpy().tobytes() == want_score.tobytes()
    one = rx.similar_nodes('n11', k=6, metric='euclidean')
    assert list(one.index) == np.asarray(T.index)[so.similar_rows(T.to_numpy(), k=6, metric='euclidean')[0][11]].tolist()
    other = _table(25, 4, seed=9, prefix='b')
    cross_n, _ = rx.similar_nodes(['n00'], k=3, candidates=other)
    assert set(cross_n.loc['n00']) <= set(other.index)
    given_n, _ = rx.similar_nodes(k=2, memberships=other)
    assert list(given_n.index) == list(other.index)
    rx.node_role_factor.iloc[0] = rx.node_role_factor.iloc[1]   # the frame is read at every call
    assert rx.similar_nodes('n00', k=1).index[0] == 'n01'
    rx.node_role_factor.iloc[0] = T.iloc[0]
    for name, value in before.items():                          # nothing fitted has changed
        now = getattr(rx, name)
        assert (now is None and value is None) or now.equals(value), name


def test_refusals_before_any_device_work(no_backend):
    from graphrole_amd import RoleExtractor, nearest_nodes
    good = _table()
    rx = RoleExtractor(n_roles=4)
    rx.node_role_factor = good

    def both(match, exc=ValueError, **kw):
        table = kw.pop('table', good)
        with pytest.raises(exc, match=match):
            nearest_nodes(table, **kw)
        if table is good:
            with pytest.raises(exc, match=match):
                rx.similar_nodes(**kw)
        else:
            with pytest.raises(exc, match=match):
                rx.similar_nodes(memberships=table, **kw)

    both('non-finite', table=good.assign(role_1=np.nan))
    both('fillna', table=good.assign(role_0=np.inf))
    both('not numeric', table=good.assign(role_2='x'))
    both('DataFrame', table=good.to_numpy())
    both('duplicate', table=pd.concat([good, good.iloc[:1]]))
    both('GRX_MAX_ROLES', table=pd.DataFrame(np.ones((5, 33))))
    both('GRX_MAX_ROLES', table=good.iloc[:, :0])
    for bad_k in (0, -3, 2.5, True):
        both('k must be an integer >= 1', k=bad_k)
    both('GRX_MAX_TOPK', k=65)
    both('only 39 candidates are admissible', k=40)
    both('include_self=True', k=40)
    both('only 40 candidates', k=41, include_self=True)
    both('only 5 candidates', k=6, candidates=good.iloc[:5])
    both("metric must be 'cosine' or 'euclidean'", metric='manhattan')
    both('n99', exc=KeyError, nodes=['n00', 'n99'])
    both('exactly the columns of table', candidates=good.rename(columns={'role_0': 'role_9'}))
    both('exactly the columns of table', candidates=good.iloc[:, :3])
    both('non-finite', candidates=good.assign(role_3=-np.inf))
    both('DataFrame', candidates=good.to_numpy())


# ------------------------------------------------------------------------------------------------------- sklearn
def test_against_sklearn_brute_force(cpu_backend):
    NearestNeighbors = pytest.importorskip('sklearn.neighbors').NearestNeighbors
    from graphrole_amd import nearest_nodes
    k = 8
    T = _table(120, 6, seed=2)
    X = T.to_numpy()
    for metric in so.METRICS:
        # the comparison means something only where the authority separates rank k from rank k + 1 by more than the
        # rounding of either side: asserted here, for every query
        exact, bound = so.authority(X, X, metric)
        sign = so.nearer(metric)
        ranked = sign * exact
        np.fill_diagonal(ranked, -np.inf)
        order = np.argsort(-ranked, axis=1, kind='stable')
        rows = np.arange(len(X))
        gap = ranked[rows, order[:, k - 1]] - ranked[rows, order[:, k]]
        assert np.all(gap > 2 * np.maximum(bound[rows, order[:, k - 1]], bound[rows, order[:, k]])), metric
        nn = NearestNeighbors(n_neighbors=k + 1, algorithm='brute', metric=metric).fit(X)
        dist, ind = nn.kneighbors(X)
        neighbors, scores = nearest_nodes(T, k=k, metric=metric)
        for q in range(len(X)):
            theirs = [i for i in ind[q] if i != q][:k]
            assert set(np.asarray(T.index)[theirs]) == set(neighbors.iloc[q]), (metric, q)
        theirs = np.sort(np.where(ind == rows[:, None], np.inf, dist), axis=1)[:, :k]
        ours = np.sort(1.0 - scores.to_numpy() if metric == 'cosine' else scores.to_numpy(), axis=1)
        np.testing.assert_allclose(ours, theirs, rtol=0, atol=1e-12 if metric == 'cosine' else 1e-7)


# ----------------------------------------------------------------------------------------------------------- ABI
def test_entry_points_are_declared_and_bound():
    from graphrole_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'grx.h')).read()
    for name in ('grx_similar_rows', 'grx_similar_rows_workspace_bytes'):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)
        assert re.search(r'\b' + name + r'\(int64_t n', header)
    assert re.search(r'#define\s+GRX_VERSION\s+1100\b', header)
    assert re.search(r'#define\s+GRX_MAX_TOPK\s+64\b', header) and 'GRX_SIMILARITY_EUCLIDEAN' in header
    lib = _lib.load()
    # argument checks need no device
    args = lambda **kw: [kw.get(key, default) for key, default in (
        ('n', 10), ('c', 3), ('X', None), ('ldx', 3), ('nq', 10), ('Q', None), ('ldq', 3), ('self', None), ('k', 2),
        ('metric', 0), ('segments', 0), ('index', None), ('score', None), ('ld_out', 2), ('ws', None), ('ws_bytes', 0),
        ('stream', None))]
    assert lib.grx_similar_rows(*args()) == -1 and b'null pointer' in lib.grx_last_error()
    assert lib.grx_similar_rows(*args(c=33, ldx=33, ldq=33)) == -4 and b'GRX_MAX_ROLES' in lib.grx_last_error()
    assert lib.grx_similar_rows(*args(k=65, ld_out=65)) == -1 and b'GRX_MAX_TOPK' in lib.grx_last_error()
    assert lib.grx_similar_rows(*args(nq=0)) == 0
    assert lib.grx_similar_rows_workspace_bytes(1000, 10, 6, 10, 1) >= (1000 + 10) * 6 * 8
    assert lib.grx_similar_rows_workspace_bytes(1000, 10, 6, 10, 4) > lib.grx_similar_rows_workspace_bytes(1000, 10, 6, 10, 1)
