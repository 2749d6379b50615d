"""
GPU: structural similarity.  grx_similar_rows (csrc/grx_similarity.hip) against the numpy restatement of its arithmetic
and order (tests/similarity_oracle.py) bit for bit, index bytes and score bytes both, every call made twice.

The shapes are a cross-section, not the product.  The kernel has four independent places where a size changes the path,
and each group below walks one of them with the others held at a value that already crosses every tile once
(n = 2 TC + 3 candidates in three tiles, so that segments 0, 1, 2, 3 and more-than-tiles all differ; c = 5 or 6, the
first padded and the first exact width):
  'n'   n in {1, 2, k, k + 1, TC - 1, TC, TC + 1, 2 TC + 3}: the candidate tile and its ragged end, the short lists, and
        the whole set of `segments` (0, 1, 2, 3, the largest the library chooses, one above the tile count) -- a segment
        boundary only exists relative to n, so the two are varied together; the rows query themselves (Q=None).
  'nq'  nq in {1, TQ - 1, TQ, TQ + 1}: the query tile, its idle lanes and its second workgroup, with an external Q and a
        d_self that mixes rows to leave out with -1.
  'c'   c in {1, 2, 5, 6, 17, 32}: every compiled width class once exact and once padded, each also with the leading
        dimension c + 3 on X and on Q (the columns behind c hold values that would change every score if read).
  'k'   k in {1, 2, 10, 16, 17, 64}: the list length, with both sides of the threshold between the two compiled list
        capacities (SIM_SMALL_K = 16).
Both metrics run everywhere.  The selection never looks at c and the arithmetic never looks at k or at the segments, so
crossing the groups would re-run the same code on the same data paths.  Then every case class of the oracle (one-hot
ties, duplicates, zero rows, the column of ones, both adversarial arrival orders), short lists at kernel level, the
symmetry of the scores, the argument contract, and the public interface end to end.
"""
import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import graphs, similarity_oracle as so

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    from graphrole_amd import kernels
    return kernels


def _check(K, got, want, what):
    index, score = (np.asarray(K.to_host(t)) for t in got)
    assert index.dtype == np.int32 and score.dtype == np.float64 and index.shape == want[0].shape, what
    assert index.tobytes() == want[0].tobytes(), (what, 'index')
    assert score.tobytes() == want[1].tobytes(), (what, 'score')


def _padded(rng, A, extra=3):
    """A with `extra` columns of noise behind it: the leading dimension c + 3."""
    return np.concatenate([A, rng.standard_normal((len(A), extra)) * 7.0], axis=1)


def _shapes(K):
    TQ, TC, top = K.similarity_shape()
    assert (TQ, TC, top) == (K.SIM_QUERY_TILE, K.SIM_CANDIDATE_TILE, K.SIM_MAX_SEGMENTS)
    all_segments = (0, 1, 2, 3, top, 2 * TC + 3)
    big = 2 * TC + 3
    out = []
    for n in (1, 2, 10, 11, TC - 1, TC, TC + 1, big):
        out.append(dict(group='n', n=n, nq=None, c=5, k=10, segments=all_segments, pad=False))
    for nq in (1, TQ - 1, TQ, TQ + 1):
        out.append(dict(group='nq', n=big, nq=nq, c=6, k=10, segments=(0, 2), pad=False))
    for c in (1, 2, 5, 6, 17, 32):
        out.append(dict(group='c', n=big, nq=70, c=c, k=10, segments=(1, 3), pad=False))
        out.append(dict(group='c', n=big, nq=70, c=c, k=10, segments=(1, 3), pad=True))
    for k in (1, 2, 10, K.SIM_SMALL_K, K.SIM_SMALL_K + 1, K.MAX_TOPK):
        out.append(dict(group='k', n=big, nq=None, c=6, k=k, segments=(0, 3), pad=False))
    return out


def test_bit_parity_with_the_oracle(K):
    assert K.MAX_TOPK == 64
    for shape in _shapes(K):
        n, nq, c, k = shape['n'], shape['nq'], shape['c'], shape['k']
        rng = np.random.default_rng(1000 * n + 10 * c + k)
        X = so.memberships(n, c, seed=1)
        Q = None if nq is None else so.memberships(nq, c, seed=2)
        self_rows = None
        if Q is not None:                                       # rows to leave out mixed with -1
            self_rows = np.where(rng.random(nq) < 0.5, rng.integers(0, n, nq), -1).astype(np.int32)
        Xd = K.to_device(_padded(rng, X) if shape['pad'] else X)
        Qd = None if Q is None else K.to_device(_padded(rng, Q) if shape['pad'] else Q)
        Sd = None if self_rows is None else K.to_device(self_rows)
        for metric in so.METRICS:
            want = so.similar_rows(X, Q, self_rows, k, metric)
            for segments in shape['segments']:
                for again in (False, True):
                    got = K.similar_rows(Xd, Qd, Sd, k=k, metric=metric, segments=segments, c=c)
                    _check(K, got, want, (shape, metric, segments, again))


@pytest.mark.parametrize('name', list(so.cases()))
def test_every_case_class(K, name):
    case = so.cases()[name]
    X, Q, k = case['X'], case['Q'], case['k']
    Xd, Qd = K.to_device(X), None if Q is None else K.to_device(Q)
    for metric in so.METRICS:
        want = so.similar_rows(X, Q, case['self_rows'], k, metric)
        if name == 'one_hot' and metric == 'cosine':
            assert set(np.unique(want[1])) == {0.0, 1.0}          # ties nearly everywhere: the row index decides
        if name == 'ones_column' and metric == 'cosine':
            assert np.all(want[1] == 1.0)
        for segments in (0, 1, 3):
            _check(K, K.similar_rows(Xd, Qd, k=k, metric=metric, segments=segments), want, (name, metric, segments))


def test_short_lists_hold_minus_one_and_nan(K):
    X = so.memberships(5, 3)
    Xd = K.to_device(X)
    for metric in so.METRICS:
        want = so.similar_rows(X, k=10, metric=metric)
        assert np.all(want[0][:, :4] >= 0) and np.all(want[0][:, 4:] == -1) and np.isnan(want[1][:, 4:]).all()
        for segments in (0, 1, 4):
            _check(K, K.similar_rows(Xd, k=10, metric=metric, segments=segments), want, (metric, segments))
    # two segments of 64 and 6 candidates, k = 64: the second segment's list is short (and the first one's where its
    # row 0 is left out), their union fills every slot
    X = so.memberships(70, 4)
    Q = so.memberships(3, 4, seed=8)
    self_rows = np.array([0, -1, 69], dtype=np.int32)
    for metric in so.METRICS:
        want = so.similar_rows(X, Q, self_rows, 64, metric)
        got = K.similar_rows(K.to_device(X), K.to_device(Q), K.to_device(self_rows), k=64, metric=metric, segments=2)
        _check(K, got, want, metric)
    # the output block's leading dimension: nothing behind column k is touched
    index, score = K.to_device(np.full((5, 13), 7, dtype=np.int32)), K.to_device(np.full((5, 13), -7.0))
    K.similar_rows(Xd, k=10, out=(index, score))
    assert np.all(K.to_host(index)[:, 10:] == 7) and np.all(K.to_host(score)[:, 10:] == -7.0)
    _check(K, (index[:, :10], score[:, :10]), so.similar_rows(so.memberships(5, 3), k=10), 'out')


def test_scores_are_symmetric_bit_for_bit(K):
    n = 40
    X = so.memberships(n, 7)
    for metric in so.METRICS:
        index, score = (np.asarray(K.to_host(t)) for t in K.similar_rows(K.to_device(X), k=n - 1, metric=metric))
        table = np.full((n, n), np.nan)
        table[np.arange(n)[:, None], index] = score
        off = ~np.eye(n, dtype=bool)
        assert not np.isnan(table[off]).any()
        assert table[off].tobytes() == table.T[off].tobytes(), metric


def test_sizes_and_argument_errors(K):
    from graphrole_amd import _lib, nearest_nodes
    lib = _lib.load()
    X = K.to_device(so.memberships(8, 40))
    index, score = K.empty((8, 4), K.torch.int32), K.empty((8, 4))
    ws_bytes = lib.grx_similar_rows_workspace_bytes(8, 8, 32, 4, 0)
    ws = K.empty(ws_bytes, K.torch.uint8)
    stream = K._stream()

    def status(n=8, c=3, x=X, ldx=40, nq=8, q=X, ldq=40, self_rows=None, k=4, metric=0, segments=0, i=index, s=score,
               ld_out=4, w=ws, w_bytes=ws_bytes):
        return lib.grx_similar_rows(n, c, K._ptr(x), ldx, nq, K._ptr(q), ldq, K._ptr(self_rows), k, metric, segments,
                                    K._ptr(i), K._ptr(s), ld_out, K._ptr(w), w_bytes, stream)

    assert status() == 0 and status(c=32) == 0 and status(metric=1, segments=5) == 0
    assert status(c=33) == -4 and b'GRX_MAX_ROLES' in lib.grx_last_error()      # GRX_ERR_UNSUPPORTED
    for bad in (dict(c=0), dict(k=0), dict(k=65, ld_out=65), dict(n=-1), dict(n=1 << 31), dict(nq=-1), dict(ldx=2),
                dict(ldq=2), dict(ld_out=3), dict(metric=2), dict(metric=-1), dict(segments=-1),
                dict(w_bytes=lib.grx_similar_rows_workspace_bytes(8, 8, 3, 4, 0) - 1),
                dict(w_bytes=0), dict(x=None), dict(q=None), dict(i=None), dict(s=None), dict(w=None)):
        assert status(**bad) == -1, bad                                         # GRX_ERR_INVALID
        assert lib.grx_last_error()
    # n = 0 and nq = 0, with and without pointers
    assert status(nq=0) == 0 and status(nq=0, x=None, q=None, i=None, s=None, w=None, w_bytes=0) == 0
    assert status(n=0, x=None, q=None, i=None, s=None, w=None, w_bytes=0) == 0
    assert status(n=0, x=None, w=None, w_bytes=0) == 0                           # queries without candidates: -1 / NaN
    assert np.all(K.to_host(index) == -1) and np.isnan(K.to_host(score)).all()
    assert lib.grx_similar_rows_workspace_bytes(0, 8, 3, 4, 0) == 0
    with pytest.raises(_lib.GrxError, match='GRX_MAX_ROLES'):
        K.similar_rows(X, c=33)
    with pytest.raises(_lib.GrxInvalid, match='GRX_MAX_TOPK'):
        K.similar_rows(X, k=65, c=3)
    with pytest.raises(ValueError, match='metric'):
        K.similar_rows(X, metric='manhattan')
    empty = K.similar_rows(K.empty((0, 3)), k=2)
    assert tuple(empty[0].shape) == (0, 2) and tuple(empty[1].shape) == (0, 2)
    with pytest.raises(ValueError, match='GRX_MAX_TOPK'):
        nearest_nodes(pd.DataFrame(np.ones((70, 2))), k=65)
    # the device still answers after the refusals
    got = K.similar_rows(K.to_device(np.eye(3)[[0, 1, 0]]), k=2)
    assert K.to_host(got[0]).tolist() == [[2, 1], [0, 2], [0, 1]] and K.to_host(got[1]).tolist() == [[1, 0], [0, 0], [1, 0]]


def _fit(G):
    from graphrole_amd import RecursiveFeatureExtractor, RoleExtractor
    features = RecursiveFeatureExtractor(G).extract_features()
    np.random.seed(0)
    role_extractor = RoleExtractor(n_roles=3)
    role_extractor.extract_role_factors(features)
    return features, role_extractor


def _as_frames(table, candidates, index, score):
    labels = np.asarray((table if candidates is None else candidates).index)
    return labels[index].tolist(), score.tobytes()


@pytest.mark.parametrize('name', ['karate', 'ba300'])
def test_end_to_end(name):
    from graphrole_amd import RecursiveFeatureExtractor, nearest_nodes
    G = nx.karate_club_graph() if name == 'karate' else graphs.ba(300, 3, 1)[0]
    features, role_extractor = _fit(G)
    P = role_extractor.node_role_factor
    before = P.copy()
    for metric in so.METRICS:
        neighbors, scores = role_extractor.similar_nodes(k=5, metric=metric)
        want = so.similar_rows(P.to_numpy(), k=5, metric=metric)
        assert list(neighbors.index) == list(P.index) and scores.attrs == {'metric': metric, 'k': 5}
        assert (neighbors.to_numpy().tolist(), scores.to_numpy().tobytes()) == _as_frames(P, None, *want)
        node = 33
        one = role_extractor.similar_nodes(node, k=5, metric=metric)
        assert list(one.index) == neighbors.loc[node].tolist() and one.to_numpy().tobytes() == scores.loc[node].to_numpy().tobytes()
        with_self = role_extractor.similar_nodes([node], k=3, metric=metric, include_self=True)
        want = so.similar_rows(P.to_numpy(), P.loc[[node]].to_numpy(), np.array([-1]), 3, metric)
        assert (with_self[0].to_numpy().tolist(), with_self[1].to_numpy().tobytes()) == _as_frames(P, None, *want)
    # cross-graph: which nodes of graph B resemble node x of graph A
    Gb = graphs.ba(300, 3, 2)[0]
    features_b = RecursiveFeatureExtractor(Gb).replay_features(features.columns)
    Pb = role_extractor.transform(features_b)
    x = 7
    neighbors, scores = nearest_nodes(P, nodes=[x], k=10, candidates=Pb)
    want = so.similar_rows(Pb.to_numpy(), P.loc[[x]].to_numpy(), np.array([-1]), 10)
    assert (neighbors.to_numpy().tolist(), scores.to_numpy().tobytes()) == _as_frames(P, Pb, *want)
    assert role_extractor.node_role_factor.equals(before)
