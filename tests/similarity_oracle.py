"""
The arithmetic and the order of grx_similar_rows (csrc/grx_similarity.hip) restated in numpy, a high-precision authority
with a derived error bound, and the case builders the CPU and the GPU tests share.

The restatement.  numpy rounds every elementwise product, difference, quotient and sum on its own, which is the kernel's
contract (no fused multiply-add), and ``sqrt`` and ``/`` are correctly rounded on both sides; the loop over the columns
runs j = 0 .. c - 1 from +0.0 as the kernel's does.  So ``similar_rows`` gives the kernel's bits, index and score.
  cosine:     norm = sqrt(sum_j x_j * x_j), xn = x / norm (0 where norm is 0), score = sum_j qn_j * xn_j, key = -score
  Euclidean:  key = d2 = sum_j (q_j - x_j) * (q_j - x_j), score = sqrt(d2)
The selection is np.lexsort on (row index, key): key ascending, then the smaller row; the row `self_rows[q]` is left out
and slots without a candidate hold -1 / NaN.

The bound (u = 2^-53, first order with one unit of slack for the second; inputs far from underflow and overflow, which
the builders keep).
  cosine.  s = sum x_j^2 has non-negative terms, so its relative error is at most c u (one rounding per product, c - 1
  additions, none of them cancelling); sqrt halves it and rounds once: norm is within (c / 2 + 1) u; the division rounds
  once more: every xn_j is within (c / 2 + 2) u of x_j / ||x||, and so is qn_j.  The product of the two computed values is
  within (c + 4) u of the true one, its rounding adds u and the c - 1 additions at most (c - 1) u of the sum of the
  absolute terms: |score - exact| <= (2 c + 4) u sum_j |qn_j xn_j|.  COS_SLACK more units cover the second order and the
  authority's own rounding (80-bit or wider long double: 2^-11 of the above).
  Euclidean.  A difference rounds once (u), its square doubles that and rounds again (3 u), the additions of
  non-negative terms add at most (c - 1) u: d2 is within (c + 2) u, its square root within (c / 2 + 1) u + u:
  |score - exact| <= (c / 2 + 2) u exact, plus EUC_SLACK.
"""
import numpy as np

U = 2.0 ** -53
COS_SLACK = 2
EUC_SLACK = 1
METRICS = ('cosine', 'euclidean')


# --------------------------------------------------------------------------------------------- the restatement
def normalise(X):
    X = np.asarray(X, dtype=np.float64)
    s = np.zeros(X.shape[0])
    for j in range(X.shape[1]):
        s = s + X[:, j] * X[:, j]
    norm = np.sqrt(s)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where((norm > 0.0)[:, None], X / norm[:, None], 0.0)


def keys(Q, X, metric):
    """[nq, n] keys, smaller is nearer: -score for the cosine, the squared distance for the Euclidean metric."""
    Q, X = np.asarray(Q, dtype=np.float64), np.asarray(X, dtype=np.float64)
    acc = np.zeros((Q.shape[0], X.shape[0]))
    if metric == 'cosine':
        Qn, Xn = normalise(Q), normalise(X)
        for j in range(X.shape[1]):
            acc = acc + Qn[:, j, None] * Xn[None, :, j]
        return -acc
    for j in range(X.shape[1]):
        d = Q[:, j, None] - X[None, :, j]
        acc = acc + d * d
    return acc


def score_of(key, metric):
    return -key if metric == 'cosine' else np.sqrt(key)


def select(key, self_rows, k):
    """(index int32[nq, k], key fp64[nq, k]) of the first k candidates per row of `key` in the order (key, row), the
    row self_rows[q] left out (None or -1: nothing); -1 / NaN where the candidates run out."""
    nq, n = key.shape
    index = np.full((nq, k), -1, dtype=np.int32)
    best = np.full((nq, k), np.nan)
    rows = np.arange(n)
    for q in range(nq):
        order = np.lexsort((rows, key[q]))
        if self_rows is not None and self_rows[q] >= 0:
            order = order[order != self_rows[q]]
        order = order[:k]
        index[q, :len(order)] = order
        best[q, :len(order)] = key[q, order]
    return index, best


def similar_rows(X, Q=None, self_rows=None, k=10, metric='cosine'):
    """The kernel's result bit for bit.  Q=None: the rows of X query themselves and leave themselves out."""
    X = np.asarray(X, dtype=np.float64)
    if Q is None:
        Q = X
        if self_rows is None:
            self_rows = np.arange(len(X))
    index, best = select(keys(Q, X, metric), self_rows, k)
    score = np.full(best.shape, np.nan)                         # the one NaN the kernel writes: 0x7ff8000000000000
    score[index >= 0] = score_of(best[index >= 0], metric)
    return index, score


# ------------------------------------------------------------------------------------------------ the authority
def authority(Q, X, metric):
    """(exact [nq, n] scores rounded to fp64 from long double, bound [nq, n] on |kernel score - exact|)."""
    L = np.longdouble
    assert np.finfo(L).eps <= 2.0 ** -63, 'the authority needs a long double wider than fp64'
    Q, X = np.asarray(Q, dtype=np.float64).astype(L), np.asarray(X, dtype=np.float64).astype(L)
    c = X.shape[1]
    if metric == 'cosine':
        def unit(A):
            norm = np.sqrt((A * A).sum(axis=1))
            return np.where((norm > 0)[:, None], A / np.where(norm > 0, norm, 1)[:, None], 0)
        Qn, Xn = unit(Q), unit(X)
        exact = (Qn[:, None, :] * Xn[None, :, :]).sum(axis=2)
        mass = np.abs(Qn[:, None, :] * Xn[None, :, :]).sum(axis=2)
        return exact.astype(np.float64), ((2 * c + 4 + COS_SLACK) * U * mass).astype(np.float64)
    d = Q[:, None, :] - X[None, :, :]
    exact = np.sqrt((d * d).sum(axis=2))
    return exact.astype(np.float64), ((c / 2 + 2 + EUC_SLACK) * U * exact).astype(np.float64)


def nearer(metric):
    """+1 where a larger score is nearer, -1 where a smaller one is."""
    return 1.0 if metric == 'cosine' else -1.0


# --------------------------------------------------------------------------------------------------- the cases
def memberships(n, c, seed=0):
    """Non-negative rows like a node-role factor: gamma draws, a few exact zeros."""
    rng = np.random.default_rng(1000 * c + n + seed)
    P = rng.gamma(0.7, 1.0, size=(n, c))
    P[rng.random((n, c)) < 0.1] = 0.0
    P[P.sum(axis=1) == 0, 0] = 1.0
    return P


def one_hot(n, c, seed=0):
    return np.eye(c)[np.random.default_rng(seed).integers(0, c, n)]


def arc(n, rising):
    """(X, Q): n unit vectors at angles between 1.5 and 0.05 from the single query (1, 0).  rising: every candidate is
    nearer than all before it -- each one has to be inserted; otherwise the nearest come first and nothing is inserted
    after the first k.  The same order under both metrics."""
    theta = np.linspace(1.5, 0.05, n) if rising else np.linspace(0.05, 1.5, n)
    return np.stack([np.cos(theta), np.sin(theta)], axis=1), np.array([[1.0, 0.0]])


def cases():
    """name -> dict(X, Q (None: self-query), self_rows (None: the default of the call), k)."""
    dup = memberships(40, 5, seed=3)
    dup = np.repeat(dup, 5, axis=0)[np.random.default_rng(4).permutation(200)]
    zero = memberships(150, 6, seed=5)
    zero[::7] = 0.0
    rising, q = arc(300, True)
    falling, _ = arc(300, False)
    return {
        'random': dict(X=memberships(150, 6), Q=None, self_rows=None, k=10),
        'random_external': dict(X=memberships(140, 17), Q=memberships(9, 17, seed=1), self_rows=None, k=10),
        'one_hot': dict(X=one_hot(200, 30), Q=None, self_rows=None, k=10),     # ~7 nodes per role: ones, then zeros
        'duplicates': dict(X=dup, Q=None, self_rows=None, k=7),
        'zero_rows': dict(X=zero, Q=None, self_rows=None, k=10),
        'ones_column': dict(X=np.ones((130, 1)), Q=None, self_rows=None, k=10),
        'rising': dict(X=rising, Q=q, self_rows=None, k=10),
        'falling': dict(X=falling, Q=q, self_rows=None, k=10),
    }
