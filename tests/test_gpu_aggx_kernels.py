"""
Kernel-level parity of csrc/grx_aggx.hip (median selection, wrapping int64 aggregations, neighbour counts, the two
conversions) and of the column movers and small reductions (grx_permute_columns, grx_gather_columns, grx_transpose,
grx_add_columns, grx_min_value) on the MI355X against the numpy reference of tests/aggx_oracle.py.

Every kernel here selects, moves or does integer arithmetic, and the even-row median is the single fp64 operation
(a + b) / 2: every comparison is equality (bit patterns through .view(np.int64) where a column is moved,
assert_array_equal where inf - inf gives NaN on both sides).  A signed zero in a median compares equal and is not
otherwise distinguished.  tests/test_aggx_oracle_cpu.py pins the reference to pandas and to tests/fake_kernels.py and
checks that the cases reach the branches they are there for.
"""
import numpy as np
import pytest

from tests import aggx_oracle as ao

pytestmark = pytest.mark.gpu

GRAPH_NAMES = list(ao.GRAPHS)


@pytest.fixture(scope='module')
def K():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from graphrole_amd import kernels
    return kernels


_CSR = {}


def _csr(K, name):
    if name not in _CSR:
        row_ptr, adj = ao.graph(name)
        _CSR[name] = K.DeviceCSR(row_ptr, ao.sorted_col(row_ptr, adj), agg_col=adj)
    return _CSR[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _dev_i64(K, x):
    """int64 values -> the fp64 tensor that carries their bits."""
    return K.to_device(np.ascontiguousarray(x, dtype=np.int64).view(np.float64))


def _host_i64(K, t):
    return _bits(K.to_host(t))


def _pack(K, X, f):
    """pack_rows of the first f columns of X (float64 or int64 bits) -> (rows, ldr); the packed block holds the
    input bit for bit."""
    n = X.shape[0]
    cols = [K.to_device(np.ascontiguousarray(_bits(X[:, c])).view(np.float64)) for c in range(f)]
    rows, ldr = K.pack_rows(cols, n)
    assert ldr >= max(f, 1) and tuple(rows.shape) == (n, ldr)
    if f:
        assert np.array_equal(_bits(K.to_host(rows))[:, :f], _bits(X[:, :f]))
    return rows, ldr


# ---- grx_aggregate_median -------------------------------------------------------------------------------------------

def test_pack_rows_layouts_of_the_median_cases(K):
    ldrs = {f: int(K._lib.load().grx_aggregate_ldr(f)) for f in ao.MEDIAN_F}
    assert ldrs == {1: 2, 3: 4, 8: 8, 9: 16, 17: 32}, ldrs


@pytest.mark.parametrize('f', ao.MEDIAN_F)
@pytest.mark.parametrize('name', GRAPH_NAMES)
def test_median_equals_numpy(K, name, f):
    csr, X = _csr(K, name), ao.median_values(name)
    want = ao.median_expected(name)[:f]
    rows, ldr = _pack(K, X, f)
    full = K.to_host(K.aggregate_median(csr, rows, f, ldr))
    assert full.shape == (f, csr.n) and full.dtype == np.float64
    np.testing.assert_array_equal(full, want)
    # a row range whose adjacency slice starts at e_begin > 0: the same bits as the full run on those rows
    rb, re = ao.ROW_RANGES[name]
    part = K.to_host(K.aggregate_median(csr, rows, f, ldr, rb, re))
    np.testing.assert_array_equal(part[:, rb:re], want[:, rb:re])
    assert np.array_equal(_bits(part[:, rb:re]), _bits(full[:, rb:re]))
    # one row, the last row, everything from rb on
    for b, e in ((rb, rb + 1), (csr.n - 1, csr.n), (rb, csr.n)):
        got = K.to_host(K.aggregate_median(csr, rows, f, ldr, b, e))
        assert np.array_equal(_bits(got[:, b:e]), _bits(full[:, b:e])), (b, e)


@pytest.mark.parametrize('name', GRAPH_NAMES)
def test_median_empty_range_and_no_columns(K, name):
    csr, X = _csr(K, name), ao.median_values(name)
    rows, ldr = _pack(K, X, 3)
    rb = ao.ROW_RANGES[name][0]
    for b in (0, rb, csr.n):
        assert tuple(K.aggregate_median(csr, rows, 3, ldr, b, b).shape) == (3, csr.n)
    assert tuple(K.aggregate_median(csr, rows, 0, ldr).shape) == (0, csr.n)
    rows0, ldr0 = _pack(K, X, 0)
    assert tuple(K.aggregate_median(csr, rows0, 0, ldr0).shape) == (0, csr.n)


# ---- grx_aggregate_i64 ----------------------------------------------------------------------------------------------

AGGS = ('sum', 'prod', 'min', 'max')


@pytest.mark.parametrize('f', ao.I64_F)
@pytest.mark.parametrize('name', GRAPH_NAMES)
def test_int64_aggregations_equal_numpy(K, name, f):
    csr, X = _csr(K, name), ao.i64_values(name)
    want = {a: w[:f] for a, w in ao.i64_expected(name).items()}
    rows, ldr = _pack(K, X, f)
    got = K.aggregate_i64(csr, rows, f, ldr)
    assert set(got) == set(AGGS)
    for a in AGGS:
        assert np.array_equal(_host_i64(K, got[a]), want[a]), (a, np.argwhere(_host_i64(K, got[a]) != want[a])[:5])
    # subsets of `want`: each alone, and pairs
    for subset in (('sum',), ('prod',), ('min',), ('max',), ('sum', 'max'), ('prod', 'min'), ('min', 'max', 'sum')):
        got = K.aggregate_i64(csr, rows, f, ldr, want=subset)
        assert set(got) == set(subset)
        for a in subset:
            assert np.array_equal(_host_i64(K, got[a]), want[a]), (subset, a)
    rb, re = ao.ROW_RANGES[name]
    for b, e in ((rb, re), (rb, rb + 1), (csr.n - 1, csr.n), (0, rb)):
        got = K.aggregate_i64(csr, rows, f, ldr, b, e)
        for a in AGGS:
            assert np.array_equal(_host_i64(K, got[a])[:, b:e], want[a][:, b:e]), (a, b, e)
    assert set(K.aggregate_i64(csr, rows, f, ldr, rb, rb)) == set(AGGS)      # an empty range launches nothing


def test_int64_empty_rows_and_no_columns(K):
    csr, X = _csr(K, 'classes'), ao.i64_values('classes')
    empty = np.flatnonzero(np.diff(ao.graph('classes')[0]) == 0)
    rows, ldr = _pack(K, X, 5)
    got = {a: _host_i64(K, t) for a, t in K.aggregate_i64(csr, rows, 5, ldr).items()}
    assert len(empty) >= 8
    assert not got['sum'][:, empty].any() and not got['min'][:, empty].any() and not got['max'][:, empty].any()
    assert np.all(got['prod'][:, empty] == 1)
    none = K.aggregate_i64(csr, rows, 0, ldr)
    assert all(tuple(t.shape) == (0, csr.n) for t in none.values())


# ---- grx_aggregate_count --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('as_i64', [False, True])
@pytest.mark.parametrize('f', [1, 3])
@pytest.mark.parametrize('name', GRAPH_NAMES)
def test_count_equals_row_lengths(K, name, f, as_i64):
    csr = _csr(K, name)
    row_ptr = ao.graph(name)[0]
    n = csr.n

    def host(t):
        return _host_i64(K, t) if as_i64 else K.to_host(t)

    assert np.array_equal(host(K.aggregate_count(csr, f, as_i64=as_i64)), ao.count(row_ptr, f, as_i64=as_i64))
    rb, re = ao.ROW_RANGES[name]
    for b, e in ((rb, re), (rb, rb + 1), (n - 1, n)):
        got = host(K.aggregate_count(csr, f, b, e, as_i64=as_i64))
        assert np.array_equal(got[:, b:e], ao.count(row_ptr, f, b, e, as_i64)[:, b:e]), (b, e)


@pytest.mark.parametrize('as_i64', [False, True])
def test_count_leaves_rows_outside_the_range_alone(K, as_i64):
    """Rows outside [row_begin, row_end) are unspecified in the wrapper's result (it allocates without clearing):
    the kernel neither writes them (a block pre-filled with a marker keeps it) nor reads their row pointers (poisoned
    outside the range, the rows inside still come out right)."""
    row_ptr = ao.graph('classes')[0]
    n = len(row_ptr) - 1
    rb, re = ao.ROW_RANGES['classes']
    poisoned = row_ptr.copy()
    poisoned[:rb] = -2 ** 40
    poisoned[re + 1:] = 2 ** 40
    d_row_ptr = K.to_device(poisoned)
    marker = np.int64(0x7FF0DEAD0000BEEF)
    out = _dev_i64(K, np.full((3, n), marker))
    K._lib.call('grx_aggregate_count', K._ptr(d_row_ptr), 3, rb, re, int(as_i64), K._ptr(out), n, K._stream())
    got = _host_i64(K, out)
    assert np.all(got[:, :rb] == marker) and np.all(got[:, re:] == marker)
    inside = got[:, rb:re] if as_i64 else got.view(np.float64)[:, rb:re]
    assert np.array_equal(inside, ao.count(row_ptr, 3, rb, re, as_i64)[:, rb:re])


# ---- grx_convert_i64_to_f64 / grx_convert_f64_to_i64 ----------------------------------------------------------------

@pytest.mark.parametrize('n', ao.LENGTHS)
def test_conversions_equal_astype(K, n):
    x = ao.convert_i64_input(n)
    got = K.to_host(K.convert_i64_to_f64(_dev_i64(K, x)))
    assert got.dtype == np.float64 and np.array_equal(_bits(got), _bits(ao.i64_to_f64(x)))
    y = ao.convert_f64_input(n)
    got = _host_i64(K, K.convert_f64_to_i64(K.to_device(y)))
    assert np.array_equal(got, ao.f64_to_i64(y))


@pytest.mark.parametrize('n', ao.LENGTHS)
def test_conversion_round_trip_below_2_53(K, n):
    x = np.random.default_rng(n).integers(-2 ** 53 + 1, 2 ** 53, size=n, dtype=np.int64)
    x[0] = [2 ** 53 - 1, -2 ** 53 + 1][n % 2]
    back = _host_i64(K, K.convert_f64_to_i64(K.convert_i64_to_f64(_dev_i64(K, x))))
    assert np.array_equal(back, x)


# ---- grx_permute_columns / grx_gather_columns -----------------------------------------------------------------------

MOVER_F = (1, 127, 128, 129, 300)                              # the pointer table holds 128 columns per launch
MOVER_N = (1, 255, 257, 100003)


def _mover_columns(K, F, m, seed):
    """(int64 [F, m] bit patterns, their device columns): every column an allocation of its own."""
    B = ao.bit_pattern_columns(F, m, seed)
    return B, [_dev_i64(K, B[c]) for c in range(F)]


@pytest.mark.parametrize('n', MOVER_N)
@pytest.mark.parametrize('F', MOVER_F)
def test_permute_columns_moves_bits(K, F, n):
    """out[c][i] = cols[c][index[i]] for an index of n entries with repeats over columns of m rows, m > n (an index
    shorter than the column) and m < n (longer); the patterns are subnormals, NaNs with payloads and signalling NaNs
    when read as fp64."""
    rng = np.random.default_rng(1000 * F + n)
    for m in (2 * n + 3, max(n // 2, 1)):
        B, cols = _mover_columns(K, F, m, F + n + m)
        index = rng.integers(0, m, size=n).astype(np.int32)
        index[-1] = m - 1
        index[0] = index[n // 2]                               # a repeat also when n <= m
        out = K.permute_columns(cols, K.to_device(index), n)
        assert tuple(out.shape) == (F, n)
        got = _bits(K.to_host(out.contiguous()))
        assert np.array_equal(got, B[:, index]), (F, n, m, np.argwhere(got != B[:, index])[:5])
    # the identity and the reversal
    B, cols = _mover_columns(K, F, n, F + n)
    for index in (np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32)[::-1].copy()):
        got = _bits(K.to_host(K.permute_columns(cols, K.to_device(index), n).contiguous()))
        assert np.array_equal(got, B[:, index])


@pytest.mark.parametrize('n', MOVER_N)
@pytest.mark.parametrize('F', MOVER_F)
def test_gather_columns_moves_bits(K, F, n):
    """out[c][:n] = cols[c][:n] for columns of exactly n rows and of more than n rows."""
    for m in (n, n + 7):
        B, cols = _mover_columns(K, F, m, 7 * F + n + m)
        out = K.gather_columns(cols, n)
        assert tuple(out.shape) == (F, n)
        got = _bits(K.to_host(out))
        assert np.array_equal(got, B[:, :n]), (F, n, m, np.argwhere(got != B[:, :n])[:5])


def test_movers_with_no_columns(K):
    index = K.to_device(np.zeros(5, dtype=np.int32))
    assert tuple(K.permute_columns([], index, 5).shape) == (0, 5)
    assert tuple(K.gather_columns([], 5).shape) == (0, 5)


# ---- grx_add_columns ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 255, 256, 257, 100003, 1000003])
def test_add_columns_is_the_ieee_sum(K, n):
    rng = np.random.default_rng(n)
    a = rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, size=n)
    b = rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, size=n)
    special = [(np.inf, -np.inf), (np.inf, 1.0), (-np.inf, -np.inf), (1.5, -1.5), (-0.0, 0.0), (-0.0, -0.0),
               (1e308, 1e308), (2.0 ** -1074, 2.0 ** -1074), (1.0, 2.0 ** -53), (1.0 + 2.0 ** -52, 2.0 ** -53)]
    at = rng.choice(n, size=min(n, 4 * len(special)), replace=False)
    for i, p in enumerate(at):
        a[p], b[p] = special[i % len(special)]
    cancel = rng.random(n) < 0.1                                # opposite signs, equal magnitudes
    cancel[at] = False
    b[cancel] = -a[cancel]
    got = K.to_host(K.add_columns(K.to_device(a), K.to_device(b)))
    with np.errstate(invalid='ignore', over='ignore'):
        want = a + b
    np.testing.assert_array_equal(got, want)
    finite = ~np.isnan(want)
    assert np.array_equal(_bits(got[finite]), _bits(want[finite]))            # the sign of a zero sum included


# ---- grx_min_value --------------------------------------------------------------------------------------------------

def _min_block(F, n, seed):
    """[F, n + 5] block: real entries in the first n columns (values >= -1000), padding below every one of them."""
    rng = np.random.default_rng(seed)
    X = np.full((F, n + 5), -1e300)
    X[:, :n] = rng.standard_normal((F, n)) * 300.0
    np.clip(X[:, :n], -1000.0, None, out=X[:, :n])
    return X, rng


@pytest.mark.parametrize('n', [1, 2047, 2049, 1000003])
@pytest.mark.parametrize('F', [1, 3, 4, 5, 37])                # the column loop of a workgroup starts at F > 4
def test_min_value_equals_numpy(K, F, n):
    X, rng = _min_block(F, n, 100 * F + n % 97)
    assert X[:, n:].max() < X[:, :n].min()
    d = K.to_device(X)
    assert K.min_value(d, n) == X[:, :n].min()
    # the minimum at every corner of the valid block and at a random place
    for r, c in ((0, 0), (F - 1, n - 1), (F - 1, 0), (0, n - 1), (int(rng.integers(F)), int(rng.integers(n)))):
        Y = X.copy()
        Y[r, c] = -2000.0
        assert K.min_value(K.to_device(Y), n) == -2000.0, (r, c)
    # a single NaN anywhere gives NaN, also next to -inf; NaN in the padding is not seen
    for r, c in ((0, 0), (F - 1, n - 1), (int(rng.integers(F)), int(rng.integers(n)))):
        Y = X.copy()
        Y[(r + 1) % F, (c + 1) % n] = -np.inf
        Y[r, c] = np.nan
        assert np.isnan(K.min_value(K.to_device(Y), n)), (r, c)
    Y = X.copy()
    Y[:, n:] = np.nan
    assert K.min_value(K.to_device(Y), n) == X[:, :n].min()
    Y[F - 1, n - 1] = -np.inf
    assert K.min_value(K.to_device(Y), n) == -np.inf
    # a contiguous block (ld == n) and zeros of both signs
    Z = np.ascontiguousarray(X[:, :n])
    assert K.min_value(K.to_device(Z), n) == Z.min()
    Z = np.abs(Z)
    Z[F - 1, n - 1] = -0.0
    Z[0, 0] = 0.0
    assert K.min_value(K.to_device(Z), n) == 0.0 == Z.min()


# ---- grx_transpose --------------------------------------------------------------------------------------------------

def _transpose_source(rows, ld, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(ao.I64_MIN, ao.I64_MAX, size=(rows, ld), dtype=np.int64)


@pytest.mark.parametrize('shape', [(1, 1), (31, 33), (32, 32), (33, 31), (70001, 7), (5, 70001), (64, 96), (1, 257),
                                   (257, 1)])
def test_transpose_equals_numpy(K, shape):
    rows, cols = shape
    for ld in (cols, cols + 3):                                # a source with ld > cols: the padding is not moved
        B = _transpose_source(rows, ld, rows + cols + ld)
        out = K.transpose(_dev_i64(K, B), rows, cols)
        assert tuple(out.shape) == (cols, rows)
        got = _host_i64(K, out)
        assert np.array_equal(got, B[:, :cols].T), (shape, ld, np.argwhere(got != B[:, :cols].T)[:5])


def test_transpose_tall(K):
    """rows = 32 * 65536 + 33, cols = 3 (roles/factor.py transposes n x F and n x r blocks with rows = n): 65 538
    tiles of 32 rows in grid.y.  Observed on the MI355X: the launch with grid.y = 65 538 is accepted and the result
    equals X.T exactly, so the kernel keeps its layout; the guard of grx_transpose that could never fire now refuses
    only a tile count beyond a 32-bit grid dimension (tests/test_aggx_oracle_cpu.py).  Runs once, last."""
    rows, cols = 32 * 65536 + 33, 3
    B = _transpose_source(rows, cols, 5)
    got = _host_i64(K, K.transpose(_dev_i64(K, B), rows, cols))
    assert np.array_equal(got, B.T), np.argwhere(got != B.T)[:5]
