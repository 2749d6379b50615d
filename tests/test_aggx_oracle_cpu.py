"""
-m "not gpu": the numpy reference of tests/aggx_oracle.py against pandas (what the reference project hands its
neighbour frames to) and against tests/fake_kernels.py (what the CPU suite runs the host logic on), so the CPU suite
and tests/test_gpu_aggx_kernels.py are pinned to the same answers; and, for every case of the GPU tests, the
conditions that make it reach what it is there for.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from tests import aggx_oracle as ao
from tests import fake_kernels as FK

GRAPH_NAMES = list(ao.GRAPHS)


def _sample_rows(row_ptr, seed, k=40):
    """The class rows / the longest rows, empty rows and a random sample."""
    deg = np.diff(row_ptr)
    rng = np.random.default_rng(seed)
    rows = set(np.argsort(deg)[-20:].tolist()) | set(np.flatnonzero(deg == 0)[:3].tolist())
    rows |= set(rng.choice(len(deg), size=min(k, len(deg)), replace=False).tolist())
    return sorted(rows)


@pytest.mark.parametrize('name', GRAPH_NAMES)
def test_graphs_are_well_formed(name):
    row_ptr, adj = ao.graph(name)
    n = len(row_ptr) - 1
    assert row_ptr[0] == 0 and row_ptr[-1] == len(adj) and np.all(np.diff(row_ptr) >= 0)
    assert adj.dtype == np.int32 and adj.min() >= 0 and adj.max() < n
    col = ao.sorted_col(row_ptr, adj)
    for v in _sample_rows(row_ptr, 1):
        a, b = row_ptr[v], row_ptr[v + 1]
        assert np.array_equal(col[a:b], np.sort(adj[a:b])) and len(np.unique(adj[a:b])) == b - a
    rb, re = ao.ROW_RANGES[name]
    assert 0 < rb < re < n and row_ptr[rb] > 0 and row_ptr[re] > row_ptr[rb]


def test_degree_class_graph_has_every_boundary():
    row_ptr, _ = ao.graph('classes')
    deg = np.diff(row_ptr)
    assert tuple(deg[40:40 + len(ao.DEGREE_CLASSES)]) == ao.DEGREE_CLASSES
    for d in (0, 1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 1000, 1001):
        assert (deg == d).any(), d
    assert np.all(deg[-7:] == 0) and deg[:40].sum() > 0       # trailing empty rows; the classes start at an offset
    rb, re = ao.ROW_RANGES['classes']
    assert {64, 65} <= set(deg[rb:re].tolist())               # the row range cuts through the rank / radix boundary


def test_star_and_powerlaw_shapes():
    row_ptr, adj = ao.graph('star')
    deg = np.diff(row_ptr)
    assert deg[0] == 70001 and np.all(deg[1:] == 1) and np.all(adj[70001:] == 0)
    assert sorted(adj[:70001].tolist()) == list(range(1, 70002)) and not np.all(np.diff(adj[:70001]) > 0)
    deg = np.diff(ao.graph('powerlaw')[0])
    assert deg.max() > 64 and (deg <= 64).any() and (deg % 2 == 0).any() and (deg % 2 == 1).any()


@pytest.mark.parametrize('name', GRAPH_NAMES)
def test_median_equals_pandas_and_fake_kernels(name):
    row_ptr, adj = ao.graph(name)
    X = ao.median_values(name)
    want = ao.median_expected(name)
    assert want.shape == (X.shape[1], len(row_ptr) - 1) and X.shape[1] == max(ao.MEDIAN_F)
    with np.errstate(invalid='ignore'):
        for v in _sample_rows(row_ptr, 2):
            nb = adj[row_ptr[v]:row_ptr[v + 1]]
            got = pd.DataFrame(X[nb]).median().fillna(0).to_numpy()
            np.testing.assert_array_equal(got, want[:, v], err_msg=str(v))
            if len(nb):
                np.testing.assert_array_equal(np.median(X[nb], axis=0), want[:, v])
        csr = FK.DeviceCSR(row_ptr, ao.sorted_col(row_ptr, adj), agg_col=adj)
        fake = FK.aggregate_median(csr, torch.from_numpy(X.copy()), X.shape[1], X.shape[1]).numpy()
        np.testing.assert_array_equal(fake, want)
        rb, re = ao.ROW_RANGES[name]
        part = FK.aggregate_median(csr, torch.from_numpy(X.copy()), 3, X.shape[1], rb, re).numpy()
        np.testing.assert_array_equal(part, ao.median(row_ptr, adj, X[:, :3], rb, re))
        np.testing.assert_array_equal(part[:, rb:re], want[:3, rb:re])


@pytest.mark.parametrize('name', GRAPH_NAMES)
def test_int64_aggregations_equal_pandas_and_fake_kernels(name):
    row_ptr, adj = ao.graph(name)
    X = ao.i64_values(name)
    want = ao.i64_expected(name)
    assert X.dtype == np.int64 and X.shape[1] == max(ao.I64_F)
    for v in _sample_rows(row_ptr, 3):
        nb = adj[row_ptr[v]:row_ptr[v + 1]]
        frame = pd.DataFrame(X[nb])
        assert all(str(t) == 'int64' for t in frame.dtypes)
        for agg in ('sum', 'prod', 'min', 'max'):
            got = getattr(frame, agg)().fillna(0).to_numpy().astype(np.int64)
            assert np.array_equal(got, want[agg][:, v]), (agg, v)
        assert np.array_equal(frame.count().to_numpy(), ao.count(row_ptr, X.shape[1], as_i64=True)[:, v])
    csr = FK.DeviceCSR(row_ptr, ao.sorted_col(row_ptr, adj), agg_col=adj)
    rows = torch.from_numpy(X.view(np.float64).copy())
    fake = FK.aggregate_i64(csr, rows, X.shape[1], X.shape[1])
    for agg in ('sum', 'prod', 'min', 'max'):
        assert np.array_equal(fake[agg].numpy().view(np.int64), want[agg]), agg
    rb, re = ao.ROW_RANGES[name]
    part = FK.aggregate_i64(csr, rows, 4, X.shape[1], rb, re, want=('prod', 'min'))
    ref = ao.aggregate_i64(row_ptr, adj, X[:, :4], rb, re)
    assert set(part) == {'prod', 'min'}
    for agg in part:
        assert np.array_equal(part[agg].numpy().view(np.int64)[:, rb:re], ref[agg][:, rb:re]), agg
        assert np.array_equal(ref[agg][:, rb:re], want[agg][:4, rb:re])
    for as_i64 in (False, True):
        for f in (1, 3):
            got = FK.aggregate_count(csr, f, rb, re, as_i64=as_i64).numpy()
            got = got.view(np.int64) if as_i64 else got
            assert np.array_equal(got, ao.count(row_ptr, f, rb, re, as_i64))


def test_empty_rows_give_the_fillna_values():
    row_ptr, adj = ao.graph('classes')
    empty = np.flatnonzero(np.diff(row_ptr) == 0)
    assert len(empty) >= 8
    assert not ao.median_expected('classes')[:, empty].any()
    want = ao.i64_expected('classes')
    assert not want['sum'][:, empty].any() and not want['min'][:, empty].any() and not want['max'][:, empty].any()
    assert np.all(want['prod'][:, empty] == 1)
    assert not ao.count(row_ptr, 2)[:, empty].any()


@pytest.mark.parametrize('name', ['classes', 'powerlaw'])
def test_median_columns_take_the_sides_of_the_even_row_decision(name):
    """`n_le < k + 2` of med_select_kernel: a column of distinct values can only need the next key, a constant one
    can only keep the lower middle's; every other column makes even rows of this graph do both."""
    row_ptr, adj = ao.graph(name)
    X = ao.median_values(name)
    for j in range(X.shape[1]):
        column = ao.MEDIAN_COLUMNS[j % len(ao.MEDIAN_COLUMNS)]
        same, nxt = ao.even_row_sides(row_ptr, adj, X[:, j])
        print(f'{name} column {j} ({column.name}): {same} even rows keep the key, {nxt} take the next')
        if column.sides == 'both':
            assert same > 0 and nxt > 0, (name, j, column.name, same, nxt)
        elif column.sides == 'next':
            assert same == 0 and nxt > 0, (name, j, column.name, same, nxt)
        else:
            d2 = int(((np.diff(row_ptr) % 2 == 0) & (np.diff(row_ptr) > 0)).sum())
            assert same == d2 > 0 and nxt == 0, (name, j, column.name, same, nxt)
    for f in ao.MEDIAN_F[1:]:                                  # every case with more than the first column does both
        sides = [ao.even_row_sides(row_ptr, adj, X[:, j]) for j in range(f)]
        assert sum(s for s, _ in sides) > 0 and sum(t for _, t in sides) > 0


def test_the_star_has_no_even_row():
    """Its centre has 70 001 neighbours and every leaf one: the star is there for the length of the radix passes and
    the 32-bit histogram counts, the even-row decision belongs to the other two graphs."""
    assert np.all(np.diff(ao.graph('star')[0]) % 2 == 1)


def test_the_two_valued_column_splits_rows_exactly_in_half():
    row_ptr, adj = ao.graph('classes')
    x = ao.median_values('classes')[:, 4]
    assert abs(int((x == -2.5).sum()) - int((x == 7.25).sum())) <= 1 and set(x.tolist()) == {-2.5, 7.25}
    med = ao.median_expected('classes')[4]
    even = (np.diff(row_ptr) % 2 == 0) & (np.diff(row_ptr) > 0)
    assert {-2.5, 2.375, 7.25} <= set(med[even].tolist())     # more low, exactly half, more high


def test_median_columns_hold_what_they_claim():
    X = ao.median_values('classes')
    bits = X.view(np.int64)
    assert len(np.unique(bits[:, 2] >> 8)) == 1 and len(np.unique(bits[:, 2] & 0xFF)) > 200
    assert len(np.unique(bits[:, 3] & ~(0xFF << 24))) == 1 and len(np.unique((bits[:, 3] >> 24) & 0xFF)) > 200
    zeros = X[:, 5] == 0
    assert np.signbit(X[zeros, 5]).any() and not np.signbit(X[zeros, 5]).all() and (X[:, 5] < 0).any()
    assert np.abs(X[:, 6]).min() < 1e-290 and np.abs(X[:, 6]).max() > 1e290 and (X[:, 6] < 0).any()
    assert len(np.unique(X[:, 7])) == 1
    assert np.isposinf(X[:, 8]).any() and np.isneginf(X[:, 8]).any() and not np.isnan(X).any()
    med = ao.median_expected('classes')
    assert np.isnan(med[8]).any() or np.isinf(med[8]).any()   # the infinities reach the middle of some row


@pytest.mark.parametrize('name', GRAPH_NAMES)
def test_int64_sum_and_product_leave_the_range_in_exact_arithmetic(name):
    row_ptr, adj = ao.graph(name)
    X = ao.i64_values(name)
    want = ao.i64_expected(name)
    for j, which in ((ao.I64_SUM_WRAP_COLUMN, 'sum'), (ao.I64_PROD_WRAP_COLUMN, 'prod'),
                     (ao.I64_PROD_ZERO_COLUMN, 'prod')):
        sums, prods = ao.exact_row_reductions(row_ptr, adj, X[:, j])
        exact = sums if which == 'sum' else prods
        outside = [v for v, t in enumerate(exact) if not ao.I64_MIN <= t <= ao.I64_MAX]
        assert outside, (name, j, which)
        wrapped = np.array([((t + 2 ** 63) % 2 ** 64) - 2 ** 63 for t in exact], dtype=np.int64)
        assert np.array_equal(wrapped, want[which][j]), (name, j, which)
        if j == ao.I64_PROD_WRAP_COLUMN:
            assert np.all(want['prod'][j] % 2 != 0)           # odd factors: never 0
        if j == ao.I64_PROD_ZERO_COLUMN:
            assert any(want['prod'][j][v] == 0 for v in outside)
    assert {-1, 0, 1, ao.I64_MIN, ao.I64_MAX} == set(X[:, 3].tolist())


def test_conversion_inputs():
    x = ao.convert_i64_input(257)
    for v in (0, 1, -1, 2 ** 53 - 1, 2 ** 53 + 1, ao.I64_MAX, ao.I64_MIN):
        assert v in x.tolist()
    f = ao.i64_to_f64(x)
    assert f[x.tolist().index(2 ** 53 + 1)] == 2.0 ** 53 and f[x.tolist().index(2 ** 53 + 3)] == 2.0 ** 53 + 4
    y = ao.convert_f64_input(257)
    assert np.all(y == np.rint(y)) and y.max() == float(ao.BELOW_2_63) < 2.0 ** 63 and y.min() == -2.0 ** 63
    with np.errstate(all='raise'):
        back = ao.f64_to_i64(y)
    assert np.array_equal(back.astype(np.float64), y)
    for n in ao.LENGTHS:
        assert len(ao.convert_i64_input(n)) == n and len(ao.convert_f64_input(n)) == n
    small = np.random.default_rng(1).integers(-2 ** 53 + 1, 2 ** 53, size=1000)
    assert np.array_equal(ao.f64_to_i64(ao.i64_to_f64(small)), small)


def test_bit_pattern_columns_are_what_arithmetic_would_corrupt():
    B = ao.bit_pattern_columns(3, 5000, 1)
    f = B.view(np.float64)
    assert np.isnan(f).any() and (B == ao.SNAN_BITS).any() and (B == -1).any() and (B == 1).any()
    sub = (f != 0) & (np.abs(f) < np.finfo(np.float64).tiny)
    assert sub.any()
    with np.errstate(invalid='ignore'):
        moved = (f + 0.0).view(np.int64)                       # what a kernel that "adds zero" would store
    assert not np.array_equal(moved, B)


def test_transpose_refuses_a_tile_count_beyond_the_grid_before_any_launch():
    """grx_transpose launches ceil(cols / 32) x ceil(rows / 32) workgroups: a count that does not fit a 32-bit grid
    dimension is an error of the call (GRX_ERR_INVALID = -1), found before the pointers are looked at."""
    from graphrole_amd import _lib
    lib = _lib.load()
    for rows, cols in ((32 * 2 ** 31 + 1, 1), (1, 32 * 2 ** 31 + 1)):
        assert lib.grx_transpose(rows, cols, None, cols, None, rows, None) == -1
        assert b'32-bit grid' in lib.grx_last_error()
    assert lib.grx_transpose(32 * 65536 + 33, 3, None, 3, None, 32 * 65536 + 33, None) == -1
    assert b'NULL pointer' in lib.grx_last_error()            # 65 538 row tiles pass the shape checks
    assert lib.grx_transpose(0, 3, None, 3, None, 0, None) == 0
