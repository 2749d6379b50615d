"""
No GPU: pins tests/lloyd_max_oracle.py, the twin grx_lloyd_max is compared with (tests/test_gpu_lloyd_max.py).

  * exact on tiny inputs: against every contiguous partition, costed in fractions.Fraction (doubles are dyadic
    rationals, so that arithmetic has no rounding at all);
  * the fast DP (monotone arg-min over a band) against the O(k cells^2) statement of the same recurrence;
  * translation-invariant by construction: exact shifts give identical edges, identical centred centres, pivots that
    differ by the shift;
  * an optimum over one-value cells is a Lloyd fixed point: zero iterations on every tie-free case with m <= 8192;
  * flip-free: on EVERY entry of CASES the fp64 run and the long-double run take the same discrete decisions, and every
    decision has a margin >= 1e-9, so the order of the device's fp64 additions cannot flip one.

Seeds chosen for the flip-free condition (the list of cases is the issue's; only seeds moved): 'heavy_tail_m30000_k64'
has seed 17 -- with lognormal(0, 2) the span is ~1e3 and the dense values near 0 lie ~3e-9 of it apart, so most seeds
have some Lloyd search within 1e-9 (seeds 9 and 11 to 13 gave 6e-11 to 7e-10); 'levels_m20000_k256/257' have seed 20
(seed 3 gave 9.7e-10) and draw rand()**3: an unbounded tail gives the companding start of 257 levels an empty cell
above a one-value cell, whose inherited centre IS that value -- a tie by construction.

Exact cases (Case.exact: small integers or a constant).  Fewer distinct values than levels means clusters of equal
centre, whose midpoint is that centre and a value of the data: a Lloyd margin of 0 is what these cases are for, as it is
for the midpoint-tie case.  For all of them the test demands instead that nothing is rounded: every centre of every
iteration and every midpoint is the same number in fp64 and in long double.  Their DP ties are exact too: the tied
candidates cost 0 (clusters of one repeated value, D = 0 before them), in any arithmetic.
"""
import itertools
from fractions import Fraction

import numpy as np
import pytest

from tests import lloyd_max_oracle as O

LD_EPS = float(np.finfo(np.longdouble).eps)


def _frac(v):
    """a long double as the rational it is"""
    return Fraction(*[int(t) for t in np.longdouble(v).as_integer_ratio()])


def _fraction_optimum(sorted_values, kk):
    """(cost, edges) of every optimal partition of the sorted values into kk non-empty contiguous clusters"""
    f = [Fraction(float(v)) for v in sorted_values]
    m = len(f)
    best, arg = None, []
    for cut in itertools.combinations(range(1, m), kk - 1):
        edges = (0,) + cut + (m,)
        cost = Fraction(0)
        for a, b in zip(edges[:-1], edges[1:]):
            mean = sum(f[a:b]) / (b - a)
            cost += sum((v - mean) ** 2 for v in f[a:b])
        if best is None or cost < best:
            best, arg = cost, [edges]
        elif cost == best:
            arg.append(edges)
    return best, arg


@pytest.mark.parametrize('shift', [0.0, float(1 << 27)])
@pytest.mark.parametrize('m,k', [(1, 1), (2, 2), (5, 2), (8, 3), (11, 4), (12, 6), (12, 12), (12, 1)])
def test_tiny_inputs_equal_exhaustive_search_in_fractions(m, k, shift):
    rng = np.random.RandomState(100 * m + k)
    x = rng.randint(0, 1 << 20, m) / 1024.0 + shift           # the shift is exact
    r = O.quantise(x, k)
    s = np.sort(x)
    cost, arg = _fraction_optimum(s, min(k, m))
    assert len(arg) == 1, 'the tiny inputs have one optimum'
    assert tuple(r.dp_edges) == arg[0]
    assert abs(_frac(r.dp_cost) - cost) <= 64 * LD_EPS * cost
    assert r.iterations == 0 and tuple(r.hi) == arg[0][1:]
    f = [Fraction(float(v)) for v in s]
    for j, (a, b) in enumerate(zip(arg[0][:-1], arg[0][1:])):
        mean = sum(f[a:b]) / (b - a)
        assert abs(Fraction(float(r.centers[j])) - mean) <= 2.0 ** -52 * max(abs(mean), 1)
        centred = _frac(r.centers_centred[j]) + Fraction(float(r.pivot))
        assert abs(centred - mean) <= 8 * LD_EPS * 1024
    assert np.array_equal(np.sort(r.labels), np.repeat(np.arange(min(k, m)), np.diff(arg[0])))
    assert np.all(np.diff(r.labels[r.order]) >= 0)
    assert abs(_frac(O.objective(x, r.labels)) - cost) <= 64 * LD_EPS * max(cost, 1)


@pytest.mark.parametrize('name,m,k', [('uniform', 60, 7), ('gamma', 400, 33), ('randint5', 300, 8), ('constant', 50, 4),
                                      ('lognormal1', 9000, 6), ('randint20', 9000, 32), ('grid4', 8220, 4)])
def test_fast_dp_equals_the_plain_recurrence(name, m, k):
    x = getattr(O, '_' + name)(np.random.RandomState(21), m)
    fast = O.quantise(x, k, 0)
    edges, cost = O.dp_plain(x, k)
    assert np.array_equal(fast.dp_edges, edges)
    assert abs(fast.dp_cost - cost) <= 8 * LD_EPS * cost


@pytest.mark.parametrize('m', sorted(O.TRANSLATION))
def test_exact_shifts_change_nothing_but_the_pivot(m):
    base, *shifted = O.TRANSLATION[m]
    assert base.shift == 0 and [c.shift for c in shifted] == [2.0 ** 20, 2.0 ** 27]
    r0 = O.reference(base)
    for case in shifted:
        assert np.array_equal(O.data(case) - case.shift, O.data(base)), 'the shift is exact'
        for run0, run in ((r0, O.reference(case)), (_float64(base), _float64(case))):
            assert run.pivot - run0.pivot == case.shift
            assert np.array_equal(run.cell_edges, run0.cell_edges) and np.array_equal(run.dp_edges, run0.dp_edges)
            assert np.array_equal(run.hi, run0.hi) and run.info == run0.info
            assert np.array_equal(run.labels, run0.labels)
            assert np.array_equal(run.centers_centred, run0.centers_centred)
            assert run.dp_cost == run0.dp_cost
        assert np.abs((O.reference(case).centers - case.shift) - r0.centers).max() <= 2.0 ** -52 * case.shift


_F64 = {}


def _float64(case):
    if case not in _F64:
        _F64[case] = O.quantise_float64(O.data(case), case.k, case.max_iter)
    return _F64[case]


def test_the_named_shapes_are_all_there():
    have = {(c.m, c.k) for c in O.CASES}
    want = {(m, k) for m in (1, 2, 7, 2047, 2048, 2049, 4097) for k in (1, 2, 5) if k <= m}
    want |= {(1024, 16), (1025, 16), (8192, 4), (8193, 4), (3000, 256), (3000, 257), (20000, 256), (20000, 257),
             (1, 1), (300, 300), (1500, 1500), (10000, 10000), (5000, 8), (20000, 32), (5000, 16), (30000, 64),
             (600, 8), (5000, 8)}
    assert want <= have
    by_name = {c.name: c for c in O.CASES}
    assert len(by_name) == len(O.CASES)
    assert sorted(c.max_iter for c in O.CASES if c.name.startswith('max_iter')) == [0, 1, 300]
    assert all(c.m > O.QC_BIG and c.k <= O.Q_MAX_BINS for c in O.CASES if c.name.startswith('max_iter'))
    # what each case is for really happens in it
    r = O.reference(by_name['few_distinct_randint5_m5000_k8'])
    assert len(np.unique(O.data(by_name['few_distinct_randint5_m5000_k8']))) == 5 and r.nonempty < 8 and r.dp_ties
    r = O.reference(by_name['few_distinct_randint20_m20000_k32'])
    assert len(r.cell_edges) - 1 == 20 < 32 and r.nonempty == 20 and np.all(r.centers[20:] == r.centers[19])
    r = O.reference(by_name['constant_m9000_k4'])
    assert r.Gp[-1] == 0 and list(r.cell_edges) == [0, 1, 9000]
    r = O.reference(by_name['midpoint_ties_grid_m8220_k4'])
    assert r.margins['lloyd'] == 0 and r.iterations >= 2 and r.nonempty == 4, 'values sit exactly on a midpoint'
    r = O.reference(by_name['k_eq_m_10000'])
    assert r.dp_edges is None and np.array_equal(r.start_edges, np.arange(10001))
    r0, r1 = O.reference(by_name['max_iter0_m12000_k32']), O.reference(by_name['max_iter300_m12000_k32'])
    assert r0.info[0] == 0 and r1.info[0] > 1 and np.array_equal(r0.hi, r0.dp_edges[1:])
    assert np.array_equal(r0.centers_centred, r1.c_history[0])
    assert O.reference(by_name['max_iter1_m12000_k32']).info[0] == 1


@pytest.mark.parametrize('case', O.CASES, ids=lambda c: c.name)
def test_case_is_flip_free_and_the_exact_path_needs_no_iteration(case):
    ld, dd = O.reference(case), _float64(case)
    # every discrete decision agrees between fp64 and long double
    for a, b in ((ld.cell_edges, dd.cell_edges), (ld.dp_edges, dd.dp_edges), (ld.start_edges, dd.start_edges),
                 (ld.hi, dd.hi), (ld.labels, dd.labels)):
        assert (a is None and b is None) or np.array_equal(a, b)
    assert len(ld.hi_history) == len(dd.hi_history)
    assert all(np.array_equal(a, b) for a, b in zip(ld.hi_history, dd.hi_history))
    assert ld.info == dd.info
    # every margin >= 1e-9
    for run in (ld, dd):
        assert run.margins['cells'] >= O.MARGIN, run.margins
        assert run.margins.get('dp', np.inf) >= O.MARGIN, run.margins
        if not case.exact:
            assert run.margins['lloyd'] >= O.MARGIN and run.margins['assign'] >= O.MARGIN, run.margins
            assert not run.dp_ties
    if case.exact:
        # nothing is rounded: centres and midpoints are the same numbers in both formats; DP ties are ties of zeros
        assert ld.dp_ties == dd.dp_ties and all(t == 0.0 for t in ld.dp_ties)
        for a, b in zip(ld.c_history, dd.c_history):
            assert np.array_equal(a.astype(np.float64), b) and np.array_equal(a, b.astype(np.longdouble))
            mid = 0.5 * (a[:-1] + a[1:])
            assert np.array_equal(mid.astype(np.float64).astype(np.longdouble), mid)
        assert np.array_equal(ld.centers, dd.centers)
    else:
        scale = max(float(ld.s[-1] - ld.s[0]), 1e-300)
        assert np.abs(ld.centers - dd.centers).max() <= 1e-12 * max(scale, np.abs(ld.centers).max())
    # an optimum over one-value cells is a Lloyd fixed point
    if case.m <= O.QC_BIG and not case.exact:
        assert ld.iterations == 0 and dd.iterations == 0
