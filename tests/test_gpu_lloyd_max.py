"""
-m gpu: grx_lloyd_max (csrc/grx_quant.hip), through kernels.lloyd_max only, against its stage-by-stage twin
tests/lloyd_max_oracle.py on every named case (prefix tiles, cell-cap and level-count switches, k == m, fewer
distinct values than levels, midpoint ties, signed data, max_iter, heavy tail through micro-cells, translation).

tests/test_lloyd_max_oracle_cpu.py shows, without a GPU, that every discrete decision of every case has a margin
>= 1e-9 (or is an exact tie of exactly representable numbers), so the device has to take the same decisions: the
checks on info and labels are equalities.  Centres: 1e-12 relative to max(|c|, spread).

Translation (x, x + 2**20, x + 2**27; exact shifts): same labels, centres that move with the shift, and an objective
within the rounding bound of centred fp64 prefix sums of the optimum (derived in the oracle's docstring; no constant
was taken from a device result).  The centres at a shift t are fp64 numbers near t, half an ulp of which is 1.2e-10 at
2**20 and 1.5e-8 at 2**27; the spread is 1024, so no fp64 output can be within 1e-12 * spread = 1e-9 of the unshifted
centre + 2**27.  The check is therefore 1e-12 * spread PLUS half an ulp of the shifted centre: the error of
(P[b] - P[a]) / n has to meet the 1e-12, the final rounding of pivot + that is what the format imposes.

Before the pivot (prefix sums of s and s^2 themselves: the library of the parent commit, loaded through GRX_LIB_PATH,
this module, MI355X): 43 of 48 pass.  Shift 0 and shift 2**20 pass for m = 600 and m = 5000 (the device adds its prefix
sums in a tree, which is more accurate than the index-order sums that lose the optimum from 2**20 on).  At 2**27
test_case[translation_m600_shift2p27], test_case[translation_m5000_shift2p27], test_translation[600] and
test_translation[5000] FAIL: info[0] is 2 (m = 600) and 3 (m = 5000) instead of 0 -- the DP returned a partition that
is not the optimum and Lloyd iterations had to repair it; on these two inputs they ended in the optimum's labels
(0 labels differ, objective - optimum = 0), which nothing guarantees.  test_case[k_eq_m_10000] FAILS there too: a
centre is 1.87e-12 of the spread from the value it is the mean of (uncentred P reaches 5e3), 1.0e-12 allowed.  These
are failing assertions, not faults.  With the pivot all 48 pass (largest centre error 0.59 of the tolerance, in k_eq_m_10000).
"""
import numpy as np
import pytest

from tests import lloyd_max_oracle as O

pytestmark = pytest.mark.gpu

_RUNS = {}


def _device(case):
    """(quantized, centers, info) of a case on the device, run once"""
    if case not in _RUNS:
        _RUNS[case] = _call(case)
    return _RUNS[case]


def _call(case):
    from graphrole_amd import kernels as K
    q, c, info = K.lloyd_max(K.to_device(O.data(case)), case.k, case.max_iter)
    return np.array(K.to_host(q)), np.array(K.to_host(c)), tuple(int(v) for v in K.to_host(info))


def _labels(q, centers):
    """the label of every value: the first cluster whose centre is, bit for bit, the quantised value (clusters of
    equal centre are an empty one above its heir, or equal means: the assign kernels send a value to the lowest)"""
    distinct, first = np.unique(centers, return_index=True)
    at = np.minimum(np.searchsorted(distinct, q), len(distinct) - 1)
    assert np.array_equal(distinct[at], q), 'a quantised value that is no centre'
    return first[at]


def _check_against_oracle(case, q, centers, info):
    ref = O.reference(case)
    print(case.name, 'info', info, 'oracle', ref.info, 'margins', ref.margins)
    assert info == ref.info
    labels = _labels(q, centers)
    differ = int(np.count_nonzero(labels != ref.labels))
    print(case.name, 'labels that differ', differ)
    assert differ == 0
    assert np.array_equal(q, centers[labels])
    spread = float(ref.s[-1] - ref.s[0])
    tol = 1e-12 * np.maximum(np.abs(ref.centers), spread)
    err = np.abs(centers - ref.centers)
    print(case.name, 'centre error / tolerance', float((err / np.maximum(tol, 1e-300)).max()))
    live = ref.counts > 0
    assert np.all(err[live] <= tol[live])
    # empty clusters: the centre they inherited, or kept from the iteration that emptied them
    assert np.all(err[~live] <= tol[~live])
    heirs = np.flatnonzero(~live[1:] & (ref.centers[1:] == ref.centers[:-1])) + 1
    assert np.array_equal(centers[heirs], centers[heirs - 1])


@pytest.mark.parametrize('case', O.CASES, ids=lambda c: c.name)
def test_case(case):
    q, centers, info = _device(case)
    _check_against_oracle(case, q, centers, info)
    if case.max_iter == 0:
        assert info[0] == 0                                    # the centres are the start's
    if case.m <= O.QC_BIG and not case.exact:
        assert info[0] == 0                                    # an optimum over one-value cells is a Lloyd fixed point
    again = _call(case)
    assert np.array_equal(q, again[0]) and np.array_equal(centers, again[1]) and info == again[2]


@pytest.mark.parametrize('m', sorted(O.TRANSLATION))
def test_translation(m):
    base, *shifted = O.TRANSLATION[m]
    q0, c0, info0 = _device(base)
    labels0 = _labels(q0, c0)
    spread = float(O.reference(base).s[-1] - O.reference(base).s[0])
    optimum = O.objective(O.data(base), O.reference(base).labels)
    for case in [base] + shifted:
        q, c, info = _device(case)
        labels = _labels(q, c)
        moved = np.abs((c - case.shift) - c0)
        tol = 1e-12 * spread + 0.5 * np.spacing(np.abs(c))
        excess = O.objective(O.data(case), labels) - optimum
        bound = O.rounding_bound(O.data(case))
        print(case.name, 'labels that differ from shift 0:', int(np.count_nonzero(labels != labels0)),
              'centre movement / tolerance', float((moved / tol).max()), 'objective - optimum', float(excess),
              'bound', float(bound), 'optimum', float(optimum))
        assert info == info0
        assert np.array_equal(labels, labels0)
        assert np.all(moved <= tol)
        assert excess <= bound
