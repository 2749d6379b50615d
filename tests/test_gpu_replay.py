"""
-m gpu: ``RecursiveFeatureExtractor.replay_features`` on the device against values the REFERENCE produced -- the
candidate columns of every recorded generation of tests/golden/refex_*.npz, which include the columns pruning later
dropped and so check the aggregation chain independently of ``extract_features()`` -- against ``extract_features()``
itself (DataFrame.equals, dtypes included) and, across graphs, against tests/replay_oracle.py.
Unweighted graphs agree bit for bit, weighted ones within util.WEIGHTED_RTOL_FIXTURES.
"""
import numpy as np
import pytest

from tests import replay_oracle, util
from tests.test_gpu_refex import _graph_for

pytestmark = pytest.mark.gpu


def _extractor(name, **extra):
    from graphrole_amd import RecursiveFeatureExtractor
    g = util.load_refex(name)
    G, kwargs = _graph_for(name, g)
    return g, RecursiveFeatureExtractor(G, aggs=util.golden_aggs(g), max_generations=int(g['max_generations']),
                                        **dict(kwargs, **extra))


def _check_values(actual, expected, weighted, what):
    if weighted:
        np.testing.assert_allclose(actual, expected, rtol=util.WEIGHTED_RTOL_FIXTURES, atol=0, err_msg=what)
    else:
        assert np.array_equal(actual, expected), f'{what}: {int((actual != expected).sum())} entries differ'


@pytest.mark.parametrize('name', util.REFEX_CASES)
def test_replay_matches_the_reference(name):
    g, fe = _extractor(name)
    weighted = bool(len(g['w']))
    # every recorded generation's candidates, dropped ones included
    for gen in range(int(g['n_generations_recorded'])):
        names = g.js(f'g{gen}_cand_names')
        R = fe.replay_features(names)
        assert list(R.columns) == names and list(R.index) == g.js('labels')
        _check_values(R.to_numpy(dtype=np.float64), g[f'g{gen}_cand_values'], weighted, f'generation {gen}')
    # the final columns: the table extract_features() of a fresh extractor returns, dtypes included
    final = g.js('final_columns')
    R = fe.replay_features(final)
    assert fe._final_names == {} and not fe._work, 'replay left state behind'
    F = _extractor(name)[1].extract_features()
    assert list(F.columns) == final
    assert [str(t) for t in R.dtypes] == [str(t) for t in F.dtypes]
    if weighted:
        np.testing.assert_allclose(R.to_numpy(dtype=np.float64), F.to_numpy(dtype=np.float64),
                                   rtol=util.WEIGHTED_RTOL_FIXTURES, atol=0)
    else:
        assert R.equals(F)
    # extract_features() after a replay is what it always was; and a replay after it too
    F2 = fe.extract_features()
    assert F2.equals(F)
    R2 = fe.replay_features(final)
    assert R2.equals(R) and fe.extract_features().equals(F)


@pytest.mark.parametrize('fit,other', [('ba300', 'er300'), ('er300', 'ba300')])
def test_replay_on_another_graph_matches_the_oracle(fit, other):
    columns = util.load_refex(fit).js('final_columns')
    g, fe = _extractor(other)
    R = fe.replay_features(columns)
    og = util.oracle_graph_from_golden(g)
    names0, cols0 = util.typed_gen0(g)
    ref = replay_oracle.replay(og, names0, cols0, columns)
    assert list(R.columns) == columns and list(R.index) == g.js('labels')
    for nm in columns:
        assert R[nm].dtype == ref[nm].dtype, nm
        assert np.array_equal(R[nm].to_numpy(), ref[nm]), nm
    # not the table this graph's own extraction keeps: transfer needs the replay
    assert list(fe.extract_features().columns) != columns


@pytest.mark.parametrize('name', ['ba300_prodmean', 'karate_sumprodwrap', 'dw200_medianmax'])
def test_replay_typed_cases(name):
    """'prod' over integer columns (carried as wrapping int64) and 'median': the final table of the reference"""
    g, fe = _extractor(name)
    final = g.js('final_columns')
    R = fe.replay_features(final)
    weighted = bool(len(g['w']))
    util.assert_typed_final_equal(g, list(R.columns), {c: R[c].to_numpy() for c in R.columns},
                                  rtol=util.WEIGHTED_RTOL_FIXTURES if weighted else 0.0)
    F = _extractor(name)[1].extract_features()
    assert [str(t) for t in R.dtypes] == [str(t) for t in F.dtypes]
    if not weighted:
        assert R.equals(F)
