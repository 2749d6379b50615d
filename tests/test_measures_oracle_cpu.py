"""
-m "not gpu": the long-double oracle of tests/measures_oracle.py against networkx on the small graphs of
tests/test_gpu_sense.py, and -- for every case tests/test_gpu_measures_kernels.py runs -- the two conditions that
make its comparison mean something: the stopping iteration is not within rounding of the threshold, and a plain
fp64 restatement stays a factor ten inside the GPU tests' 1e-12.
"""
import networkx as nx
import numpy as np
import pytest

from tests import measures_oracle as mo
from tests import sense_oracle
from tests.test_gpu_sense import GRAPHS as SENSE_GRAPHS, MAX_ITER as SENSE_MAX_ITER

MARGIN = 1e-6                                                  # |err / (N tol) - 1| at and before the stop
HEADROOM = 1e-13                                               # fp64 restatement against long double, relative


def _in_adjacency(G):
    nodelist = list(G)
    A = nx.to_scipy_sparse_array(G, nodelist=nodelist, weight='weight', dtype=float).T.tocsr()
    A.sort_indices()
    return nodelist, A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data


def test_long_double_is_extended_precision():
    assert np.finfo(np.longdouble).eps < 1e-18


@pytest.mark.parametrize('key', list(SENSE_GRAPHS))
def test_oracle_agrees_with_networkx_on_the_sense_graphs(key):
    G = SENSE_GRAPHS[key]()
    nodelist, row_ptr, col, w = _in_adjacency(G)
    max_iter = SENSE_MAX_ITER.get(key, 100)
    x, it, errs = mo.pagerank_ld(row_ptr, col, w, max_iter=max_iter)
    want = nx.pagerank(G, max_iter=max_iter)
    np.testing.assert_allclose(x.astype(np.float64), [want[v] for v in nodelist], rtol=1e-12, atol=0)
    assert it == sense_oracle.pagerank(G, max_iter=max_iter)[1] == len(errs)
    if G.is_multigraph():
        return                                                 # networkx has no eigenvector_centrality for it
    x, it, errs = mo.eigenvector_ld(row_ptr, col, w, max_iter=max_iter)
    want = nx.eigenvector_centrality(G, max_iter=max_iter, weight='weight')
    np.testing.assert_allclose(x.astype(np.float64), [want[v] for v in nodelist], rtol=1e-12, atol=0)
    assert it == sense_oracle.eigenvector(G, max_iter=max_iter)[1] == len(errs)


def test_unweighted_equals_unit_weights_and_empty_rows_are_zero():
    g = mo.graph('hubs_dir')
    assert (np.diff(g.row_ptr) == 0).any()
    for fn in (mo.pagerank_ld, mo.eigenvector_ld):
        a = fn(g.row_ptr, g.col, None)
        b = fn(g.row_ptr, g.col, np.ones(len(g.col)))
        assert a[1] == b[1] and np.array_equal(a[0], b[0])
    with pytest.raises(mo.NotConverged) as info:
        mo.pagerank_ld(g.row_ptr, g.col, None, max_iter=2)
    assert info.value.iterations == 2 and len(info.value.errs) == 2


def test_case_ids_are_unique_and_cover_the_issue_list():
    ids = [c.id for c in mo.CASES]
    assert len(set(ids)) == len(ids)
    for m in ('pagerank', 'eigenvector'):
        assert {c.stop_at for c in mo.CASES if c.measure == m and c.stop_at} == {1, 7, 8, 9, 16, 17}
        assert {c.lanes for c in mo.CASES if c.measure == m and c.graph == 'hubs_w'} == {4, 8, 16, 32}
        assert {c.tol for c in mo.CASES if c.measure == m and c.id.startswith('args-tol')} == {1e-3, 1e-10}
    assert {c.alpha for c in mo.CASES if c.id.startswith('args-alpha')} == {0.5, 0.99}


@pytest.mark.parametrize('cid', [c.id for c in mo.CASES])
def test_case_has_stopping_margin_and_fp64_headroom(cid):
    case = next(c for c in mo.CASES if c.id == cid)
    g = mo.graph(case.graph)
    tol = mo.case_tol(case)
    x, it, errs = mo.expected(case)
    assert len(errs) == it < mo.MAX_ITER
    if case.stop_at is not None:
        assert it == case.stop_at
    thresh = mo.LD(g.n) * mo.LD(tol)
    margins = [abs(float(e / thresh) - 1.0) for e in errs[-2:]]
    x64, it64, _ = mo.run(case, tol, dtype=np.float64)
    dev = mo.max_rel_dev(x64, x)
    print(f'{cid}: iterations {it}, margins {margins}, fp64 deviation {dev:.2e}')
    assert min(margins) > MARGIN, (cid, margins)               # 1. the count cannot flip under fp64 rounding
    assert it64 == it
    assert dev < HEADROOM, (cid, dev)                          # 2. a correct fp64 kernel is far inside 1e-12


def test_local_measures_follows_networkx():
    G = nx.gnm_random_graph(120, 500, seed=3)
    G.add_edges_from([(3, 3), (9, 9)])
    G.add_nodes_from([500, 501])
    nodes = sorted(G)
    idx = {v: i for i, v in enumerate(nodes)}
    src = [idx[u] for u, v in G.edges] + [idx[v] for u, v in G.edges if u != v]
    dst = [idx[v] for u, v in G.edges] + [idx[u] for u, v in G.edges if u != v]
    g = mo.csr_from_arcs(len(nodes), src, dst)
    own, nl = mo.loop_counts(g.row_ptr, g.col)
    T = np.array([nx.triangles(G, v) for v in nodes])
    cl, es = mo.local_measures(np.diff(g.row_ptr), own, T, nl)
    want_cl, want_es = nx.clustering(G), nx.effective_size(G)
    assert np.array_equal(cl, [want_cl[v] for v in nodes])
    want = np.array([want_es[v] for v in nodes])
    assert np.array_equal(np.isnan(es), np.isnan(want)) and np.array_equal(es[~np.isnan(want)], want[~np.isnan(want)])
    # degree 1 with T = 0: d'(d' - 1) = 0 never divides
    cl, es = mo.local_measures([1, 1, 0], [0, 1, 0], [0, 0, 0], [0, 0, 0])
    assert cl.tolist() == [0.0, 0.0, 0.0] and es[0] == 1.0 and np.isnan(es[1]) and np.isnan(es[2])
