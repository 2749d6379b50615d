"""
-m gpu: csrc/grx_ingest.hip kernel by kernel against the numpy reference of tests/ingest_oracle.py, on the cases
listed there (tests/test_ingest_oracle_cpu.py checks what each of them reaches: scan tiles and the top chunk, sort
tiles, sentinel slots, both edge orientations, hub rows, every grid stride, the ballot loop, the 1023 saturation,
weight bit patterns).  Everything is compared with equality: integers, and weights as int64 bit patterns.
"""
import functools
from math import comb

import numpy as np
import pytest

from tests import ingest_oracle as io

pytestmark = pytest.mark.gpu

UNDIRECTED = [c.name for c in io.CASES if not c.directed]


def _ingest(name):
    from graphrole_amd import kernels as K
    n, src, dst, w, directed = io.graph(name)
    return K.device_ingest(n, src, dst, w, directed, io.expected(name).nnz)


@functools.lru_cache(maxsize=None)
def _ingested(name):
    """One ingest per case and module (the arrays stay in HBM for the tests that look at them)."""
    return _ingest(name)


def _host(t, count=None):
    a = t.cpu().numpy()
    return a if count is None else a[:count]


def _arrays(result, ref):
    """Every array grx_ingest returned, sliced to its valid length, weights as bit patterns."""
    perm, inv, row_ptr, out, tr = result
    got = {'perm': _host(perm).astype(np.int64), 'inv': _host(inv).astype(np.int64), 'row_ptr': np.asarray(row_ptr),
           'd_row_ptr': _host(out.row_ptr), 'col': _host(out.col, ref.nnz), 'agg_col': _host(out.agg_col, ref.nnz)}
    if out.w is not None:
        got['w'] = io.bits(_host(out.w, ref.nnz))
    if tr is not None:
        got['t_row_ptr'] = _host(tr.row_ptr)
        got['t_col'] = _host(tr.col, ref.m)
        if tr.w is not None:
            got['t_w'] = io.bits(_host(tr.w, ref.m))
    return got


def _first_difference(a, b):
    if a.shape != b.shape:
        return f'shapes {a.shape} / {b.shape}'
    at = np.flatnonzero(a != b)
    return f'{len(at)} differ, first at {at[0]}: {a[at[0]]} / {b[at[0]]}' if len(at) else 'equal'


@pytest.mark.parametrize('name', io.CASE_NAMES)
def test_ingest_arrays_equal_the_reference(name):
    ref = io.expected(name)
    result = _ingested(name)
    got = _arrays(result, ref)
    out, tr = result[3], result[4]
    assert out.n == ref.n and out.nnz == ref.nnz and (out.w is None) == (ref.w is None)
    assert (tr is None) == (not ref.directed)
    want = {'perm': ref.perm, 'inv': ref.inv, 'row_ptr': ref.row_ptr, 'd_row_ptr': ref.row_ptr, 'col': ref.col,
            'agg_col': ref.agg_col}
    if ref.w is not None:
        want['w'] = io.bits(ref.w)
    if ref.directed:
        want.update(t_row_ptr=ref.t_row_ptr, t_col=ref.t_col)
        if ref.t_w is not None:
            want['t_w'] = io.bits(ref.t_w)
    assert set(got) == set(want)
    for key in want:
        assert np.array_equal(got[key], want[key]), (name, key, _first_difference(got[key], want[key]))


def _assert_oriented(o, ref_o, what):
    o_nnz = int(ref_o.row_ptr[-1])
    assert o.nnz == o_nnz, what
    for key, got, want in (('row_ptr', _host(o.row_ptr), ref_o.row_ptr), ('col', _host(o.col, o_nnz), ref_o.col),
                           ('arc', _host(o.arc, o_nnz), ref_o.arc)):
        assert np.array_equal(got, want), (what, key, _first_difference(got, want))


@pytest.mark.parametrize('name', UNDIRECTED)
def test_orientation_of_the_ingested_graph_equals_the_reference(name):
    out = _ingested(name)[3]
    assert out._host[1] is None                               # no host columns: oriented() is the device path
    _assert_oriented(out.oriented(), io.expected_oriented(name), name)


@pytest.mark.parametrize('name', io.LABEL_ORDER_CASES)
def test_orientation_of_a_csr_that_is_not_degree_sorted(name):
    """grx_orient_count / grx_orient_fill on the LABEL-order CSR: the kernel apart from the ingest it normally
    follows (hub and clique rows in the middle of the row range, d' not monotone in the row index)."""
    from graphrole_amd import kernels as K
    row_ptr, col, ref_o = io.label_order(name)
    assert not np.all(np.diff(row_ptr)[1:] <= np.diff(row_ptr)[:-1])
    csr = K.DeviceCSR.from_device(K.to_device(row_ptr), K.to_device(col), None, None, row_ptr)
    assert not csr.degree_sorted
    _assert_oriented(csr._oriented_on_device(), ref_o, name)


@pytest.mark.parametrize('name', ['hubs', 'hubs_loop', 'clique1026'])
def test_triangle_counts_through_the_ingested_arrays(name):
    """The arrays drive the next kernel: triangle counts of the ingested graph, mapped back to label order, equal
    those of the host-built CSR of the same graph (numpy orientation); every node of K_1026 is in C(1025, 2)."""
    from graphrole_amd import kernels as K
    n = io.expected(name).n
    perm, inv, _, out, _ = _ingested(name)
    T_internal = _host(K.triangle_counts(out), n)
    T = T_internal[_host(inv).astype(np.int64)]
    row_ptr, col, _ = io.label_order(name)
    host_csr = K.DeviceCSR(row_ptr, col)
    assert np.array_equal(T, _host(K.triangle_counts(host_csr), n))
    if name == 'clique1026':
        assert np.all(T[io.clique_labels()] == comb(io.CLIQUE - 1, 2))
    else:
        # the big centre, a smaller centre and one of its leaves form a triangle; the cliques are on their own
        spokes = sum(cnt - 1 for cnt in io.HUB_STARS)
        assert T[io.HUB_BIG_LABEL] == spokes
        assert T.sum() == 3 * (spokes + sum(comb(k, 3) for k in io.HUB_CLIQUES))


def test_row_sums_through_the_ingested_directed_hub_arrays():
    """row_sums of the out CSR and of the transposed CSR (a 70 001-arc row each) against sequential sums in row order.
    The weights are multiples of 1 / 8 below 1000, so every order of the additions gives the same fp64 number."""
    from graphrole_amd import kernels as K
    name = 'dhubs_finite'
    ref = io.expected(name)
    _, _, _, out, tr = _ingested(name)
    for csr, row_ptr, w in ((out, ref.row_ptr, ref.w), (tr, ref.t_row_ptr, ref.t_w)):
        rows = np.repeat(np.arange(ref.n, dtype=np.int64), np.diff(row_ptr))
        want = np.bincount(rows, weights=w, minlength=ref.n)   # adds in array order
        got = _host(K.row_sums(csr, False), ref.n)
        assert np.array_equal(io.bits(got), io.bits(want)), _first_difference(got, want)
        assert want.max() > 70001 / 8


@pytest.mark.parametrize('name', ['hubs_loop_w', 'dhubs_w'])
def test_two_ingests_return_identical_arrays(name):
    """The degree atomics and the weight scatter must not leak their order into the result."""
    ref = io.expected(name)
    first, second = _arrays(_ingested(name), ref), _arrays(_ingest(name), ref)
    assert set(first) == set(second)
    for key in first:
        assert np.array_equal(first[key], second[key]), (name, key)


def test_a_short_workspace_is_refused_with_device_pointers_and_nothing_is_written():
    """GRX_ERR_WORKSPACE before any launch (tests/test_ingest_oracle_cpu.py checks the same without a device): the
    outputs keep the pattern they were filled with."""
    import torch
    from graphrole_amd import _lib
    from graphrole_amd import kernels as K
    n, src, dst, w, directed = io.graph('ring2049')
    m = len(src)
    lib = _lib.load()
    need = lib.grx_ingest_workspace_bytes(n, m, 0)
    d_src, d_dst = K.edges_to_device(src), K.edges_to_device(dst)
    outs = [K.to_device(np.full(2 * m + n + 1, -7, dtype=np.int64)) for _ in range(5)]
    ws = torch.empty(need, dtype=torch.uint8, device=K.device())
    p = K._ptr
    rc = lib.grx_ingest(n, m, p(d_src), p(d_dst), None, 0, 2 * m, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), None,
                        p(outs[4]), None, None, None, p(ws), need - 1, K._stream())
    assert rc == -3 and b'workspace' in lib.grx_last_error()
    K.synchronize()
    for t in outs:
        assert np.all(_host(t) == -7)
    o_need = lib.grx_orient_workspace_bytes(n)
    assert lib.grx_orient_count(n, p(outs[0]), p(outs[1]), p(outs[2]), p(ws), o_need - 1, K._stream()) == -3
    K.synchronize()
    assert np.all(_host(outs[2]) == -7)
