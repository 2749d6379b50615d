"""
The device-steered round loops (csrc/grx_common.h: grx_run_rounds, grx_read_ctrl, grx_frontier_advance) on the MI355X,
with the number of rounds on either side of every batch boundary: kernels.distance_sums, betweenness, biconnected and
core_numbers on every path of 1 .. 40 nodes (tests/round_loop_cases.py; tests/test_round_loops_cpu.py pins that these
reach 7 / 8 / 9, 15 / 16 / 17, 23 / 24 / 25 level launches and 15 / 16 / 17 peeling rounds), equal to the oracles --
integers, whole multiples of the scale and the correctly rounded harmonic sum: every assertion is an equality.  Then
the five loop families one after another and again in reverse order (they share one pinned control block per host
thread), and a call from a second host thread (a fresh block).
"""
import threading

import networkx as nx
import numpy as np
import pytest

from tests import round_loop_cases as rl

pytestmark = pytest.mark.gpu

KINDS = pytest.mark.parametrize('directed', [False, True], ids=['undirected', 'directed'])
SIZES = pytest.mark.parametrize('n', rl.SIZES)


def _device_csrs(n, directed):
    """(out, in) DeviceCSRs of the path, rows in node order; undirected: in is None."""
    from graphrole_amd import kernels as K
    row_ptr, col, in_row_ptr, in_col = rl.path_csrs(n, directed)
    return K.DeviceCSR(row_ptr, col), (K.DeviceCSR(in_row_ptr, in_col) if directed else None)


def _distance_sums(n, directed):
    from graphrole_amd import kernels as K
    out, tr = _device_csrs(n, directed)
    got = K.distance_sums(tr if directed else out, np.arange(n, dtype=np.int64))     # pulled over the in-adjacency
    return tuple(K.to_host(t)[:n].copy() for t in got)


def _betweenness(n, directed):
    from graphrole_amd import kernels as K
    out, tr = _device_csrs(n, directed)
    bc = K.betweenness(out, tr, np.arange(n, dtype=np.int64), False, rl.betweenness_scale(n, directed))
    return K.to_host(bc)[:n].copy()


def _biconnected(n):
    from graphrole_amd import kernels as K
    count, parent, label, n_components = K.biconnected(_device_csrs(n, False)[0])
    return tuple(K.to_host(t)[:n].copy() for t in (count, parent, label)) + (n_components,)


def _core_numbers(n, directed):
    from graphrole_amd import kernels as K
    core, onion, n_rounds = K.core_numbers(*_device_csrs(n, directed))
    return K.to_host(core)[:n].copy(), K.to_host(onion)[:n].copy(), n_rounds


def _pagerank(n):
    from graphrole_amd import kernels as K
    out, _ = _device_csrs(n, False)
    x, iterations = K.pagerank(out, K.row_sums(out, False), 0.85, 1e-6, 100)
    return K.to_host(x)[:n].copy(), iterations


@KINDS
@SIZES
def test_distance_sums(n, directed):
    reach, dsum, harmonic = _distance_sums(n, directed)
    w_reach, w_dsum, w_harmonic = rl.distance_sums(n, directed)
    assert np.array_equal(reach, w_reach)
    assert np.array_equal(dsum, w_dsum)
    assert harmonic.tobytes() == w_harmonic.tobytes()          # the correctly rounded sum: bit-equal


@KINDS
@SIZES
def test_betweenness(n, directed):
    assert _betweenness(n, directed).tobytes() == rl.betweenness(n, directed).tobytes()


@SIZES
def test_biconnected(n):
    count, parent, label, n_components = _biconnected(n)
    want = rl.biconnected(n)
    assert np.array_equal(count, want.count)
    assert np.array_equal(parent, want.parent)
    assert np.array_equal(label, want.label)
    assert n_components == want.n_components == n - 1           # every edge of a path is a component of its own


@KINDS
@SIZES
def test_core_numbers(n, directed):
    core, onion, n_rounds = _core_numbers(n, directed)
    want = rl.core_numbers(n, directed)
    assert np.array_equal(core, want.core)
    assert np.array_equal(onion, want.onion)
    assert n_rounds == want.n_rounds == int(onion.max())
    G = nx.path_graph(n, create_using=nx.DiGraph if directed else nx.Graph)
    assert dict(enumerate(core.tolist())) == nx.core_number(G)
    if not directed:
        assert dict(enumerate(onion.tolist())) == nx.onion_layers(G)


def _flat(result):
    return b''.join(np.asarray(part).tobytes() for part in result)


def test_the_five_families_share_one_control_block():
    families = [lambda: _pagerank(17), lambda: (_betweenness(17, False),), lambda: _distance_sums(17, False),
                lambda: _biconnected(17), lambda: _core_numbers(17, False)]
    first = [_flat(run()) for run in families]
    second = [_flat(run()) for run in reversed(families)][::-1]
    assert second == first
    assert np.array_equal(np.frombuffer(first[2], dtype=np.int64)[:17], rl.distance_sums(17, False)[0])
    assert np.array_equal(np.frombuffer(first[4], dtype=np.int64)[:17], rl.core_numbers(17, False).core)


def test_a_second_host_thread_gets_its_own_control_block():
    main = _distance_sums(9, False)
    got = []
    worker = threading.Thread(target=lambda: got.append(_distance_sums(9, False)))
    worker.start()
    worker.join()
    assert len(got) == 1 and _flat(got[0]) == _flat(main)
    assert np.array_equal(main[1], rl.distance_sums(9, False)[1])
