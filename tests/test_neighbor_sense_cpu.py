"""
-m "not gpu": NeighborSense on the CPU.  The oracle of the kernel's summation order (tests/neighbor_sense_oracle.py)
against the dense authority A @ P within the derived bound, and the Python layer -- graphrole_amd.neighbor_roles,
RoleExtractor.neighbor_sense, graphrole_amd.role_mixing_matrix -- over a CPU double defined here: tests/fake_kernels plus
a numpy ``neighbor_roles`` (the oracle) and the two movers that place P^T and the row of ones; the NNLS is the real host
code of libgrx.so.  The device kernel itself is pinned on the GPU (tests/test_gpu_neighbor_sense.py).
"""
import types

import networkx as nx
import numpy as np
import pandas as pd
import pytest
import torch

from tests import fake_kernels, graphs, neighbor_sense_oracle as nso


# ------------------------------------------------------------------------------------------------- the CPU double
def _neighbor_roles(csr, P, mode='mean', w=None, r=None, lanes=0, out=None):
    r = int(P.shape[1] if r is None else r)
    N = torch.from_numpy(nso.neighbor_roles(csr.row_ptr, csr.col[:csr.nnz], None if w is None else np.asarray(w),
                                            P.numpy()[:csr.n, :r], mode))
    if out is None:
        return N
    out[:r, :csr.n] = N
    return out[:, :csr.n]


def _transpose(src, rows, cols, out=None):
    t = src[:rows, :cols].T.contiguous()
    if out is None:
        return t
    out[:cols, :rows] = t
    return out


def _upload_into(dst, a):
    dst.copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(dst.shape))


def _nnls(GtG, GtM, mm=None):
    from graphrole_amd.kernels import nnls                  # host-only entry point of libgrx.so
    return nnls(GtG, GtM, mm)


class _Forbidden:
    """A backend no refusal may reach."""

    def __getattr__(self, name):
        raise AssertionError(f'device work before the refusal: kernels.{name}')


@pytest.fixture
def cpu_backend():
    from graphrole_amd import backend
    double = types.SimpleNamespace(**{k: getattr(fake_kernels, k) for k in dir(fake_kernels) if not k.startswith('__')})
    double.neighbor_roles = _neighbor_roles
    double.transpose = _transpose
    double.upload_into = _upload_into
    double.nnls = _nnls
    backend.use(double)
    yield double
    backend.use(None)


@pytest.fixture
def no_backend():
    from graphrole_amd import backend
    backend.use(_Forbidden())
    yield
    backend.use(None)


def _frame(G, P, columns=None):
    return pd.DataFrame(P, index=sorted(G), columns=columns or [f'role_{k}' for k in range(P.shape[1])])


def _one_hot(G, r, seed=0):
    """(frame, node -> role label, role labels): hard roles with no empty role."""
    nodes = sorted(G)
    rng = np.random.default_rng(seed)
    which = np.concatenate([np.arange(r), rng.integers(0, r, len(nodes) - r)])
    rng.shuffle(which)
    roles = [f'role_{k}' for k in range(r)]
    return _frame(G, np.eye(r)[which], roles), {v: roles[k] for v, k in zip(nodes, which)}, roles


# ----------------------------------------------------------------------------- the oracle against the dense authority
CASES = nso.graph_cases()


@pytest.mark.parametrize('name', list(CASES))
def test_oracle_within_derived_bound_of_dense_authority(name):
    G = CASES[name]
    worst = 0.0
    for direction in (('out', 'in', 'all') if G.is_directed() else ('out',)):
        for weighted in (False, True):
            A = nso.adjacency(G, weighted, direction)
            row_ptr, col, w = nso.csr_of(A, weighted)
            for r in (1, 6, 17, 32):
                P = nso.memberships(len(A), r)
                for mode in ('sum', 'mean'):
                    N = nso.neighbor_roles(row_ptr, col, w, P, mode).T
                    want, bound = nso.dense(A, P, mode)
                    assert N.shape == want.shape and np.all(np.isfinite(N))
                    assert np.all(np.abs(N - want) <= bound), (direction, weighted, r, mode)
                    with np.errstate(divide='ignore', invalid='ignore'):
                        worst = max(worst, np.nanmax(np.where(bound > 0, np.abs(N - want) / bound, 0.0)))
                    assert np.all(N[np.count_nonzero(A, axis=1) == 0] == 0.0)
    # room to spare: the observed error is far inside the bound (d <= 1030 here, and errors do not all align)
    assert worst < 0.1, worst


def test_oracle_order_is_the_stated_one():
    # 11 arcs in 8 slots: slots 0..2 hold two terms, then the tree (s0 + s4) + (s2 + s6) + ((s1 + s5) + (s3 + s7))
    x = np.array([1e16, 1.0, -1e16, 3.0, 2.0 ** -30, 7.0, 1e-3, 5.0, -1.0, 2.0, 1e16])
    row_ptr, col = np.array([0, 11, 11]), np.concatenate([np.arange(11) % 2])
    P = np.zeros((2, 1))
    w = x.copy()
    P[:, 0] = 1.0
    s = [x[0] + x[8], x[1] + x[9], x[2] + x[10], x[3], x[4], x[5], x[6], x[7]]
    want = ((s[0] + s[4]) + (s[2] + s[6])) + ((s[1] + s[5]) + (s[3] + s[7]))
    got = nso.neighbor_roles(row_ptr, col, w, P, 'sum')
    assert got[0, 0] == want and got[0, 1] == 0.0
    in_turn = 0.0
    for term in x:
        in_turn += term
    assert want != in_turn                                    # the order matters for these terms


# ------------------------------------------------------------------------------------------------ the host path
@pytest.mark.parametrize('name', ['karate', 'loops_dangling', 'directed_weighted', 'directed_unweighted'])
def test_neighbor_roles_frame_against_dense(cpu_backend, name):
    from graphrole_amd import neighbor_roles
    G = CASES[name]
    P = nso.memberships(len(G), 5)
    frame = _frame(G, P, list('abcde'))
    for direction in ('out', 'in', 'all'):
        for weight in (None, 'weight'):
            for mode in ('mean', 'sum'):
                N = neighbor_roles(G, frame, weight=weight, mode=mode, direction=direction)
                assert list(N.index) == sorted(G) and list(N.columns) == list('abcde')
                assert all(dt == np.float64 for dt in N.dtypes)
                want, bound = nso.dense(nso.adjacency(G, weight is not None, direction), P, mode)
                assert np.all(np.abs(N.to_numpy() - want) <= bound), (direction, weight, mode)
    if not G.is_directed():                                   # one adjacency: the three directions are the same table
        a, b = neighbor_roles(G, frame, direction='out'), neighbor_roles(G, frame, direction='all')
        assert a.equals(b) and a.equals(neighbor_roles(G, frame, direction='in'))


def test_label_matching_shuffled_memberships(cpu_backend):
    from graphrole_amd import RoleExtractor, neighbor_roles, role_mixing_matrix
    G = nx.relabel_nodes(CASES['karate'], {v: f'n{v:02d}' for v in CASES['karate']})
    frame = _frame(G, np.abs(nso.memberships(len(G), 3)))
    shuffled = frame.iloc[np.random.default_rng(0).permutation(len(frame))]
    assert neighbor_roles(G, shuffled).equals(neighbor_roles(G, frame))
    assert role_mixing_matrix(G, shuffled).equals(role_mixing_matrix(G, frame))
    rx = RoleExtractor(n_roles=3)
    assert rx.neighbor_sense(G, shuffled).equals(rx.neighbor_sense(G, frame))


def test_four_path_by_hand(cpu_backend):
    from graphrole_amd import RoleExtractor, neighbor_roles, role_mixing_matrix
    G = nx.path_graph(4)
    frame = pd.DataFrame([[1, 0], [0, 1], [0, 1], [1, 0]], index=[0, 1, 2, 3], columns=['end', 'middle'])
    N = neighbor_roles(G, frame)
    assert N.to_numpy().tolist() == [[0, 1], [0.5, 0.5], [0.5, 0.5], [0, 1]]
    rx = RoleExtractor(n_roles=2)
    assert rx.role_affinity_factor is None
    Q = rx.neighbor_sense(G, frame)
    assert Q is rx.role_affinity_factor and rx.node_role_factor is None
    assert list(Q.index) == ['end', 'middle'] and list(Q.columns) == ['end', 'middle']
    np.testing.assert_allclose(Q.to_numpy(), [[0.0, 1.0], [0.5, 0.5]], rtol=0, atol=1e-15)
    assert role_mixing_matrix(G, frame).to_numpy().tolist() == [[0, 2], [2, 2]]
    assert neighbor_roles(G, frame, mode='sum').to_numpy().tolist() == [[0, 1], [1, 1], [1, 1], [0, 1]]


@pytest.mark.parametrize('name', ['er', 'directed_weighted'])
def test_one_hot_affinities_are_the_neighbour_shares(cpu_backend, name):
    """P's columns are orthogonal for one-hot roles, so column b of Q is the mean of N[:, b] over the nodes of each
    role: the row-stochastic role-to-role neighbour share (rows of nodes without neighbours pull it below 1)."""
    from graphrole_amd import RoleExtractor
    G = CASES[name]
    frame, role_of, roles = _one_hot(G, 4)
    for weight in (None, 'weight'):
        for direction in ('out', 'in', 'all'):
            Q = RoleExtractor(n_roles=4).neighbor_sense(G, frame, weight=weight, direction=direction)
            N, _ = nso.dense(nso.adjacency(G, weight is not None, direction), frame.to_numpy(dtype=np.float64), 'mean')
            P = frame.to_numpy(dtype=np.float64)
            share = (P.T @ N) / P.sum(axis=0)[:, None]
            np.testing.assert_allclose(Q.to_numpy(), share, rtol=0, atol=1e-12)
            assert np.all(Q.to_numpy() >= 0) and np.all(Q.to_numpy().sum(axis=1) <= 1 + 1e-12)


@pytest.mark.parametrize('name', ['karate', 'loops_dangling', 'directed_unweighted', 'directed_weighted'])
def test_mixing_matrix_is_the_exact_arc_count(cpu_backend, name):
    from graphrole_amd import role_mixing_matrix
    G = CASES[name]
    frame, role_of, roles = _one_hot(G, 3, seed=1)
    for direction in ('out', 'in', 'all'):
        C = role_mixing_matrix(G, frame, direction=direction)
        assert list(C.index) == roles and list(C.columns) == roles
        assert np.array_equal(C.to_numpy(), nso.arc_counts(G, role_of, roles, direction))
    if not G.is_directed():
        inside = [sum(1 for u, v in G.edges if u != v and role_of[u] == role_of[v] == role) for role in roles]
        loops = [sum(1 for u, v in G.edges if u == v and role_of[u] == role) for role in roles]
        assert np.diag(C.to_numpy()).tolist() == [2 * a + b for a, b in zip(inside, loops)]
    # weights: both sides sum at most ~300 positive terms per entry in their own order, each within 300 * 2^-53 = 3.3e-14
    # of the exact sum (relative)
    Cw = role_mixing_matrix(G, frame, weight='weight')
    np.testing.assert_allclose(Cw.to_numpy(), nso.arc_counts(G, role_of, roles, 'out', True), rtol=1e-13, atol=0)


def test_neighbor_sense_solves_the_nnls_and_normalises(cpu_backend):
    from graphrole_amd import RoleExtractor, neighbor_roles
    G = CASES['ba']
    P = np.abs(nso.memberships(len(G), 4))
    rx = RoleExtractor(n_roles=4)
    with pytest.raises(ValueError, match='fitted roles'):
        rx.neighbor_sense(G)
    rx.node_role_factor = _frame(G, P)
    before = rx.node_role_factor.copy()
    for normalize in (False, True):
        Q = rx.neighbor_sense(G, normalize=normalize)
        assert Q is rx.role_affinity_factor and Q.shape == (4, 4) and np.all(Q.to_numpy() >= 0)
        N = neighbor_roles(G, rx.node_role_factor).to_numpy()
        if normalize:
            N = N / N.mean(axis=0)
        for j in range(4):
            q, m = Q.to_numpy()[:, j], N[:, j]
            g = P.T @ (P @ q - m)
            eps = 1e-8 * np.sqrt(np.max(np.sum(P * P, axis=0)) * (m @ m))
            assert np.all(g[q == 0] >= -eps) and np.all(np.abs(g[q > 0]) <= eps), (normalize, j)
    assert rx.node_role_factor.equals(before)
    other = rx.neighbor_sense(CASES['er'], _frame(CASES['er'], np.abs(nso.memberships(300, 4, seed=5))))
    assert other.shape == (4, 4) and rx.node_role_factor.equals(before)
    with pytest.raises(NotImplementedError):
        rx.explain()


def test_empty_graph_gives_empty_frame(cpu_backend):
    from graphrole_amd import RoleExtractor, neighbor_roles, role_mixing_matrix
    frame = pd.DataFrame(np.zeros((0, 3)), columns=['a', 'b', 'c'])
    N = neighbor_roles(nx.Graph(), frame)
    assert N.shape == (0, 3) and list(N.columns) == ['a', 'b', 'c']
    assert role_mixing_matrix(nx.Graph(), frame).to_numpy().tolist() == [[0.0] * 3] * 3
    assert RoleExtractor(n_roles=3).neighbor_sense(nx.Graph(), frame).shape == (3, 3)


def test_catalogue_is_unchanged():
    from graphrole_amd import measures
    assert len(measures.CATALOGUE) == 16 and 'neighbor_roles' not in measures.CATALOGUE
    assert measures.available_measures(False, False) == ['degree', 'weighted_degree', 'clustering', 'effective_size',
                                                         'pagerank', 'eigenvector']


def test_entry_point_is_declared_and_registered():
    import os
    from graphrole_amd import _lib
    assert 'grx_neighbor_roles' in _lib.EXPORTED_SYMBOLS
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'grx.h')).read()
    assert 'int grx_neighbor_roles(' in header and 'GRX_NEIGHBOR_MEAN' in header
    assert hasattr(_lib.load(), 'grx_neighbor_roles')


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_before_any_device_work(no_backend):
    from graphrole_amd import RoleExtractor, neighbor_roles, role_mixing_matrix
    G = CASES['karate']
    good = _frame(G, np.abs(nso.memberships(len(G), 3)))
    rx = RoleExtractor(n_roles=3)

    def every(**kw):
        return [lambda: neighbor_roles(G, **kw), lambda: role_mixing_matrix(G, **{k: v for k, v in kw.items() if k != 'mode'}),
                lambda: rx.neighbor_sense(G, **kw)]

    for call in every(memberships=good, weight='cost'):
        with pytest.raises(NotImplementedError, match="'weight'"):
            call()
    for call in every(memberships=good, direction='both'):
        with pytest.raises(ValueError, match='direction'):
            call()
    for call in (lambda: neighbor_roles(G, good, mode='median'), lambda: rx.neighbor_sense(G, good, mode='max')):
        with pytest.raises(ValueError, match='mode'):
            call()
    bad_tables = {
        'DataFrame': good.to_numpy(),
        'role columns': good.iloc[:, :0],
        'GRX_MAX_ROLES': _frame(G, np.ones((len(G), 33))),
        'same labels': good.iloc[:-1],
        'the same labels': good.rename(index={0: 'zero'}),
        'duplicate': pd.concat([good.iloc[:-1], good.iloc[:1]]),
        'not numeric': good.assign(role_1='x'),
        'non-finite': good.assign(role_2=np.nan),
        'non-finite entries': good.assign(role_0=np.inf),
    }
    for match, table in bad_tables.items():
        for call in every(memberships=table):
            with pytest.raises(ValueError, match=match):
                call()
    for multi in (nx.MultiGraph(G), nx.MultiDiGraph(G)):
        with pytest.raises(NotImplementedError, match='parallel edges'):
            neighbor_roles(multi, good)
        with pytest.raises(NotImplementedError, match='parallel edges'):
            rx.neighbor_sense(multi, good, weight='weight')
    for bad in (-1.0, float('nan'), float('inf')):
        H = G.copy()
        H[0][1]['weight'] = bad
        for call in (lambda: neighbor_roles(H, good, weight='weight'), lambda: role_mixing_matrix(H, good, weight='weight'),
                     lambda: rx.neighbor_sense(H, good, weight='weight')):
            with pytest.raises(ValueError, match='finite and >= 0'):
                call()
    with pytest.raises(ValueError, match='fitted roles'):
        rx.neighbor_sense(G)
    assert rx.role_affinity_factor is None
    with pytest.raises(TypeError):
        neighbor_roles([(0, 1)], good)
