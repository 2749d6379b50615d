"""
GPU: NeighborSense.  grx_neighbor_roles (csrc/grx_neighbor_sense.hip) against the numpy restatement of its summation
order bit for bit -- every graph of tests/neighbor_sense_oracle.graph_cases (the star's centre takes the workgroup path
beside empty rows), every width of WIDTHS, both modes, with and without weights, every direction, a padded leading
dimension, every lanes_per_row, twice -- and within the derived bound of the dense authority A @ P; then
RoleExtractor.neighbor_sense end to end on karate (KKT conditions and scipy's objective with the tolerances of
tests/test_gpu_sense.py), the transfer to a second graph, role_mixing_matrix against Python arc counts, and the argument
errors.
"""
import networkx as nx
import numpy as np
import pandas as pd
import pytest

from tests import graphs, neighbor_sense_oracle as nso

pytestmark = pytest.mark.gpu

CASES = nso.graph_cases()


def _bits(K, N, want, what):
    got = K.to_host(N)
    assert got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), (what, float(np.max(np.abs(got - want))))


@pytest.mark.parametrize('name', list(CASES))
def test_kernel_parity_bit_for_bit(name):
    from graphrole_amd import kernels as K
    assert K.NS_LONG_ROW == nso.LONG_ROW
    G = CASES[name]
    for direction in (('out', 'in', 'all') if G.is_directed() else ('out',)):
        for weighted in (False, True):
            A = nso.adjacency(G, weighted, direction)
            row_ptr, col, w = nso.csr_of(A, weighted)
            if name == 'star':
                assert np.diff(row_ptr).max() == nso.LONG_ROW + 1 and np.diff(row_ptr).min() == 0
            csr = K.DeviceCSR(row_ptr, col, w)
            n = csr.n
            for r in nso.WIDTHS:
                padded = nso.memberships(n, r, ld=r + 3)
                P = np.ascontiguousarray(padded[:, :r])
                Pd, Pp = K.to_device(P), K.to_device(padded)
                for mode in ('sum', 'mean'):
                    what = (direction, weighted, r, mode)
                    want = nso.neighbor_roles(row_ptr, col, w, P, mode)
                    assert np.all(np.isfinite(want)) and np.all(want[:, np.diff(row_ptr) == 0] == 0.0)
                    _bits(K, K.neighbor_roles(csr, Pd, mode, csr.w), want, what)
                    _bits(K, K.neighbor_roles(csr, Pd, mode, csr.w), want, what + ('again',))
                    _bits(K, K.neighbor_roles(csr, Pp, mode, csr.w, r=r), want, what + ('ld = r + 3',))
                    for lanes in K.neighbor_lanes(r):
                        _bits(K, K.neighbor_roles(csr, Pd, mode, csr.w, lanes=lanes), want, what + (lanes,))
                    dense, bound = nso.dense(A, P, mode)
                    assert np.all(np.abs(want.T - dense) <= bound), what


def test_output_block_under_the_transpose():
    """The layout neighbor_sense uses: N written into the lower half of a [2 r, n] block, nothing else touched."""
    from graphrole_amd import kernels as K
    A = nso.adjacency(CASES['ba'], False)
    row_ptr, col, w = nso.csr_of(A, False)
    csr = K.DeviceCSR(row_ptr, col)
    n, r = csr.n, 6
    P = nso.memberships(n, r)
    X = K.to_device(np.full((2 * r + 1, n), -7.0))
    K.transpose(K.to_device(P), n, r, out=X[:r])
    K.neighbor_roles(csr, K.to_device(P), 'mean', out=X[r:2 * r])
    got = K.to_host(X)
    assert got[:r].tobytes() == np.ascontiguousarray(P.T).tobytes()
    assert got[r:2 * r].tobytes() == nso.neighbor_roles(row_ptr, col, None, P, 'mean').tobytes()
    assert np.all(got[2 * r] == -7.0)


@pytest.fixture(scope='module')
def karate_roles():
    from graphrole_amd import RecursiveFeatureExtractor, RoleExtractor
    G = nx.karate_club_graph()
    features = RecursiveFeatureExtractor(G).extract_features()
    np.random.seed(0)
    role_extractor = RoleExtractor(n_roles=3)
    role_extractor.extract_role_factors(features)
    return G, role_extractor


def test_karate_end_to_end_neighbor_sense(karate_roles):
    scipy_optimize = pytest.importorskip('scipy.optimize')
    from graphrole_amd import neighbor_roles
    G, role_extractor = karate_roles
    assert role_extractor.role_affinity_factor is None
    roles = ['role_0', 'role_1', 'role_2']
    Pf = role_extractor.node_role_factor
    P = Pf.to_numpy(dtype=np.float64)
    before = Pf.copy()
    for kwargs in ({}, {'normalize': True}, {'weight': 'weight', 'mode': 'sum'}):
        Q = role_extractor.neighbor_sense(G, **kwargs)
        assert Q is role_extractor.role_affinity_factor
        assert list(Q.index) == roles and list(Q.columns) == roles and np.all(Q.to_numpy() >= 0)
        N = neighbor_roles(G, Pf, weight=kwargs.get('weight'), mode=kwargs.get('mode', 'mean'))
        assert list(N.index) == list(Pf.index) and list(N.columns) == roles
        dense, bound = nso.dense(nso.adjacency(G, 'weight' in kwargs), P, kwargs.get('mode', 'mean'))
        assert np.all(np.abs(N.to_numpy() - dense) <= bound)
        Nv = N.to_numpy(dtype=np.float64)
        if kwargs.get('normalize'):
            Nv = Nv / Nv.mean(axis=0)
        for j, name in enumerate(roles):
            q, m = Q[name].to_numpy(), Nv[:, j]
            g = P.T @ (P @ q - m)
            eps = 1e-8 * np.sqrt(np.max(np.sum(P * P, axis=0)) * (m @ m))
            assert np.all(g[q == 0] >= -eps) and np.all(np.abs(g[q > 0]) <= eps), (kwargs, name)
            x_ref, _ = scipy_optimize.nnls(P, m)
            obj, obj_ref = np.sum((P @ q - m) ** 2), np.sum((P @ x_ref - m) ** 2)
            assert abs(obj - obj_ref) <= 1e-10 * (m @ m), (kwargs, name)
    # the same table in another row order; an explicit table; nothing fitted changed
    Q = role_extractor.neighbor_sense(G)
    shuffled = Pf.iloc[np.random.default_rng(0).permutation(len(Pf))]
    assert role_extractor.neighbor_sense(G, shuffled).equals(Q)
    assert role_extractor.node_role_factor.equals(before)
    with pytest.raises(NotImplementedError):
        role_extractor.explain()


def test_transfer_to_a_second_graph():
    from graphrole_amd import RecursiveFeatureExtractor, RoleExtractor, role_mixing_matrix
    Ga, Gb = graphs.ba(300, 3, 1)[0], graphs.ba(300, 3, 2)[0]
    features_a = RecursiveFeatureExtractor(Ga).extract_features()
    np.random.seed(0)
    role_extractor = RoleExtractor(n_roles=3)
    role_extractor.extract_role_factors(features_a)
    before = role_extractor.node_role_factor.copy()
    Qa = role_extractor.neighbor_sense(Ga).copy()
    features_b = RecursiveFeatureExtractor(Gb).replay_features(features_a.columns)
    Pb = role_extractor.transform(features_b)
    Qb = role_extractor.neighbor_sense(Gb, Pb)
    r = before.shape[1]
    assert Qa.shape == (r, r) and Qb.shape == (r, r) and np.all(Qb.to_numpy() >= 0) and np.all(Qa.to_numpy() >= 0)
    assert list(Qb.index) == list(Pb.columns) and list(Qb.columns) == list(Pb.columns)
    assert Qb is role_extractor.role_affinity_factor
    assert role_extractor.node_role_factor.equals(before)
    # the dominant hard roles of B: the block-model arc counts, exact
    roles = list(Pb.columns)
    first = Pb.to_numpy().argmax(axis=1)
    hard = pd.DataFrame(np.eye(r)[first], index=Pb.index, columns=roles)
    role_of = {v: roles[k] for v, k in zip(Pb.index, first)}
    C = role_mixing_matrix(Gb, hard)
    assert np.array_equal(C.to_numpy(), nso.arc_counts(Gb, role_of, roles))
    assert C.to_numpy().sum() == 2 * Gb.number_of_edges()


def test_mixing_matrix_directions_exact():
    from graphrole_amd import role_mixing_matrix
    G = CASES['directed_unweighted']
    nodes = sorted(G)
    roles = ['a', 'b', 'c', 'd']
    which = np.random.default_rng(3).integers(0, 4, len(nodes))
    hard = pd.DataFrame(np.eye(4)[which], index=nodes, columns=roles)
    role_of = {v: roles[k] for v, k in zip(nodes, which)}
    for direction in ('out', 'in', 'all'):
        C = role_mixing_matrix(G, hard, direction=direction)
        assert np.array_equal(C.to_numpy(), nso.arc_counts(G, role_of, roles, direction)), direction


def test_sizes_and_argument_errors():
    from graphrole_amd import _lib, kernels as K, neighbor_roles
    lib = _lib.load()
    csr = K.DeviceCSR(np.array([0, 1, 2]), np.array([1, 0]))
    P = K.to_device(np.ones((2, 40)))
    out = K.empty((40, 2))
    stream = K._stream()

    def status(n, r, mode=1, lanes=0, ldp=40, ld_out=2, row_ptr=csr.row_ptr, p=P):
        return lib.grx_neighbor_roles(n, K._ptr(row_ptr), K._ptr(csr.col), None, K._ptr(p), ldp, r, mode, lanes,
                                      K._ptr(out), ld_out, stream)

    assert status(2, 32) == 0 and all(status(2, 3, lanes=lanes) == 0 for lanes in K.neighbor_lanes(3))
    assert K.neighbor_lanes(1) == (1, 2, 4, 8) and K.neighbor_lanes(6) == (4, 8, 16, 32) and K.neighbor_lanes(32) == (16, 32, 64)
    assert status(0, 3) == 0 and status(0, 3, row_ptr=None, p=None) == 0     # n = 0 returns at once
    assert status(2, 33) == -4                                                # GRX_ERR_UNSUPPORTED
    for bad in (dict(n=-1, r=3), dict(n=2, r=0), dict(n=2, r=3, mode=2), dict(n=2, r=3, lanes=3),
                dict(n=2, r=3, lanes=32), dict(n=2, r=3, lanes=-2), dict(n=2, r=32, lanes=8), dict(n=2, r=32, lanes=128), dict(n=2, r=3, ldp=2), dict(n=2, r=3, ld_out=1),
                dict(n=2, r=3, row_ptr=None), dict(n=2, r=3, p=None)):
        assert status(**bad) == -1, bad                                       # GRX_ERR_INVALID
    with pytest.raises(_lib.GrxError, match='GRX_MAX_ROLES'):
        K.neighbor_roles(csr, P, 'mean', r=33)
    with pytest.raises(_lib.GrxInvalid, match='lanes_per_row'):
        K.neighbor_roles(csr, P, 'mean', r=3, lanes=3)
    with pytest.raises(ValueError, match='mode'):
        K.neighbor_roles(csr, P, 'median', r=3)
    empty = K.neighbor_roles(K.DeviceCSR(np.array([0]), np.zeros(0, np.int32)), K.empty((0, 3)), 'mean')
    assert tuple(empty.shape) == (3, 0)
    G = nx.path_graph(3)
    with pytest.raises(ValueError, match='GRX_MAX_ROLES'):
        neighbor_roles(G, pd.DataFrame(np.ones((3, 33)), index=[0, 1, 2]))
    assert neighbor_roles(nx.Graph(), pd.DataFrame(np.zeros((0, 2)), columns=['a', 'b'])).shape == (0, 2)
    # the device still answers after the refusals
    N = K.to_host(K.neighbor_roles(csr, P, 'sum', r=2))
    assert N.tolist() == [[1.0, 1.0], [1.0, 1.0]]
