"""
Core number and onion layers on the MI355X: graphrole_amd.core_number and onion_layers equal to networkx computed here
(integers: exact) on every graph kind -- hub rows, a star whose centre takes 1 500 decrements in one round, a 300-round
path that crosses several read-back batches, a clique behind a long tail (k jumps 1 -> 39) and directed graphs with hub
rows in both CSRs and reciprocal arcs included; the same result for a relabelled copy and in a second run;
kernels.core_numbers on the adapter's structure CSRs against tests/kcore_oracle.py, at full size on BA 1 M / 10 M; and
the karate sense-making run with both columns.
"""
import networkx as nx
import numpy as np
import pytest

from tests import kcore_oracle as ko

pytestmark = pytest.mark.gpu


def _disconnected():
    G = nx.disjoint_union(nx.barabasi_albert_graph(200, 2, seed=1), nx.cycle_graph(9))
    G.add_nodes_from([1000, 1001])
    return G


def _clique_with_tail():
    G = nx.complete_graph(40)
    nx.add_path(G, [0] + list(range(40, 240)))
    return G


def _directed_hubs():
    """A random digraph with one in-hub (1500 arcs into node 0) and another out-hub (1500 arcs out of node 1): the
    transposed CSR has its own hub list."""
    G = nx.gnm_random_graph(2000, 8000, seed=12, directed=True)
    G.add_edges_from((v, 0) for v in range(2, 1502))
    G.add_edges_from((1, v) for v in range(500, 2000))
    return G


GRAPHS = {
    'karate': nx.karate_club_graph,
    'er300': lambda: nx.gnm_random_graph(300, 1200, seed=1),
    'ba2000': lambda: nx.barabasi_albert_graph(2000, 5, seed=3),
    'star': lambda: nx.star_graph(1500),
    'path600': lambda: nx.path_graph(600),
    'grid40': lambda: nx.grid_2d_graph(40, 40),
    'disconnected': _disconnected,
    'strings': lambda: nx.relabel_nodes(nx.karate_club_graph(), lambda v: f'node-{v:02d}'),
    'n1': lambda: nx.empty_graph(1),
    'n2': lambda: nx.path_graph(2),
    'n3': lambda: nx.path_graph(3),
    'empty5': lambda: nx.empty_graph(5),
    'clique_tail': _clique_with_tail,
}


@pytest.mark.parametrize('key', list(GRAPHS))
def test_matches_networkx(key):
    from graphrole_amd import core_number, onion_layers
    G = GRAPHS[key]()
    core, onion = core_number(G), onion_layers(G)
    assert core.name == 'core_number' and core.dtype == np.int64 and list(core.index) == sorted(G)
    assert onion.name == 'onion_layer' and onion.dtype == np.int64 and list(onion.index) == sorted(G)
    assert core.to_dict() == nx.core_number(G)
    assert onion.to_dict() == nx.onion_layers(G)


def test_the_graph_kinds_are_what_they_are_here_for():
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    for key in ('star', 'ba2000'):
        assert NetworkxInterface(GRAPHS[key]())._structure_csrs()[0].n_hubs > 0, key
    assert len(set(nx.core_number(GRAPHS['er300']()).values())) == 4
    assert max(nx.onion_layers(GRAPHS['er300']()).values()) == 15
    assert max(nx.onion_layers(GRAPHS['ba2000']()).values()) == 27
    assert max(nx.onion_layers(GRAPHS['path600']()).values()) == 300
    assert max(nx.onion_layers(GRAPHS['grid40']()).values()) == 39
    assert sorted(set(nx.core_number(_clique_with_tail()).values())) == [1, 39]
    assert nx.onion_layers(GRAPHS['empty5']()) == {v: 1 for v in range(5)}


@pytest.mark.parametrize('make', [lambda: nx.gnm_random_graph(300, 1200, seed=7, directed=True), _directed_hubs],
                         ids=['gnm300', 'hubs'])
def test_directed_matches_networkx(make):
    from graphrole_amd import core_number
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    D = make()
    assert any(D.has_edge(v, u) for u, v in D.edges())          # reciprocal arcs: they count twice
    if make is _directed_hubs:
        s_out, s_in = NetworkxInterface(D)._structure_csrs()
        assert s_out.n_hubs > 0 and s_in.n_hubs > 0
    core = core_number(D)
    assert core.dtype == np.int64 and list(core.index) == sorted(D)
    assert core.to_dict() == nx.core_number(D)


def test_directed_onion_layers_and_loops_raise_before_any_device_work(monkeypatch):
    from graphrole_amd import core_number, kernels as K, node_measures, onion_layers
    from graphrole_amd.graph.interface.networkx import NetworkxInterface

    def no_device(*args, **kwargs):
        raise AssertionError('device work for a refused graph')

    monkeypatch.setattr(K, 'core_numbers', no_device)
    monkeypatch.setattr(NetworkxInterface, '_device_graph', no_device)
    D = nx.gnm_random_graph(30, 90, seed=2, directed=True)
    L = nx.karate_club_graph()
    L.add_edge(3, 3)
    M = nx.MultiGraph([(0, 1), (0, 1), (1, 2)])
    for call, word in ((lambda: onion_layers(D), 'directed'), (lambda: node_measures(D, ['onion_layer']), 'directed'),
                       (lambda: core_number(L), 'selfloop_edges'), (lambda: onion_layers(L), 'selfloop_edges'),
                       (lambda: core_number(M), 'multigraph'), (lambda: onion_layers(M), 'multigraph')):
        with pytest.raises(NotImplementedError, match=word):
            call()


def test_relabelled_copy_and_second_run_give_the_same_result():
    from graphrole_amd import node_measures
    G = nx.barabasi_albert_graph(2000, 5, seed=3)
    names = ['core_number', 'onion_layer']
    a = node_measures(G, names)
    b = node_measures(G, names)
    assert a.to_numpy().tobytes() == b.to_numpy().tobytes()
    shuffled = np.random.default_rng(5).permutation(2000)
    H = nx.relabel_nodes(G, {v: int(shuffled[v]) for v in G})   # other ids: other rows, lists and hub blocks
    c = node_measures(H, names)
    back = c.loc[[int(shuffled[v]) for v in a.index]]
    assert back.to_numpy().tobytes() == a.to_numpy().tobytes()
    assert a['core_number'].to_dict() == nx.core_number(G) and a['onion_layer'].to_dict() == nx.onion_layers(G)


def _kernel_run(graph, want_onion=True):
    from graphrole_amd import kernels as K
    s_out, s_in = graph._structure_csrs()
    n = s_out.n
    core, onion, n_rounds = K.core_numbers(s_out, s_in if graph.directed else None, want_onion=want_onion)
    host = [None if t is None else K.to_host(t)[:n].copy() for t in (core, onion)]

    def arrays(csr):
        return K.to_host(csr.row_ptr).astype(np.int64), K.to_host(csr.col)[:csr.nnz].astype(np.int64)

    return host, n_rounds, arrays(s_out) + (arrays(s_in) if graph.directed else (None, None))


@pytest.mark.parametrize('key', ['ba2000', 'star', 'path600', 'clique_tail', 'directed_hubs'])
def test_kernel_equals_oracle_on_the_same_csrs(key):
    from graphrole_amd.graph.interface.networkx import NetworkxInterface
    G = _directed_hubs() if key == 'directed_hubs' else GRAPHS[key]()
    (core, onion), n_rounds, csrs = _kernel_run(NetworkxInterface(G))
    want = ko.core_numbers(*csrs)
    assert core.dtype == np.int64 and onion.dtype == np.int64
    assert np.array_equal(core, want.core) and np.array_equal(onion, want.onion)
    assert n_rounds == want.n_rounds == int(onion.max())
    (core2, onion2), n2, _ = _kernel_run(NetworkxInterface(G), want_onion=False)
    assert onion2 is None and n2 == n_rounds
    assert core2.tobytes() == core.tobytes()


def test_full_size_ba_1m_equals_oracle():
    """BA 1 M / 10 M (the BASELINE graph, 130 rounds) against tests/kcore_oracle.py on the same CSR; the oracle takes a
    few seconds there (every round is a handful of whole-array numpy calls), networkx would take minutes."""
    from graphrole_amd import synth
    from graphrole_amd.measures import _adapter
    (core, onion), n_rounds, csrs = _kernel_run(_adapter(synth.ba_graph(1_000_000, 10, seed=0)))
    want = ko.core_numbers(*csrs)
    assert np.array_equal(core, want.core) and np.array_equal(onion, want.onion)
    assert n_rounds == want.n_rounds == int(onion.max())


def test_karate_end_to_end_sense_making():
    from graphrole_amd import RecursiveFeatureExtractor, RoleExtractor, node_measures
    G = nx.karate_club_graph()
    features = RecursiveFeatureExtractor(G).extract_features()
    np.random.seed(0)
    role_extractor = RoleExtractor(n_roles=3)
    role_extractor.extract_role_factors(features)
    M = node_measures(G, ['degree', 'core_number', 'onion_layer'])
    assert list(M.columns) == ['degree', 'core_number', 'onion_layer']
    assert M['core_number'].to_dict() == nx.core_number(G) and M['onion_layer'].to_dict() == nx.onion_layers(G)
    E = role_extractor.sense_making(M)
    assert E.shape == (3, 3) and list(E.columns) == list(M.columns)
    assert np.all(E.to_numpy() >= 0)
