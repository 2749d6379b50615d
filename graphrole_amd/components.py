"""
Connected, weakly connected and strongly connected components on the GPU, the reachability sets and the bow-tie
position they induce: what ``nx.connected_components``, ``nx.weakly_connected_components``,
``nx.strongly_connected_components``, ``nx.descendants`` and ``nx.ancestors`` of networkx 3.4.2 find with sequential
searches, computed by csrc/grx_components.hip on the device CSR the feature extractor uses -- a lock-free union-find
for the connected and the weak components, trim / colour / close rounds for the strong ones, a level-synchronous
closure for reachability.

Real graphs are never connected: ``eccentricity``, ``diameter``, ``radius``, ``center`` and ``periphery`` raise on a
graph that is not (strongly) connected, and the betweenness, truss and graphlet columns of a fragment mean something
else than those of the giant component.  ``largest_component(G)`` is what to pass to ``G.subgraph(...)`` first, and
``component_table(G)['component_size']`` and ``bow_tie(G)`` are columns ``RoleExtractor.sense_making`` can explain roles
by (``M['component_size'] = component_table(G)['component_size']``); they are not catalogue entries of
``node_measures``.

Everything is indexed like ``node_measures``: by the sorted node labels.  Multigraph edges count once and self-loops
change nothing, as in networkx.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import pandas as pd

from graphrole_amd.measures import _adapter, _label_index, _rows_of, _structure_pair

BOW_TIE_CATEGORIES = ['core', 'in', 'out', 'tube', 'tendril', 'other']

_NX_NAME = {'connected': 'connected_components', 'weak': 'weakly_connected_components',
            'strong': 'strongly_connected_components'}


def _checked_adapter(G, kind: Optional[str], what: str):
    """The adapter of G and the component kind, after networkx's own refusals: the undirected functions are not
    implemented for a directed graph, the weak / strong ones not for an undirected graph."""
    graph = _adapter(G)
    if kind is None:
        kind = 'weak' if graph.directed else 'connected'
    if kind not in _NX_NAME:
        raise ValueError(f"kind must be 'connected', 'weak', 'strong' or None, got {kind!r}")
    if kind == 'connected' and graph.directed:
        raise NotImplementedError(f'networkx does not implement nx.{what}(G) for a directed graph; use the weakly or '
                                  f'strongly connected form, or pass G.to_undirected()')
    if kind != 'connected' and not graph.directed:
        raise NotImplementedError(f'networkx does not implement nx.{what}(G) for an undirected graph; use the '
                                  f'connected form, or pass G.to_directed()')
    return graph, kind


def _table_adapter(G, kind: Optional[str]):
    """``_checked_adapter`` for the functions that take `kind`: the kind is resolved first (None = connected for an
    undirected graph, weak for a directed one), then the refusals name the networkx function of that kind."""
    if kind is None:
        kind = 'weak' if _adapter(G).directed else 'connected'
    if kind not in _NX_NAME:
        raise ValueError(f"kind must be 'connected', 'weak', 'strong' or None, got {kind!r}")
    return _checked_adapter(G, kind, _NX_NAME[kind])


def _n_nodes(graph) -> int:
    return len(list(graph.get_nodes()))


def _component_columns(graph, kind: str, what: str):
    """(name int64[n], size int64[n], n_components, rounds) in label order; `name` is an arbitrary id per component
    (the kernel's label: the smallest INTERNAL row)."""
    if _n_nodes(graph) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 0, 0
    K = graph._K()
    host = graph._device_graph()[0]
    if kind == 'strong':
        s_out, s_in = _structure_pair(graph, what)
    else:
        s_out, s_in = graph._structure_csrs()[0], None
    label, size, n_components, rounds = K.components(s_out, s_in, mode=kind)
    name = host.to_label_order(np.asarray(K.to_host(label))[:host.n]).astype(np.int64)
    size = host.to_label_order(np.asarray(K.to_host(size))[:host.n]).astype(np.int64)
    return name, size, n_components, rounds


def _groups(name: np.ndarray):
    """(first int64[c], members: list of int64 arrays) of the classes of `name`, ordered by their first member."""
    if not len(name):
        return np.zeros(0, dtype=np.int64), []
    order = np.argsort(name, kind='stable')
    cuts = np.nonzero(np.diff(name[order]))[0] + 1
    members = np.split(order, cuts)                              # ascending rows inside a class (stable sort)
    first = np.array([m[0] for m in members], dtype=np.int64)
    by_first = np.argsort(first, kind='stable')
    return first[by_first], [members[i] for i in by_first]


def _label_sets(graph, members) -> list:
    labels = graph.to_csr().labels
    if isinstance(labels, range) and labels == range(len(labels)):
        return [set(m.tolist()) for m in members]
    return [{labels[i] for i in m.tolist()} for m in members]


def _component_list(G, kind: str) -> list:
    what = _NX_NAME[kind]
    graph, kind = _checked_adapter(G, kind, what)
    name, _, n_components, _ = _component_columns(graph, kind, what)
    _, members = _groups(name)
    assert len(members) == n_components
    return _label_sets(graph, members)


def connected_components(G) -> list:
    """
    The connected components of an undirected graph as ``list(nx.connected_components(G))``: a list of node-label sets,
    from the union-find of csrc/grx_components.hip.

    :param G: any undirected graph ``node_measures`` accepts; multigraph edges count once, self-loops change nothing
    :return: list of sets, ordered by each component's first member in the index (the sorted node labels).  Stated
      divergence: networkx yields the same sets in the graph's node order
    :raises NotImplementedError: G is directed (as networkx)
    """
    return _component_list(G, 'connected')


def weakly_connected_components(G) -> list:
    """
    The weakly connected components of a directed graph as ``list(nx.weakly_connected_components(G))``, from the
    union-find of csrc/grx_components.hip over the out-arcs alone (no in-adjacency needed).

    :return: list of sets, ordered by each component's first member in the index; networkx yields in the graph's node
      order (the stated divergence)
    :raises NotImplementedError: G is undirected (as networkx)
    """
    return _component_list(G, 'weak')


def strongly_connected_components(G) -> list:
    """
    The strongly connected components of a directed graph as ``list(nx.strongly_connected_components(G))``, by the trim
    / colour / close rounds of csrc/grx_components.hip (Orzan 2004; Barnat et al. 2011).

    :return: list of sets, ordered by each component's first member in the index; networkx yields in the reverse
      topological order its search finds them in (the stated divergence)
    :raises NotImplementedError: G is undirected (as networkx), or its adapter has no in-adjacency
    """
    return _component_list(G, 'strong')


def _count(G, kind: str, what: str) -> int:
    graph, kind = _checked_adapter(G, kind, what)
    return int(_component_columns(graph, kind, what)[2])


def number_connected_components(G) -> int:
    """``nx.number_connected_components(G)``; refusals as ``connected_components``."""
    return _count(G, 'connected', 'number_connected_components')


def number_weakly_connected_components(G) -> int:
    """``nx.number_weakly_connected_components(G)``; refusals as ``weakly_connected_components``."""
    return _count(G, 'weak', 'number_weakly_connected_components')


def number_strongly_connected_components(G) -> int:
    """``nx.number_strongly_connected_components(G)``; refusals as ``strongly_connected_components``."""
    return _count(G, 'strong', 'number_strongly_connected_components')


def _is_one(G, kind: str, what: str) -> bool:
    graph, kind = _checked_adapter(G, kind, what)
    if _n_nodes(graph) == 0:
        import networkx as nx
        raise nx.NetworkXPointlessConcept('Connectivity is undefined for the null graph.')
    return int(_component_columns(graph, kind, what)[2]) == 1


def is_connected(G) -> bool:
    """``nx.is_connected(G)``.

    :raises networkx.NetworkXPointlessConcept: the null graph (networkx's message)
    :raises NotImplementedError: G is directed (as networkx)
    """
    return _is_one(G, 'connected', 'is_connected')


def is_weakly_connected(G) -> bool:
    """``nx.is_weakly_connected(G)``; the null graph and an undirected graph are refused as networkx refuses them."""
    return _is_one(G, 'weak', 'is_weakly_connected')


def is_strongly_connected(G) -> bool:
    """``nx.is_strongly_connected(G)``; the null graph and an undirected graph are refused as networkx refuses them."""
    return _is_one(G, 'strong', 'is_strongly_connected')


def _ranked(name: np.ndarray, size: np.ndarray):
    """(component int64[n] = rank of the node's component by decreasing size, ties by first member; members of rank 0)."""
    first, members = _groups(name)
    if not len(first):
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    sizes = size[first]
    by_rank = np.lexsort((first, -sizes))
    component = np.empty(len(name), dtype=np.int64)
    for rank, i in enumerate(by_rank.tolist()):
        component[members[i]] = rank
    return component, members[by_rank[0]]


def component_table(G, kind: Optional[str] = None) -> pd.DataFrame:
    """
    The array-native form: the component of every node and its size.

    :param G: any graph ``node_measures`` accepts
    :param kind: ``'connected'``, ``'weak'`` or ``'strong'``; None = connected for an undirected graph, weak for a
      directed one
    :return: int64 frame indexed by the sorted node labels with the columns ``component`` -- the rank of the node's
      component by decreasing size, ties by first member in the index, so 0 is the giant component -- and
      ``component_size``; ``.attrs['n_components']`` and ``.attrs['rounds']`` (the rounds of the strong method, else 0)
    :raises NotImplementedError: a kind networkx does not define for this graph (connected on a directed graph, weak
      or strong on an undirected one); strong on an adapter without in-adjacency
    """
    graph, kind = _table_adapter(G, kind)
    name, size, n_components, rounds = _component_columns(graph, kind, _NX_NAME[kind])
    component, _ = _ranked(name, size)
    frame = pd.DataFrame({'component': component, 'component_size': size},
                         index=_index(graph, len(name)), columns=['component', 'component_size'])
    frame.attrs['n_components'] = int(n_components)
    frame.attrs['rounds'] = int(rounds)
    return frame


def _index(graph, n: int) -> pd.Index:
    return _label_index(graph) if n else pd.Index([])


def largest_component(G, kind: Optional[str] = None) -> pd.Index:
    """
    The labels of component 0 of ``component_table(G, kind)`` -- the largest component, ties by first member in the
    index -- as a ``pd.Index`` in index order: what to pass to ``G.subgraph(...)`` before ``eccentricity``.
    """
    graph, kind = _table_adapter(G, kind)
    name, size, _, _ = _component_columns(graph, kind, _NX_NAME[kind])
    _, rows = _ranked(name, size)
    return _index(graph, len(name))[rows]


# ------------------------------------------------------------------------------------------------- reachability
def _closure(graph, K, csr, member: np.ndarray) -> np.ndarray:
    """bool[n] in label order: the rows reachable from the label-order set `member` along csr's arcs, members included."""
    host = graph._device_graph()[0]
    flag, _, _ = K.reachable(csr, host.to_internal(member.astype(np.int32)))
    return host.to_label_order(np.asarray(K.to_host(flag))[:host.n]) != 0


def _reach_from(G, source, what: str, backward: bool) -> set:
    import networkx as nx
    graph = _adapter(G)
    try:
        known = source in set(graph.get_nodes())
    except TypeError:
        known = False
    if not known:
        raise nx.NetworkXError(f"The node {source} is not in the {'digraph' if graph.directed else 'graph'}.")
    if graph.directed and backward:
        csr = _structure_pair(graph, what)[1]
    else:
        csr = graph._structure_csrs()[0]
    n = _n_nodes(graph)
    member = np.zeros(n, dtype=bool)
    row = int(_rows_of(graph, [source])[0])
    member[row] = True
    reached = _closure(graph, graph._K(), csr, member)
    reached[row] = False
    return _label_sets(graph, [np.nonzero(reached)[0]])[0]


def descendants(G, source) -> set:
    """
    ``nx.descendants(G, source)``: the nodes reachable from `source` along the arcs, without `source`, by the
    level-synchronous closure of csrc/grx_components.hip.  An undirected graph gives the rest of the component.

    :raises networkx.NetworkXError: `source` is not a node
    """
    return _reach_from(G, source, 'descendants', backward=False)


def ancestors(G, source) -> set:
    """
    ``nx.ancestors(G, source)``: the nodes from which `source` is reachable, without `source` (the closure over the
    in-adjacency).  An undirected graph gives the rest of the component.

    :raises networkx.NetworkXError: `source` is not a node
    :raises NotImplementedError: G is directed and its adapter has no in-adjacency
    """
    return _reach_from(G, source, 'ancestors', backward=True)


def bow_tie(G) -> pd.Series:
    """
    The bow-tie position of every node of a directed graph (Broder et al., "Graph structure in the web", 2000).  With S
    the largest strongly connected component (ties broken by first member in the index):

    * ``core``: in S;  ``in``: reaches S, not in S;  ``out``: reached from S, not in S;
    * ``tube``: reached from ``in`` and reaches ``out``, and none of the above;
    * ``tendril``: exactly one of those two, and none of the above;  ``other``: the rest.

    One strong-components call and four closures (ancestors and descendants of S, descendants of ``in``, ancestors of
    ``out``) of csrc/grx_components.hip.  There is no networkx function to restate; the definition above written with
    ``nx.descendants`` / ``nx.ancestors`` is the authority.

    :return: categorical Series named ``bow_tie`` indexed by the sorted node labels, categories ``['core', 'in',
      'out', 'tube', 'tendril', 'other']``; ``.attrs['sizes']``: the count of every category
    :raises NotImplementedError: G is undirected; or its adapter has no in-adjacency
    """
    graph = _adapter(G)
    if not graph.directed:
        raise NotImplementedError('bow_tie is defined for a directed graph: the bow-tie position follows the strongly '
                                  'connected components, which networkx does not implement for an undirected graph; '
                                  'pass G.to_directed()')
    name, size, _, _ = _component_columns(graph, 'strong', 'bow_tie')
    n = len(name)
    code = np.full(n, 5, dtype=np.int8)
    if n:
        K = graph._K()
        s_out, s_in = _structure_pair(graph, 'bow_tie')
        _, rows = _ranked(name, size)
        core = np.zeros(n, dtype=bool)
        core[rows] = True
        inn = _closure(graph, K, s_in, core) & ~core
        out = _closure(graph, K, s_out, core) & ~core
        from_in = _closure(graph, K, s_out, inn)
        to_out = _closure(graph, K, s_in, out)
        rest = ~(core | inn | out)
        code[rest & (from_in ^ to_out)] = 4
        code[rest & from_in & to_out] = 3
        code[out], code[inn], code[core] = 2, 1, 0
    series = pd.Series(pd.Categorical.from_codes(code, categories=BOW_TIE_CATEGORIES), index=_index(graph, n),
                       name='bow_tie')
    counts = np.bincount(code, minlength=len(BOW_TIE_CATEGORIES))
    series.attrs['sizes'] = {c: int(k) for c, k in zip(BOW_TIE_CATEGORIES, counts)}
    return series
