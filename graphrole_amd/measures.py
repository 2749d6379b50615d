"""
Node measures for RolX sense making (Henderson et al., KDD 2012, section 4): the node x measure table M that
``RoleExtractor.sense_making`` explains by E >= 0 with G E ~ M.  Every measure restates networkx 3.4.2 with its
default arguments and is computed on the device CSR the feature extractor uses (graph/interface/base.py
``_device_graph``): degrees by grx_row_sums, clustering and effective size by grx_local_structure_measures on the
triangle counts of grx_triangle_counts, PageRank and eigenvector centrality by the power iterations of
csrc/grx_measures.hip, betweenness centrality (opt-in: O(n m)) by the batched Brandes passes of
csrc/grx_betweenness.hip, and closeness and harmonic centrality (opt-in: O(n m)) from the per-target distance sums of
the bitset multi-source BFS of csrc/grx_closeness.hip, the number of biconnected components of every node (opt-in;
more than one: an articulation point) by the Tarjan-Vishkin sweeps of csrc/grx_biconnected.hip, and the core number
and onion layer of every node (opt-in) by the synchronous peeling of csrc/grx_kcore.hip, and the eccentricity of every
node (opt-in) -- with it diameter, radius, center and periphery -- by the extremal passes of the same multi-source
BFS (grx_eccentricity in csrc/grx_closeness.hip), and Burt's constraint of every node (opt-in) -- with it the weighted
and directed form of effective size -- by the per-arc row intersections of csrc/grx_structural_holes.hip over the
mutual-weight CSR, the first measures here besides ``weighted_degree``, ``pagerank`` and ``eigenvector`` that read an
edge weight, and -- with ``node_measures(..., distance='weight')`` -- closeness, harmonic centrality and eccentricity
over shortest paths by edge weight, together with the distances themselves (``dijkstra_path_lengths``), by the batched
Bellman-Ford relaxation of csrc/grx_sssp.hip, whose fixed point is networkx's Dijkstra distance bit for bit, and --
with ``weighted_betweenness_centrality`` or ``node_measures(..., betweenness_weight='weight')`` -- betweenness
centrality over those shortest paths by csrc/grx_weighted_betweenness.hip: the same relaxation, the shortest-path DAG
read off its converged distances (arc u -> v is on a lightest path iff fl(D(u) + w) == D(v) and D(u) < D(v), networkx's
own test of equally short), and Brandes' two passes in the order of the depth in that DAG, with no priority queue,
and -- with ``clustering`` / ``average_clustering`` or ``node_measures(..., clustering_weight='weight')`` -- the
clustering coefficient of a directed graph (Fagiolo) and of a graph with weights (Onnela's geometric mean of the
normalised triangle weights), as networkx's ``clustering(G, nodes, weight)`` defines them, by
csrc/grx_clustering.hip: the cube root of every normalised weight once per arc, then the per-arc row intersections of
the structural-hole kernel over the all-neighbours CSR, and -- with ``square_clustering`` -- the square clustering
coefficient of an undirected graph (the density of 4-cycles, the one local density that says anything on a bipartite
graph), as networkx's ``square_clustering(G, nodes)`` defines it, by csrc/grx_square_clustering.hip: the two-hop
neighbours of every node counted in an LDS hash table (dense counters for the rows with more than 3 072 wedges), all
in integers until one division, and -- with ``neighbor_roles`` / ``role_mixing_matrix``, the tables behind
``RoleExtractor.neighbor_sense`` (the paper's NeighborSense: each role explained by the roles of its neighbours) -- the
node x role table N = op(A) P of the memberships of every node's neighbours by csrc/grx_neighbor_sense.hip: a gather
of one membership row per arc in a summation order fixed by the positions of the row's arcs, and -- with ``truss_number`` / ``node_truss_number`` / ``k_truss`` -- the truss number
of every edge and node of an undirected graph (the largest k with the edge or node in networkx's ``k_truss(G, k)``), by
the level-synchronous edge peeling of csrc/grx_truss.hip: a row intersection per edge for the triangle supports and
one more per edge as the edges leave, all in integers, and -- with ``graphlet_degree_vectors`` / ``graphlet_counts`` --
the graphlet degree vector of every node of a simple undirected graph (Przulj's orbits 0-14 of the graphs on 2, 3 and 4
nodes, induced; there is no networkx function to restate: the authority is brute-force enumeration), by
csrc/grx_graphlets.hip: non-induced counts from degrees, triangles per edge, the 4-cycles of the square-clustering
kernel and a 4-clique listing on the degree-oriented graph, then an integer back-substitution, and -- with
``edge_betweenness_centrality`` -- the betweenness of every edge, by hops or by weight, as networkx's
``edge_betweenness_centrality(G, k, normalized, weight, seed)`` defines it, by the two betweenness files with sigma kept
and one pass per batch over the arcs of the shortest-path DAGs (csrc/grx_edge_sum.h states the order of its sums), and
-- with ``triadic_census`` / ``node_triad_census`` -- the triad census of a directed graph (Holland and Leinhardt's 16
classes of three nodes with their arcs), for the graph as networkx's ``triadic_census(G, nodelist)`` and per node, by
csrc/grx_triads.hip: the closed triads by one row intersection per adjacent pair of the all-neighbours CSR with one
direction byte per arc slot, the open and the dyadic ones from neighbour classes, degrees and common neighbours.
"""
from __future__ import annotations

import copy
import math
import random
from numbers import Integral
from typing import List, Optional, Sequence

import numpy as np
import pandas as pd

from graphrole_amd._lib import ConvergenceError  # noqa: F401  (re-exported)

#: name -> networkx call it restates
CATALOGUE = {
    'degree': 'G.degree()',
    'weighted_degree': "G.degree(weight='weight')",
    'in_degree': 'G.in_degree()',
    'out_degree': 'G.out_degree()',
    'clustering': 'nx.clustering(G)',
    'effective_size': 'nx.effective_size(G)',
    'constraint': 'nx.constraint(G, weight=weight)',
    'pagerank': "nx.pagerank(G, alpha, weight='weight', tol=tol, max_iter=max_iter)",
    'eigenvector': "nx.eigenvector_centrality(G, max_iter=max_iter, tol=tol, weight='weight')",
    'betweenness_centrality': 'nx.betweenness_centrality(G, k=k, normalized=normalized, endpoints=endpoints, '
                              'seed=seed)',
    'closeness_centrality': 'nx.closeness_centrality(G, distance=distance, wf_improved=wf_improved)',
    'harmonic_centrality': 'nx.harmonic_centrality(G, distance=distance)',
    'biconnected_components': 'Counter(v for c in nx.biconnected_components(G) for v in c)',
    'core_number': 'nx.core_number(G)',
    'onion_layer': 'nx.onion_layers(G)',
    'eccentricity': 'nx.eccentricity(G)',                      # distance='weight': nx.eccentricity(G, weight='weight')
}

#: catalogue entries computed only when named: not in ``available_measures`` nor in the default table -- the
#: centralities and 'eccentricity' because they cost up to O(n m), 'biconnected_components', 'core_number',
#: 'onion_layer' (O(n + m)) and 'constraint' (a row intersection per arc) because the default table and
#: ``available_measures`` are pinned as they were before they existed
OPT_IN = ('betweenness_centrality', 'closeness_centrality', 'harmonic_centrality', 'biconnected_components',
          'core_number', 'onion_layer', 'eccentricity', 'constraint')


def _unavailable(name: str, directed: bool, multi: bool) -> Optional[str]:
    """Why `name` is not computed for this kind of graph (None = it is)."""
    kind = ('directed ' if directed else 'undirected ') + ('multigraph' if multi else 'graph')
    if name in ('in_degree', 'out_degree') and not directed:
        return f'{name} is defined for directed graphs only'
    if name in ('clustering', 'effective_size'):
        if multi and name == 'clustering':
            return f'networkx does not implement {CATALOGUE[name]} for a multigraph'
        if directed or multi:
            also = ('; clustering(G) of this package computes the directed form' if name == 'clustering' and not multi
                    else '')
            return (f'{name} of a {kind} is not computed here (only undirected graphs without parallel edges); '
                    f'use {CATALOGUE[name]} from networkx{also}')
    if name == 'constraint' and multi:
        return (f'{name} of a {kind} is not computed here (networkx adds key dictionaries there, not weights: its '
                f'result on a multigraph is not meaningful); merge the parallel edges first')
    if name == 'eigenvector' and multi:
        return f'networkx does not implement {CATALOGUE[name]} for a multigraph'
    if name == 'biconnected_components' and directed:
        return f'networkx does not implement nx.biconnected_components(G) for a {kind}'
    if name in ('core_number', 'onion_layer') and multi:
        return f'networkx does not implement {CATALOGUE[name]} for a multigraph'
    if name == 'onion_layer' and directed:
        return f'networkx does not implement nx.onion_layers(G) for a {kind}'
    return None


def available_measures(directed: bool, multi: bool) -> List[str]:
    """The catalogue entries defined for a graph of this kind, in catalogue order (the opt-in ones excepted)."""
    return [name for name in CATALOGUE if name not in OPT_IN and _unavailable(name, directed, multi) is None]


def _adapter(G):
    from graphrole_amd.graph import interface
    cls = interface.get_interface(G)
    if cls is None:
        raise TypeError(f'Input graph G must be from one of the following supported libraries: '
                        f'{interface.get_supported_graph_libraries()}')
    return cls(G)


def _count_csrs(graph, K, host):
    """Multigraph: device CSRs whose weights are the edge multiplicities (out, and in when directed) -- the degree
    counts of networkx's G.degree() count parallel edges."""
    if getattr(graph, '_count_pair', None) is None:
        from graphrole_amd.graph.csr import CSRGraph, InternalGraph
        g = graph.to_csr()
        src, dst, mult = graph._multiplicity
        counts = InternalGraph(CSRGraph(g.n, src, dst, mult, graph.directed, labels=g.labels, validate=False))
        assert np.array_equal(counts.perm, host.perm)
        out = K.DeviceCSR(counts.row_ptr, counts.col, counts.w)
        tr = K.DeviceCSR(counts.t_row_ptr, counts.t_col, counts.t_w) if graph.directed else None
        graph._count_pair = (out, tr)
    return graph._count_pair


def node_measures(G, measures: Optional[Sequence[str]] = None, *, alpha: float = 0.85, tol: float = 1e-6,
                  max_iter: int = 100, k: Optional[int] = None, seed=None, normalized: bool = True,
                  endpoints: bool = False, wf_improved: bool = True, weight=None,
                  distance=None, betweenness_weight=None, clustering_weight=None) -> pd.DataFrame:
    """
    Node x measure table of well-known graph measures, computed on the GPU.

    :param G: any graph ``RecursiveFeatureExtractor`` accepts (networkx graph or multigraph, CSRGraph, igraph)
    :param measures: names from ``CATALOGUE`` in the order of the columns; None = every measure defined for the
      graph's kind (``available_measures``; ``OPT_IN`` measures such as ``'betweenness_centrality'`` only when named)
    :param alpha, tol, max_iter: networkx's arguments of pagerank (alpha, tol, max_iter) and eigenvector_centrality
      (tol, max_iter)
    :param k, seed, normalized, endpoints: networkx's arguments of betweenness_centrality (see
      ``betweenness_centrality``); they apply to ``'betweenness_centrality'`` only
    :param wf_improved: networkx's argument of closeness_centrality; it applies to ``'closeness_centrality'`` only.
      ``'closeness_centrality'`` and ``'harmonic_centrality'`` named together share one multi-source BFS pass
    :param weight: networkx's argument of constraint: None or ``'weight'`` (see ``constraint``); it applies to
      ``'constraint'`` only
    :param distance: None = the distance columns count hops; ``'weight'`` = ``'closeness_centrality'``,
      ``'harmonic_centrality'`` and ``'eccentricity'`` measure shortest paths by the edge attribute ``'weight'`` (a
      missing attribute counts 1), as networkx's ``distance='weight'`` resp. ``weight='weight'``: all three come from
      one pass of grx_weighted_distances with every node a source, and ``'eccentricity'`` is then a float64 column.
      It applies to these three columns only
    :param betweenness_weight: None = ``'betweenness_centrality'`` counts hops; ``'weight'`` = the column is
      ``weighted_betweenness_centrality`` (shortest paths by the edge attribute ``'weight'``, a missing attribute counts
      1) with the same `k`, `seed`, `normalized` and `endpoints`; ``.attrs['weighted_betweenness']`` then holds its
      ``rounds`` and ``levels``.  It applies to that column only
    :param clustering_weight: None = ``'clustering'`` is the coefficient of an undirected graph without weights, as it
      always was; ``'weight'`` = the column is ``clustering(G, weight='weight')``: the weighted form, of an undirected or
      of a directed graph (a missing attribute counts 1).  It applies to that column only
    :return: DataFrame indexed by the sorted node labels (the index of ``extract_features()``);
      ``.attrs['iterations']`` holds the power-iteration counts
    :raises ValueError: an unknown measure name; ``distance='weight'`` with a negative, NaN or infinite edge weight;
      ``betweenness_weight='weight'`` with a weight that is not finite and > 0; ``clustering_weight='weight'`` with a
      negative or non-finite weight, or with weights that are all zero
    :raises NotImplementedError: a measure that networkx does not implement for this kind of graph (among them
      ``'biconnected_components'`` and ``'onion_layer'`` of a directed graph, and ``'core_number'`` and
      ``'onion_layer'`` of a multigraph or of a graph with a self-loop), or that is outside this implementation's scope
      (directed / multigraph clustering and effective size -- ``effective_size(G)`` and ``clustering(G)`` compute the
      directed and the weighted forms, and ``clustering_weight='weight'`` brings the latter into this table --,
      ``'constraint'`` of a multigraph, weighted distances of a multigraph or of a graph with
      parallel edges, a `distance`, `betweenness_weight` or `clustering_weight` other than None and ``'weight'``)
    :raises ConvergenceError: PageRank or eigenvector centrality did not converge within max_iter iterations
    :raises networkx.NetworkXError: ``'eccentricity'`` of a graph that is not (strongly) connected, as networkx

    Stated divergence: ``effective_size`` of a node whose only neighbour is itself is NaN (networkx raises
    ZeroDivisionError).
    """
    return measures_of(_adapter(G), measures, alpha=alpha, tol=tol, max_iter=max_iter, k=k, seed=seed,
                       normalized=normalized, endpoints=endpoints, wf_improved=wf_improved, weight=weight,
                       distance=distance, betweenness_weight=betweenness_weight, clustering_weight=clustering_weight)


def measures_of(graph, measures: Optional[Sequence[str]] = None, *, alpha: float = 0.85, tol: float = 1e-6,
                max_iter: int = 100, k: Optional[int] = None, seed=None, normalized: bool = True,
                endpoints: bool = False, wf_improved: bool = True, weight=None, distance=None,
                betweenness_weight=None, clustering_weight=None) -> pd.DataFrame:
    """``node_measures`` on an existing graph adapter (its device CSR is built once and reused)."""
    directed = bool(graph.directed)
    multi = bool(getattr(graph, '_multi', False))
    if measures is None:
        names = available_measures(directed, multi)
    else:
        names = [measures] if isinstance(measures, str) else list(measures)
        unknown = [nm for nm in names if nm not in CATALOGUE]
        if unknown:
            raise ValueError(f'unknown measure(s) {unknown}; the catalogue is {list(CATALOGUE)}')
    # the weighted clustering column is defined for directed graphs too: its own refusals stand in for _unavailable
    by_weight_cl = 'clustering' in names and _weight_flag('clustering', clustering_weight)
    if measures is not None:
        for nm in names:
            why = None if (nm == 'clustering' and by_weight_cl) else _unavailable(nm, directed, multi)
            if why is not None:
                raise NotImplementedError(why)
    if by_weight_cl:
        _clustering_refusals(graph, True)                     # argument errors before any device work
    by_weight_bc = False
    if 'betweenness_centrality' in names:
        sources = _betweenness_sources(graph, k, seed)        # argument errors before any device work
        if _weight_flag('betweenness_centrality', betweenness_weight):
            _weighted_betweenness_refusals(graph, "node_measures(G, ..., betweenness_weight='weight')")
            by_weight_bc = True
    peeled = [nm for nm in names if nm in ('core_number', 'onion_layer')]
    if peeled:
        _peeling_refusals(graph, peeled[0])                   # likewise: read from the host CSR
    if 'constraint' in names:
        weighted = _weight_flag('constraint', weight)
        _structural_hole_refusals(graph, 'constraint', weighted)
    by_weight = _distance_flag(distance) and any(nm in _DISTANCE_COLUMNS for nm in names)
    if by_weight:
        _weighted_distance_refusals(graph, "node_measures(G, ..., distance='weight')")
    K = graph._K()
    host, out, tr = graph._device_graph()
    loops = bool(graph._has_loops)
    integral = bool(host.integral)
    cols, dtypes, cache, iterations = [], [], {}, {}

    def counts(which):
        # neighbour counts with parallel edges counted (networkx degree without weight)
        if multi:
            c_out, c_tr = _count_csrs(graph, K, host)
            csr = c_out if which == 'out' else c_tr
            return K.row_sums(csr, which == 'out' and not directed)
        csr = out if which == 'out' else tr
        return K.row_counts(csr, which == 'out' and not directed and loops)

    def local():
        if 'local' not in cache:
            cache['local'] = K.local_structure(out, K.triangle_counts(out), loops)
        return cache['local']

    def distances():
        # every node a source, walking the out-arcs: one pass for closeness and harmonic centrality
        if 'distances' not in cache:
            cache['distances'] = _distance_sums(graph, K, np.arange(host.n, dtype=np.int64), reverse=False)
        return cache['distances']

    def weighted_distances():
        # every node a source, walking the out-arcs by weight: one pass for the three distance columns
        if 'weighted_distances' not in cache:
            cache['weighted_distances'] = K.weighted_distances(_weighted_pull(graph, 'weighted distances'),
                                                               np.arange(host.n, dtype=np.int64))
        return cache['weighted_distances']

    def blocks():
        # the undirected graph's distinct arcs: parallel edges count once
        if 'blocks' not in cache:
            cache['blocks'] = K.biconnected(graph._structure_csrs()[0])
        return cache['blocks']

    def peeling():
        # one kernel call for both columns; the distinct arcs, out and (directed) in
        if 'peeling' not in cache:
            s_out, s_in = _structure_pair(graph, 'core_number')
            cache['peeling'] = K.core_numbers(s_out, s_in if directed else None, 'onion_layer' in names)
        return cache['peeling']

    for nm in names:
        if nm == 'degree':
            col = counts('out') if not directed else K.add_columns(counts('out'), counts('in'))
            dt = np.dtype('int64')
        elif nm == 'weighted_degree':
            col = (K.row_sums(out, loops) if not directed
                   else K.add_columns(K.row_sums(out, False), K.row_sums(tr, False)))
            dt = np.dtype('int64') if integral else np.dtype('float64')
        elif nm == 'in_degree':
            col, dt = counts('in'), np.dtype('int64')
        elif nm == 'out_degree':
            col, dt = counts('out'), np.dtype('int64')
        elif nm == 'clustering' and by_weight_cl:
            if 'weighted_clustering' not in cache:
                cache['weighted_clustering'] = _clustering_column(graph, K, True)
            col, dt = cache['weighted_clustering'], np.dtype('float64')
        elif nm == 'clustering':
            col, dt = local()[0], np.dtype('float64')
        elif nm == 'effective_size':
            col, dt = local()[1], np.dtype('float64')
        elif nm == 'constraint':
            if 'constraint' not in cache:
                cache['constraint'] = _structural_holes(graph, K, weighted, True, False)[0]
            col, dt = cache['constraint'], np.dtype('float64')
        elif nm == 'betweenness_centrality' and by_weight_bc:
            if 'weighted_betweenness' not in cache:
                # shortest paths by weight: the weighted CSRs, out for the backward pass and (directed) in for the
                # relaxation and the forward pass
                if directed:
                    _weighted_pull(graph, 'weighted betweenness centrality')
                cache['weighted_betweenness'] = K.weighted_betweenness(
                    out, tr if directed else None, np.asarray(host.inv)[sources], endpoints,
                    _rescale_factor(host.n, normalized, directed, k, endpoints))
            col, dt = cache['weighted_betweenness'][0], np.dtype('float64')
        elif nm == 'betweenness_centrality':
            # BFS walks G[v]: the distinct arcs, out and (directed) in, not a neighbour multiset
            s_out, s_in = _structure_pair(graph, 'betweenness_centrality')
            col = K.betweenness(s_out, s_in if directed else None, np.asarray(host.inv)[sources], endpoints,
                                _rescale_factor(host.n, normalized, directed, k, endpoints))
            dt = np.dtype('float64')
        elif nm == 'closeness_centrality' and by_weight:
            reach, dsum = weighted_distances()[:2]
            col = K.to_device(_closeness_by_weight(K.to_host(reach)[:host.n], K.to_host(dsum)[:host.n], host.n,
                                                   wf_improved))
            dt = np.dtype('float64')
        elif nm == 'harmonic_centrality' and by_weight:
            col, dt = weighted_distances()[2], np.dtype('float64')
        elif nm == 'eccentricity' and by_weight:
            reach, source_ecc = weighted_distances()[0], weighted_distances()[4]
            _require_full_reach(K, reach, np.arange(host.n, dtype=np.int64), host.n, directed)
            col, dt = source_ecc, np.dtype('float64')           # source b is row b: nothing to scatter
        elif nm == 'closeness_centrality':
            reach, dsum, _ = distances()
            col = K.to_device(_closeness(K.to_host(reach)[:host.n], K.to_host(dsum)[:host.n], host.n, wf_improved))
            dt = np.dtype('float64')
        elif nm == 'harmonic_centrality':
            col, dt = distances()[2], np.dtype('float64')
        elif nm == 'biconnected_components':
            col, dt = blocks()[0], np.dtype('int64')
        elif nm == 'core_number':
            col, dt = peeling()[0], np.dtype('int64')
        elif nm == 'onion_layer':
            col, dt = peeling()[1], np.dtype('int64')
        elif nm == 'eccentricity':
            if 'eccentricity' not in cache:                   # its own kernel: not one of the sums of distances()
                cache['eccentricity'] = _eccentricity_column(graph, K, 'all')[0]
            col, dt = cache['eccentricity'], np.dtype('int64')
        elif nm == 'pagerank':
            col, iterations[nm] = K.pagerank(tr if directed else out, K.row_sums(out, False), alpha, tol, max_iter)
            dt = np.dtype('float64')
        else:
            col, iterations[nm] = K.eigenvector_centrality(tr if directed else out, tol, max_iter)
            dt = np.dtype('float64')
        cols.append(col)
        dtypes.append(dt)
    frame = graph._frame(names, cols, dtypes)
    frame.attrs['iterations'] = iterations
    if 'weighted_betweenness' in cache:
        frame.attrs['weighted_betweenness'] = dict(rounds=cache['weighted_betweenness'][1],
                                                   levels=cache['weighted_betweenness'][2])
    return frame


def _structure_pair(graph, what: str):
    """``graph._structure_csrs()``: (out CSR, in CSR) of the distinct arcs; refuses a directed graph whose adapter has
    no in-adjacency, naming the measure `what`."""
    s_out, s_in = graph._structure_csrs()
    if graph.directed and s_in is None:
        raise NotImplementedError(f'{type(graph).__name__} has no in-adjacency for this directed graph; '
                                  f'{what} cannot be computed on it')
    return s_out, s_in


def _py_random_state(seed) -> random.Random:
    """networkx's @py_random_state for int, None and random.Random seeds (None = the global state of `random`)."""
    if seed is None:
        return random._inst
    if isinstance(seed, random.Random):
        return seed
    if isinstance(seed, Integral):
        return random.Random(seed)
    raise TypeError(f'seed must be an int, None or a random.Random instance (got {type(seed).__name__}); '
                    f'networkx also accepts numpy random states, this implementation does not')


def _betweenness_sources(graph, k: Optional[int], seed) -> np.ndarray:
    """networkx's source list -- every node in the graph's own order, or seed.sample(list(G), k) -- as rows of
    ``graph.to_csr()`` (sorted labels), in that order."""
    nodes = list(graph.get_nodes())
    if k is not None:
        if isinstance(k, bool) or not isinstance(k, Integral) or not 1 <= k <= len(nodes):
            raise ValueError(f'k must be an integer in 1..{len(nodes)} (the number of nodes), got {k!r}')
        nodes = _py_random_state(seed).sample(nodes, int(k))
    return _rows_of(graph, nodes)


def _rescale_factor(n: int, normalized: bool, directed: bool, k: Optional[int], endpoints: bool) -> float:
    """The factor of networkx's _rescale (1.0 where networkx leaves the sums as they are)."""
    if normalized:
        if endpoints:
            scale = None if n < 2 else 1 / (n * (n - 1))
        elif n <= 2:
            scale = None
        else:
            scale = 1 / ((n - 1) * (n - 2))
    else:
        scale = None if directed else 0.5
    if scale is not None and k is not None:
        scale = scale * n / k
    return 1.0 if scale is None else scale


def betweenness_centrality(G, k: Optional[int] = None, normalized: bool = True, weight=None, endpoints: bool = False,
                           seed=None) -> pd.Series:
    """
    Betweenness centrality on the GPU: networkx 3.4.2's ``betweenness_centrality(G, k, normalized, weight=None,
    endpoints, seed)`` (Brandes' algorithm, one BFS per source) restated by csrc/grx_betweenness.hip, many sources
    per batch.

    :param G: any graph ``node_measures`` accepts; multigraph edges count once, self-loops never lie on a shortest path
    :param k: None = every node is a source, in the graph's own node order (``list(G)``, igraph vertex order, CSRGraph
      row order); otherwise ``seed.sample(list(nodes), k)`` sources in the sampled order, and the sums scaled by n / k
    :param normalized, endpoints: as networkx
    :param weight: must be None here; ``weighted_betweenness_centrality(G, weight='weight')`` computes betweenness
      over shortest paths by weight
    :param seed: int (``random.Random(seed)``), None (the global state of ``random``, as networkx) or ``random.Random``
    :return: float64 Series indexed by the sorted node labels (the index of ``node_measures``)
    :raises NotImplementedError: weight is not None
    :raises ValueError: k outside 1..n
    :raises TypeError: a seed of another type

    Values agree with networkx to 1e-12 relative: only the order of the additions inside one source's dependency
    delta(v) differs.  Stated divergences: k = 0 raises ValueError (networkx: ZeroDivisionError); a numpy random state
    as seed raises TypeError (networkx accepts it).
    """
    if weight is not None:
        raise NotImplementedError(f'weighted betweenness (nx.betweenness_centrality(G, weight={weight!r})) walks '
                                  f'shortest paths by weight, which this function does not; '
                                  f"weighted_betweenness_centrality(G, weight='weight') computes it")
    frame = node_measures(G, ['betweenness_centrality'], k=k, seed=seed, normalized=normalized, endpoints=endpoints)
    return frame['betweenness_centrality']


def _weighted_betweenness_refusals(graph, what: str) -> None:
    """What betweenness by weight refuses, read from the host edge arrays: no device work."""
    if _has_parallel_edges(graph):
        raise NotImplementedError(f'{what}: shortest paths by weight are not computed on a multigraph or a graph with '
                                  f'parallel edges (their weights are summed into one arc here, where Dijkstra takes '
                                  f'the lightest); merge the parallel edges first')
    w = _host_arcs(graph.to_csr())[2]
    if w is not None and len(w) and (not np.all(np.isfinite(w)) or np.min(w) <= 0):
        raise ValueError(f'{what}: edge weights must be finite and > 0 (a zero weight makes networkx count paths '
                         f'through nodes it has already settled, so its own result depends on the order of its heap; '
                         f'a negative, NaN or infinite weight defines no shortest path)')


def weighted_betweenness_centrality(G, k: Optional[int] = None, normalized: bool = True, weight='weight',
                                    endpoints: bool = False, seed=None) -> pd.Series:
    """
    Betweenness centrality over shortest paths by edge weight on the GPU: networkx 3.4.2's
    ``betweenness_centrality(G, k, normalized, weight='weight', endpoints, seed)`` (Brandes' algorithm with one
    Dijkstra search per source) restated without a priority queue by csrc/grx_weighted_betweenness.hip, up to 64
    sources per batch.  The Bellman-Ford relaxation of ``dijkstra_path_lengths`` gives networkx's distances D bit for
    bit; the arc u -> v of weight w lies on a lightest path iff ``D[u] + w == D[v]`` as doubles -- networkx's own test
    of "equally short" -- and ``D[u] < D[v]``; the path counts and the dependencies then run over that DAG in the order
    of its depth.

    :param G: any graph ``node_measures`` accepts, without parallel edges; self-loops never lie on a shortest path
    :param k, normalized, endpoints, seed: as ``betweenness_centrality``: the same sources, in the same order, and the
      same scale
    :param weight: ``'weight'`` = the edge attribute the adapters read (a ``CSRGraph``'s weight array; a missing
      attribute counts 1); None = ``betweenness_centrality(G, ...)``, the unweighted kernel
    :return: float64 Series named ``betweenness_centrality`` indexed by the sorted node labels; ``.attrs['rounds']``
      holds the relaxation rounds run (summed over the batches of sources) and ``.attrs['levels']`` the deepest level
      of any source's shortest-path DAG (the most arcs on a lightest path)
    :raises ValueError: a weight that is not finite and > 0; k outside 1..n.  A zero weight is refused because
      networkx then counts paths through nodes it has already settled: its own result depends on the order of its heap
    :raises NotImplementedError: a multigraph or parallel edges; another `weight` (a different attribute name, a
      callable); G is directed and its adapter has no in-adjacency
    :raises TypeError: a seed of another type

    Values agree with networkx to 1e-12 relative -- only the order of the additions inside one source's dependency
    delta(v) differs -- and the entries networkx has at exactly 0 are exactly 0.  Stated divergences: those of
    ``betweenness_centrality``; zero weights raise; an edge whose weight is absorbed by the distance before it
    (``d + w == d`` in fp64, e.g. 1e-17 after 1.0) is not a shortest-path edge here, where networkx's answer depends on
    its heap order.
    """
    if not _weight_flag('betweenness_centrality', weight):
        return betweenness_centrality(G, k=k, normalized=normalized, endpoints=endpoints, seed=seed)
    frame = node_measures(G, ['betweenness_centrality'], k=k, seed=seed, normalized=normalized, endpoints=endpoints,
                          betweenness_weight='weight')
    series = frame['betweenness_centrality']
    series.attrs = dict(frame.attrs['weighted_betweenness'])
    return series


def _rescale_e_factor(n: int, normalized: bool, directed: bool) -> float:
    """The factor of networkx 3.4.2's _rescale_e as edge_betweenness_centrality calls it -- without `k`, so a sampled
    run is not multiplied by n / k (1.0 where networkx leaves the sums as they are)."""
    if normalized:
        return 1.0 if n <= 1 else 1 / (n * (n - 1))
    return 1.0 if directed else 0.5


def _edge_series(graph, u: np.ndarray, v: np.ndarray, values: np.ndarray, name: str) -> pd.Series:
    """Series of one value per (u, v) -- rows of the sorted labels -- behind the two-level MultiIndex of
    ``truss_number``, in lexicographic order."""
    order = np.lexsort((v, u))
    u, v = u[order], v[order]
    labels = _label_index(graph)
    if isinstance(labels, pd.MultiIndex):                       # tuple labels: each level holds the tuples themselves
        held = np.empty(len(labels), dtype=object)
        held[:] = list(labels)
        ends = [held[u], held[v]]
    else:
        ends = [labels.take(u), labels.take(v)]
    return pd.Series(values[order], name=name, index=pd.MultiIndex.from_arrays(ends, names=['u', 'v']))


def edge_betweenness_centrality(G, k: Optional[int] = None, normalized: bool = True, weight=None,
                                seed=None) -> pd.Series:
    """
    Edge betweenness centrality on the GPU: networkx 3.4.2's ``edge_betweenness_centrality(G, k, normalized, weight,
    seed)`` -- the share of the shortest paths that run over an edge, the quantity Girvan-Newman removes edges by.
    Next to ``truss_number`` (how embedded a tie is) it says how much traffic the tie carries: truss number 2 with a
    high value is a bridge between groups, a high truss number with a low value a redundant tie inside one.  The
    forward and backward passes are those of ``betweenness_centrality`` (csrc/grx_betweenness.hip) resp.
    ``weighted_betweenness_centrality`` (csrc/grx_weighted_betweenness.hip) with sigma kept; one more pass per batch
    adds networkx's own term ``sigma[v] * coeff(w)`` of ``_accumulate_edges`` onto every arc of a source's
    shortest-path DAG.

    :param G: any graph ``node_measures`` accepts, without parallel edges
    :param k, seed: as ``betweenness_centrality``: the same sources in the same order
    :param normalized: as networkx.  The scale is that of networkx 3.4.2 AS IT IS: ``edge_betweenness_centrality`` calls
      ``_rescale_e(betweenness, len(G), normalized=..., directed=...)`` without passing `k`, so a sampled run is NOT
      multiplied by n / k: 1 / (n (n - 1)) when normalized and n > 1, otherwise 0.5 for an undirected graph and
      nothing for a directed one
    :param weight: None = shortest paths by hops; ``'weight'`` = by the edge attribute the adapters read (a missing
      attribute counts 1)
    :return: float64 Series named ``edge_betweenness_centrality`` behind a two-level MultiIndex (levels ``u``, ``v``) of
      node labels, rows in lexicographic order of the sorted labels.  Undirected: one row per edge with u before v,
      self-loops included at 0.0 (networkx keeps them as keys); directed: one row per arc u -> v.  With a weight
      ``.attrs['rounds']`` and ``.attrs['levels']`` as ``weighted_betweenness_centrality``
    :raises NotImplementedError: a multigraph or parallel edges (networkx splits the value between parallel edges: a
      stated divergence); another `weight`; G is directed and its adapter has no in-adjacency
    :raises ValueError: k outside 1..n; with a weight, a weight that is not finite and > 0
    :raises TypeError: a seed of another type

    Values agree with networkx to 1e-12 relative (only the order of additions differs) and the entries networkx has at
    exactly 0 are exactly 0; the same bits for every batch width and run.  An empty graph or one without edges returns
    the empty Series without device work.  The name is not in ``CATALOGUE``: edges are not rows of the node table.
    """
    name = 'edge_betweenness_centrality'
    graph = _adapter(G)
    weighted = _weight_flag(name, weight)
    what = f"edge_betweenness_centrality(G, weight={weight!r})"
    if _has_parallel_edges(graph):
        raise NotImplementedError(f'{what}: not computed on a multigraph or a graph with parallel edges (networkx '
                                  f'splits the value of an arc between its parallel edges); merge them first')
    sources = _betweenness_sources(graph, k, seed)              # argument errors before any device work
    if weighted:
        _weighted_betweenness_refusals(graph, what)
    g = graph.to_csr()
    directed = bool(graph.directed)
    if g.n == 0 or g.num_edges == 0:
        series = pd.Series(np.zeros(0), name=name, index=pd.MultiIndex.from_arrays([[], []], names=['u', 'v']))
        if weighted:
            series.attrs.update(rounds=0, levels=0)
        return series
    K = graph._K()
    scale = _rescale_e_factor(g.n, normalized, directed)
    if weighted:
        host, out, tr = graph._device_graph()
        if directed:
            _weighted_pull(graph, 'weighted edge betweenness centrality')
    else:
        host = graph._device_graph()[0]
        out, tr = _structure_pair(graph, name)
    rows = np.asarray(host.inv)[sources]
    if weighted:
        ebc, rounds, levels = K.weighted_edge_betweenness(out, tr if directed else None, rows, scale)
    else:
        ebc = K.edge_betweenness(out, tr if directed else None, rows, scale)
    row_ptr = np.asarray(_row_ptr_of(K, out), dtype=np.int64)
    nnz = int(row_ptr[-1])
    perm = np.asarray(host.perm, dtype=np.int64)                # internal row -> row of the sorted labels
    u = perm[np.repeat(np.arange(host.n, dtype=np.int64), np.diff(row_ptr))]
    v = perm[_on_host(K, out.col)[:nnz].astype(np.int64)]
    values = _on_host(K, ebc)[:nnz].astype(np.float64)
    keep = np.arange(nnz) if directed else np.nonzero(u <= v)[0]   # undirected: both arcs hold the edge's value
    series = _edge_series(graph, u[keep], v[keep], values[keep], name)
    if weighted:
        series.attrs.update(rounds=rounds, levels=levels)
    return series


def _rows_of(graph, nodes) -> np.ndarray:
    """Rows of ``graph.to_csr()`` (sorted labels) of the node labels `nodes`, in that order."""
    labels = graph.to_csr().labels
    if isinstance(labels, range) and labels == range(len(labels)):
        return np.asarray(nodes, dtype=np.int64)
    row_of = {label: i for i, label in enumerate(labels)}
    return np.fromiter((row_of[v] for v in nodes), dtype=np.int64, count=len(nodes))


def _distance_sums(graph, K, sources: np.ndarray, reverse: bool):
    """kernels.distance_sums from `sources` (internal row ids) along the distinct arcs (``_structure_csrs``: G[v],
    parallel edges once): the out-arcs (pulled over the in-adjacency), or with `reverse` the reversed arcs (pulled over
    the out-adjacency)."""
    if not graph.directed or reverse:
        return K.distance_sums(graph._structure_csrs()[0], sources)
    return K.distance_sums(_structure_pair(graph, 'closeness and harmonic centrality')[1], sources)


def _closeness(reach: np.ndarray, dsum: np.ndarray, n: int, wf_improved: bool) -> np.ndarray:
    """networkx's closeness from len(sp) - 1 = reach and totsp = dsum, with its own IEEE operations:
    (len(sp) - 1.0) / totsp, then *= (len(sp) - 1.0) / (len(G) - 1); 0.0 unless totsp > 0 and len(G) > 1."""
    r = np.asarray(reach, dtype=np.int64).astype(np.float64)
    t = np.asarray(dsum, dtype=np.int64).astype(np.float64)
    ok = (t > 0) & (n > 1)
    c = np.zeros(len(r))
    c[ok] = r[ok] / t[ok]
    if wf_improved and n > 1:
        c[ok] *= r[ok] / float(n - 1)
    return c


def _closeness_by_weight(reach: np.ndarray, dsum: np.ndarray, n: int, wf_improved: bool) -> np.ndarray:
    """``_closeness`` with totsp a sum of fp64 path lengths (networkx's ``distance=``): the same three IEEE operations,
    dsum kept as it is."""
    r = np.asarray(reach, dtype=np.int64).astype(np.float64)
    t = np.asarray(dsum, dtype=np.float64)
    ok = (t > 0) & (n > 1)
    c = np.zeros(len(r))
    c[ok] = r[ok] / t[ok]
    if wf_improved and n > 1:
        c[ok] *= r[ok] / float(n - 1)
    return c


def _distance_arguments(name: str, distance, keyword: str = 'distance') -> None:
    if distance is not None:
        raise NotImplementedError(f'weighted distances (nx.{name}(G, {keyword}={distance!r})) need a shortest-path '
                                  f"search by weight, which this function does not run; "
                                  f"node_measures(G, ['{name}'], distance='weight') computes the column by weight")


#: the columns of ``node_measures`` that `distance` applies to
_DISTANCE_COLUMNS = ('closeness_centrality', 'harmonic_centrality', 'eccentricity')


def _distance_flag(distance) -> bool:
    """networkx's `distance` argument of closeness / harmonic centrality (eccentricity: `weight`): None = hops,
    'weight' = the attribute the adapters read (a CSRGraph's weight array; a missing attribute counts 1)."""
    if distance is None:
        return False
    if isinstance(distance, str) and distance == 'weight':
        return True
    raise NotImplementedError(f"distance={distance!r}: the graph adapters read the edge attribute 'weight' only; pass "
                              f"distance=None or distance='weight', or use networkx")


def _has_parallel_edges(graph) -> bool:
    """A multigraph, or an adapter whose graph holds parallel edges that ``to_csr()`` merged into one arc."""
    if bool(getattr(graph, '_multi', False)):
        return True
    if hasattr(graph, '_is_simple') and not graph._is_simple():
        return graph.get_num_edges() != graph.to_csr().num_edges
    return False


def _weighted_distance_refusals(graph, what: str) -> None:
    """What the distances by weight refuse, read from the host edge arrays: no device work."""
    if _has_parallel_edges(graph):
        raise NotImplementedError(f'{what}: shortest paths by weight are not computed on a multigraph or a graph with '
                                  f'parallel edges (their weights are summed into one arc here, where Dijkstra takes '
                                  f'the lightest); merge the parallel edges first')
    w = _host_arcs(graph.to_csr())[2]
    if w is not None and len(w) and (not np.all(np.isfinite(w)) or np.min(w) < 0):
        raise ValueError(f'{what}: edge weights must be finite and >= 0 (a shortest path by weight is not defined '
                         f'otherwise; networkx raises or loops on such weights)')


def _weighted_pull(graph, what: str):
    """The weighted device CSR a walk along the out-arcs pulls over: the in-adjacency of a directed graph."""
    _, out, tr = graph._device_graph()
    if not graph.directed:
        return out
    if tr is None:
        raise NotImplementedError(f'{type(graph).__name__} has no in-adjacency for this directed graph; '
                                  f'{what} cannot be computed on it')
    return tr


#: largest distance matrix ``dijkstra_path_lengths`` returns
_PATH_LENGTHS_MAX_BYTES = 2 << 30


def dijkstra_path_lengths(G, sources=None, weight='weight') -> pd.DataFrame:
    """
    Shortest-path distances by edge weight on the GPU: row s is networkx 3.4.2's
    ``single_source_dijkstra_path_length(G, s, weight=weight)``, bit for bit, by grx_weighted_distances
    (csrc/grx_sssp.hip) -- a Bellman-Ford relaxation, up to 64 sources per batch, whose fixed point is the minimum over
    the paths of the left-to-right fp64 sum of the weights: what Dijkstra returns when no weight is negative.

    :param G: any graph ``node_measures`` accepts, without parallel edges.  A networkx multigraph and an igraph graph
      with parallel edges are refused; a ``CSRGraph`` refuses duplicate edges when it is built, unless it was built with
      ``validate=False`` -- then duplicates go unnoticed and their weights are summed into one arc
    :param sources: node labels, one row each in the given order (a repeated label repeats its row); None = every node
      in sorted order
    :param weight: ``'weight'`` (a missing attribute counts 1) or None (every edge counts 1: hop counts)
    :return: float64 DataFrame, rows = `sources`, columns = the sorted node labels, ``inf`` where there is no path (the
      nodes networkx leaves out of its dict); ``.attrs['rounds']`` holds the relaxation rounds run
    :raises ValueError: a negative, NaN or infinite weight; a result above 2 GiB (8 bytes x sources x nodes: ask for
      fewer sources per call)
    :raises NotImplementedError: a multigraph or parallel edges; another `weight`
    :raises networkx.NodeNotFound: a source that is not a node
    """
    weighted = _weight_flag('single_source_dijkstra_path_length', weight)
    graph = _adapter(G)
    if weighted:
        _weighted_distance_refusals(graph, 'dijkstra_path_lengths')
    columns = _label_index(graph) if graph.to_csr().n else pd.Index([])
    if sources is None:
        labels = list(columns)
    else:
        labels = list(sources)
        members = set(graph.get_nodes())
        for v in labels:
            if v not in members:
                import networkx as nx
                raise nx.NodeNotFound(f'Node {v} not found in graph')
    n = len(columns)
    if 8 * len(labels) * n > _PATH_LENGTHS_MAX_BYTES:
        raise ValueError(f'dijkstra_path_lengths: {len(labels)} sources x {n} nodes is {8 * len(labels) * n} bytes of '
                         f'distances, above the limit of 2 GiB ({_PATH_LENGTHS_MAX_BYTES} bytes); pass fewer sources '
                         f'per call')
    if not n or not labels:
        return pd.DataFrame(np.empty((len(labels), n)), index=pd.Index(labels), columns=columns)
    K = graph._K()
    host = graph._device_graph()[0]
    pull = _weighted_pull(graph, 'dijkstra_path_lengths')
    if not weighted and pull.w is not None:
        pull = copy.copy(pull)                                  # the same arrays, read without their weights
        pull.w = None
    rows = np.asarray(host.inv)[_rows_of(graph, labels)]
    *_, dist, rounds = K.weighted_distances(pull, rows, want_matrix=True)
    table = host.to_label_order(np.asarray(K.to_host(dist))[:len(labels), :n])
    frame = pd.DataFrame(table, index=pd.Index(labels), columns=columns)
    frame.attrs['rounds'] = rounds
    return frame


def _node_set(graph, nbunch) -> list:
    """networkx's ``set(G.nbunch_iter(nbunch))``: every node for None, the node itself for a node, else the members
    of the iterable that are nodes (others are dropped)."""
    nodes = list(graph.get_nodes())
    if nbunch is None:
        return nodes
    members = set(nodes)
    try:
        if nbunch in members:
            return [nbunch]
    except TypeError:                                          # unhashable: a container of nodes
        pass
    import networkx as nx
    try:
        items = list(iter(nbunch))
    except TypeError as exc:
        raise nx.NetworkXError('nbunch is not a node or a sequence of nodes.') from exc
    try:
        return list(dict.fromkeys(v for v in items if v in members))
    except TypeError as exc:
        raise nx.NetworkXError(f'Node {exc} in sequence nbunch is not a valid node.') from exc


def closeness_centrality(G, u=None, distance=None, wf_improved: bool = True):
    """
    Closeness centrality on the GPU: networkx 3.4.2's ``closeness_centrality(G, u, distance=None, wf_improved)``
    (closeness.py:107-137) from the per-target distance sums of csrc/grx_closeness.hip (a bitset multi-source BFS,
    up to 1 024 sources per pass).

    :param G: any graph ``node_measures`` accepts; multigraph edges count once, self-loops never shorten a path
    :param u: None = every node (every node is a BFS source; for a directed graph the distances d(v, u) run INTO u,
      as networkx's ``G.reverse()``); a node = that node only, one BFS along the reversed arcs
    :param distance: must be None here; ``node_measures(G, [...], distance='weight')`` computes the column over shortest
      paths by weight
    :param wf_improved: as networkx: scale by the fraction of the other nodes that reach u
    :return: float64 Series indexed by the sorted node labels (the index of ``node_measures``), or a float for `u`
    :raises NotImplementedError: distance is not None
    :raises networkx.NodeNotFound: u is not a node

    Bit-equal to networkx: len(sp) - 1 and totsp are exact integer sums, and the value is formed from them with
    networkx's own three IEEE operations.
    """
    _distance_arguments('closeness_centrality', distance)
    if u is None:
        return node_measures(G, ['closeness_centrality'], wf_improved=wf_improved)['closeness_centrality']
    graph = _adapter(G)
    if u not in set(graph.get_nodes()):
        import networkx as nx
        raise nx.NodeNotFound(f'Source {u} is not in G')
    K = graph._K()
    host = graph._device_graph()[0]
    source = np.asarray(host.inv)[_rows_of(graph, [u])]
    reach, dsum, _ = _distance_sums(graph, K, source, reverse=True)
    r = int(K.to_host(reach)[:host.n].sum())
    t = int(K.to_host(dsum)[:host.n].sum())
    return float(_closeness(np.array([r]), np.array([t]), host.n, wf_improved)[0])


def harmonic_centrality(G, nbunch=None, distance=None, sources=None) -> pd.Series:
    """
    Harmonic centrality on the GPU: networkx 3.4.2's ``harmonic_centrality(G, nbunch, distance=None, sources)``
    (harmonic.py:68-89), the sum of 1 / d(v, u) over the sources v that reach u along the out-arcs, from the
    per-target distance sums of csrc/grx_closeness.hip.

    :param G: any graph ``node_measures`` accepts; multigraph edges count once, self-loops never shorten a path
    :param nbunch: the nodes to return (networkx's ``G.nbunch_iter``: a node, an iterable whose non-members are
      dropped, or None = every node)
    :param distance: must be None here; ``node_measures(G, [...], distance='weight')`` computes the column over shortest
      paths by weight
    :param sources: the BFS sources, likewise (duplicates count once)
    :return: float64 Series named ``harmonic_centrality`` indexed by the sorted members of `nbunch`
    :raises NotImplementedError: distance is not None

    Each value is the correctly rounded sum of the fp64 terms 1 / d (an exact fixed-point sum, rounded once), the same
    bits for every source order and run; networkx adds the terms one by one, so the two agree to 1e-12 relative.
    networkx runs the BFS from `nbunch` instead (along the reversed arcs) when it is smaller than `sources`; here the
    BFS always runs from `sources`: the same value, possibly more work, and only the rounding differs.
    """
    _distance_arguments('harmonic_centrality', distance)
    graph = _adapter(G)
    targets = _node_set(graph, nbunch)
    K = graph._K()
    host = graph._device_graph()[0]
    if sources is None:
        rows = np.arange(host.n, dtype=np.int64)
    else:
        rows = np.sort(np.asarray(host.inv)[_rows_of(graph, _node_set(graph, sources))])
    _, _, harmonic = _distance_sums(graph, K, rows, reverse=False)
    series = graph._frame(['harmonic_centrality'], [harmonic], [np.dtype('float64')])['harmonic_centrality']
    if nbunch is None:
        return series
    return series[series.index.isin(targets)]


def _undirected_adapter(G, what: str):
    graph = _adapter(G)
    if graph.directed:
        raise NotImplementedError(f'networkx does not implement nx.{what}(G) for a directed graph')
    return graph


def biconnected_component_counts(G) -> pd.Series:
    """
    The number of biconnected components every node belongs to, on the GPU: ``Counter(v for c in
    nx.biconnected_components(G) for v in c)`` of networkx 3.4.2 (components/biconnected.py), by the Tarjan-Vishkin
    sweeps of csrc/grx_biconnected.hip.  More than one: the node is an articulation point; 0: it has no edge but
    (possibly) a self-loop.

    :param G: any undirected graph ``node_measures`` accepts; multigraph edges count once, self-loops are ignored
    :return: int64 Series named ``biconnected_components`` indexed by the sorted node labels; equal to networkx's
      counts (nodes networkx's Counter leaves out are 0 here)
    :raises NotImplementedError: G is directed (as networkx)
    """
    return node_measures(G, ['biconnected_components'])['biconnected_components']


def articulation_points(G) -> list:
    """
    The articulation points of an undirected graph -- the nodes that lie in more than one biconnected component -- as
    ``nx.articulation_points(G)``, from ``biconnected_component_counts``.

    :return: list of node labels in index order (sorted labels).  Stated divergence: networkx yields the same nodes in
      the order its depth-first search meets them, which it does not specify
    :raises NotImplementedError: G is directed (as networkx)
    """
    counts = biconnected_component_counts(G)
    return list(counts.index[counts.to_numpy() > 1])


def biconnected_components(G) -> list:
    """
    The biconnected components of an undirected graph as ``list(nx.biconnected_components(G))``: a list of node-label
    sets, rebuilt on the host from the BFS forest and the per-tree-edge component labels of csrc/grx_biconnected.hip
    (component r is the union of {c, parent[c]} over the tree edges with label[c] = r) by one numpy group-by.

    :return: list of sets; the order of the list is unspecified, as in networkx.  Isolated nodes are in no component
    :raises NotImplementedError: G is directed (as networkx)
    """
    graph = _undirected_adapter(G, 'biconnected_components')
    K = graph._K()
    host = graph._device_graph()[0]
    _, parent, label, n_components = K.biconnected(graph._structure_csrs()[0])
    parent = np.asarray(K.to_host(parent))[:host.n].astype(np.int64)
    label = np.asarray(K.to_host(label))[:host.n].astype(np.int64)
    child = np.nonzero(parent >= 0)[0]
    # (component, member) pairs of both ends of every tree edge, distinct and grouped by component
    pairs = np.unique(np.stack([np.concatenate([label[child], label[child]]),
                                np.concatenate([child, parent[child]])], axis=1), axis=0)
    members = np.asarray(host.perm)[pairs[:, 1]]                # internal row -> row of the sorted labels
    cuts = np.nonzero(np.diff(pairs[:, 0]))[0] + 1
    labels = graph.to_csr().labels
    plain = isinstance(labels, range) and labels == range(len(labels))
    groups = np.split(members, cuts) if len(members) else []
    assert len(groups) == n_components
    return [set(g.tolist()) if plain else {labels[i] for i in g.tolist()} for g in groups]


def _peeling_refusals(graph, name: str) -> None:
    """networkx's own limits of core_number and onion_layers that the kind of graph does not show: a self-loop, and
    parallel edges of an adapter without a multigraph flag.  Read from the host CSR and edge list: no device work."""
    g = graph.to_csr()
    if not getattr(graph, '_multi', False) and hasattr(graph, '_is_simple') and not graph._is_simple():
        if graph.get_num_edges() != g.num_edges:
            raise NotImplementedError(f'networkx does not implement {CATALOGUE[name]} for a multigraph')
    if getattr(g, 'n_loops', 1) > 0:
        raise NotImplementedError(f'networkx does not implement {CATALOGUE[name]} for a graph with self-loops; remove '
                                  f'them first: G.remove_edges_from(nx.selfloop_edges(G))')


def core_number(G) -> pd.Series:
    """
    The core number of every node on the GPU -- the largest k such that the node belongs to the k-core, the maximal
    subgraph in which every node has degree at least k: ``nx.core_number(G)`` of networkx 3.4.2 (core.py), by the
    synchronous peeling of csrc/grx_kcore.hip.  For a directed graph the degree is in + out, as in networkx.

    :param G: any graph ``node_measures`` accepts, undirected or directed
    :return: int64 Series named ``core_number`` indexed by the sorted node labels; equal to networkx
    :raises NotImplementedError: G has a self-loop (networkx raises NetworkXNotImplemented there; remove them with
      ``G.remove_edges_from(nx.selfloop_edges(G))``) or is a multigraph (networkx implements neither) -- networkx's
      own limits, not divergences; or G is directed and its adapter has no in-adjacency
    """
    return node_measures(G, ['core_number'])['core_number']


def onion_layers(G) -> pd.Series:
    """
    The onion layer of every node on the GPU -- the round of the peeling in which the node is removed, which refines
    the core number (Hebert-Dufresne, Grochow and Allard, 2016): ``nx.onion_layers(G)`` of networkx 3.4.2 (core.py),
    from the same kernel call as ``core_number``.  Name ``'core_number'`` and ``'onion_layer'`` in one
    ``node_measures`` call to get both from one pass.

    :param G: any undirected graph ``node_measures`` accepts
    :return: int64 Series named ``onion_layer`` indexed by the sorted node labels (layers count from 1); equal to
      networkx
    :raises NotImplementedError: G is directed, has a self-loop or is a multigraph: networkx implements onion_layers
      for none of them (its own limits, not divergences)
    """
    return node_measures(G, ['onion_layer'])['onion_layer']


# ------------------------------------------------------------------------------------------------- eccentricity
#: source words of one round of the bounds method when the caller leaves `words` to the library (64 sources per word)
_ECC_BOUNDS_WORDS = 16
_ECC_INF = int(np.iinfo(np.int32).max)


def _row_lengths(csr) -> np.ndarray:
    """Arcs per row of a device CSR, from its host row pointers."""
    host = getattr(csr, '_host', None)                          # kernels.DeviceCSR keeps its row pointers on the host
    return np.diff(np.asarray(csr.row_ptr if host is None else host[0], dtype=np.int64))


def _label_index(graph) -> pd.Index:
    """The index of ``_frame``: the sorted node labels."""
    csr = graph.to_csr()
    return csr.label_index() if hasattr(csr, 'label_index') else pd.Index(graph._device_graph()[0].labels)


def _require_full_reach(K, reach, sources: np.ndarray, n: int, directed: bool) -> None:
    """networkx's ``len(shortest_path_length(G, s)) != len(G)`` for every source s at once: node v is reached by every
    source iff reach[v] + [v is a source] equals the number of sources."""
    got = np.asarray(K.to_host(reach))[:n].astype(np.int64) + np.bincount(sources, minlength=n)
    if np.any(got != len(sources)):
        import networkx as nx
        raise nx.NetworkXError('Found infinite path length because the digraph is not strongly connected' if directed
                               else 'Found infinite path length because the graph is not connected')


def _eccentricity_of_rows(graph, K, sources: np.ndarray, words: int):
    """method='all': one BFS per source (internal row ids) along the out-arcs, pass A only; the device int32 tensor of
    their eccentricities, in the order of `sources`."""
    if graph.directed:
        pull = _structure_pair(graph, 'eccentricity')[1]        # walking out-arcs = pulling over the in-adjacency
    else:
        pull = graph._structure_csrs()[0]
    ecc, reach, _, _ = K.eccentricity_pass(pull, sources, words)
    _require_full_reach(K, reach, sources, pull.n, bool(graph.directed))
    return ecc


def _select_sources(lower: np.ndarray, upper: np.ndarray, open_rows: np.ndarray, rank: np.ndarray,
                    batch: int) -> np.ndarray:
    """The sources of one round of the bounds method among the unresolved rows: half of the batch the rows with the
    largest upper bound, the other half the rows with the smallest lower bound (Takes and Kosters' interchanging
    rule, a batch at a time); ties by `rank` (larger degree, then smaller row).  Ascending row ids."""
    if len(open_rows) <= batch:
        return open_rows
    n_hi = batch // 2
    key = (upper[open_rows] << 31) | (len(rank) - 1 - rank[open_rows])     # distinct keys: the set is determined
    taken = np.argpartition(key, len(key) - n_hi)[len(key) - n_hi:]
    left = np.ones(len(open_rows), dtype=bool)
    left[taken] = False
    hi, rest = open_rows[taken], open_rows[left]
    key = (lower[rest] << 31) | rank[rest]
    lo = rest[np.argpartition(key, batch - n_hi - 1)[:batch - n_hi]]
    return np.sort(np.concatenate([hi, lo]))


def _eccentricity_by_bounds(graph, K, words: int):
    """method='bounds' on an undirected graph: rounds of up to 64 W sources, each one BFS pass for the sources' own
    eccentricities and a second one that tightens every node's bounds with them, until lower = upper everywhere.
    (device int32 tensor of the eccentricities in internal row order, rounds, sources used)."""
    csr = graph._structure_csrs()[0]
    n = csr.n
    batch = 64 * (int(words) or _ECC_BOUNDS_WORDS)
    deg = _row_lengths(csr)
    rank = np.empty(n, dtype=np.int64)
    rank[np.lexsort((np.arange(n), -deg))] = np.arange(n)
    lower = np.zeros(n, dtype=np.int64)
    upper = np.full(n, _ECC_INF, dtype=np.int64)
    bounds = None
    rounds = used = 0
    while True:
        open_rows = np.nonzero(lower < upper)[0]
        if not len(open_rows):
            return bounds[0], rounds, used
        if rounds * batch >= n:                                 # every round resolves at least its own sources
            raise RuntimeError(f'eccentricity bounds did not close after {rounds} rounds of {batch} sources')
        sources = _select_sources(lower, upper, open_rows, rank, batch)
        if bounds is None:
            _, reach, lo, up = K.eccentricity_pass(csr, sources, words, want_upper=True)
            _require_full_reach(K, reach, sources, n, False)    # any one source decides: the graph is undirected
        else:
            _, _, lo, up = K.eccentricity_pass(csr, sources, words, bounds=bounds)
        bounds = (lo, up)
        lower = np.asarray(K.to_host(lo))[:n].astype(np.int64)
        upper = np.asarray(K.to_host(up))[:n].astype(np.int64)
        rounds += 1
        used += len(sources)


def _eccentricity_column(graph, K, method: str, words: int = 0):
    """The eccentricity of every node as a device column in internal row order, and how it was computed:
    (column, {'method', 'rounds', 'sources'})."""
    n = graph._device_graph()[0].n
    if method == 'bounds' and not graph.directed:
        col, rounds, used = _eccentricity_by_bounds(graph, K, words)
        return col, {'method': 'bounds', 'rounds': rounds, 'sources': used}
    col = _eccentricity_of_rows(graph, K, np.arange(n, dtype=np.int64), words)
    return col, {'method': 'all', 'rounds': 1, 'sources': n}


def eccentricity(G, v=None, method: str = 'all', weight=None, words: int = 0):
    """
    Eccentricity on the GPU -- the largest distance from a node to any other node, which separates the periphery of a
    network from its centre: ``nx.eccentricity(G, v)`` of networkx 3.4.2 (distance_measures.py) by grx_eccentricity
    (csrc/grx_closeness.hip), the bitset multi-source BFS of the closeness kernels with a maximum in place of the sums.

    :param G: any graph ``node_measures`` accepts; multigraph edges count once and self-loops are ignored (as in
      networkx, where neither changes a distance)
    :param v: None = every node; a node = that node only; otherwise the members of the iterable that are nodes
      (networkx's ``G.nbunch_iter``)
    :param method: ``'all'`` (the default) runs one BFS per requested node, up to 1 024 per pass.  ``'bounds'`` pins
      every eccentricity from well-chosen BFS sources by the triangle-inequality bounds of Takes and Kosters (2013) --
      ecc(v) <= d(v, s) + ecc(s) and ecc(v) >= max(d(v, s), ecc(s) - d(v, s)) -- up to 64 `words` sources per round, two
      BFS passes per round, until the bounds meet everywhere; networkx's ``_extrema_bounding`` does the same one source
      at a time.  Both are exact.  The bounds need d(s, v) = d(v, s): a directed graph, a single node and an nbunch
      silently take ``'all'``.  ``'bounds'`` is not the default because it lost where it was measured: on the 1 M-node
      BA graph (m = 10; eccentricities 4 to 6) the bounds of most nodes never meet, 48 % of the nodes become sources
      and it takes 4.3 s against 2.45 s (``profiles/eccentricity.txt``); graphs of large diameter prune better.  Worst
      case: a vertex-transitive graph such as a cycle never prunes, every node becomes a source, and the cost is
      twice that of ``'all'``
    :param weight: must be None here; ``node_measures(G, ['eccentricity'], distance='weight')`` computes the column
      over shortest paths by weight.  networkx's ``sp`` is not offered
    :param words: 64-bit source words per BFS pass (1, 2, 4, 8 or 16; 0 = the library's choice, for ``'bounds'`` 16)
    :return: int64 Series named ``eccentricity`` indexed by the sorted node labels (the index of ``node_measures``) or
      by the sorted members of `v`; an int for a single node; equal to networkx
    :raises networkx.NetworkXError: G is not connected / not strongly connected (networkx's two messages); `v` is
      neither a node nor a sequence of nodes
    :raises NotImplementedError: weight is not None; G is directed and its adapter has no in-adjacency
    :raises ValueError: an unknown method
    """
    _distance_arguments('eccentricity', weight, 'weight')
    if method not in ('bounds', 'all'):
        raise ValueError(f"method must be 'bounds' or 'all', got {method!r}")
    graph = _adapter(G)
    single = False
    if v is not None:
        try:
            single = v in set(graph.get_nodes())
        except TypeError:                                      # unhashable: a container of nodes
            pass
    targets = _node_set(graph, v)
    if not targets:                                             # the empty graph, or no member in `v`: networkx's {}
        return pd.Series([], index=pd.Index([]), dtype=np.int64, name='eccentricity')
    K = graph._K()
    host = graph._device_graph()[0]
    if v is None:
        col, info = _eccentricity_column(graph, K, method, words)
        series = graph._frame(['eccentricity'], [col], [np.dtype('int64')])['eccentricity']
        series.attrs.update(info)
        return series
    rows = np.sort(_rows_of(graph, targets))                    # rows of the sorted labels
    ecc = _eccentricity_of_rows(graph, K, np.asarray(host.inv)[rows], words)
    values = np.asarray(K.to_host(ecc)).astype(np.int64)
    if single:
        return int(values[0])
    return pd.Series(values, index=_label_index(graph)[rows], name='eccentricity')


def _eccentricities(G, e):
    """(labels, values) of the eccentricities `e` (a Series of ``eccentricity`` or networkx's dict), computed when
    None; fails on an empty graph as networkx's max() / min() of no values does."""
    if e is None:
        e = eccentricity(G)
    if isinstance(e, pd.Series):
        labels, values = list(e.index), e.to_numpy()
    else:
        labels, values = list(e), np.asarray(list(e.values()))
    if not len(labels):
        raise ValueError('max() arg is an empty sequence: the graph has no node')
    return labels, values


def diameter(G, e=None, usebounds: bool = False) -> int:
    """
    ``nx.diameter(G, e)``: the largest eccentricity, from ``eccentricity(G)`` or the precomputed `e` (its Series, or a
    dict as networkx takes).  `usebounds` is accepted and ignored: pass ``e=eccentricity(G, method='bounds')`` for the
    bounds method (networkx's flag selects a different early exit per function, which is not restated).

    :raises networkx.NetworkXError: G is not (strongly) connected
    :raises ValueError: G has no node (as networkx)
    """
    return int(_eccentricities(G, e)[1].max())


def radius(G, e=None, usebounds: bool = False) -> int:
    """``nx.radius(G, e)``: the smallest eccentricity; arguments and errors as ``diameter``."""
    return int(_eccentricities(G, e)[1].min())


def center(G, e=None, usebounds: bool = False) -> list:
    """
    ``nx.center(G, e)``: the nodes whose eccentricity equals the radius; arguments and errors as ``diameter``.

    :return: list of node labels in index order (sorted labels; the order of `e` when it is given).  Stated
      divergence: networkx lists the same nodes in the graph's own node order
    """
    labels, values = _eccentricities(G, e)
    return [labels[i] for i in np.nonzero(values == values.min())[0]]


def periphery(G, e=None, usebounds: bool = False) -> list:
    """
    ``nx.periphery(G, e)``: the nodes whose eccentricity equals the diameter; arguments and errors as ``diameter``.

    :return: list of node labels in index order (sorted labels; the order of `e` when it is given).  Stated
      divergence: networkx lists the same nodes in the graph's own node order
    """
    labels, values = _eccentricities(G, e)
    return [labels[i] for i in np.nonzero(values == values.max())[0]]


# -------------------------------------------------------------------------------------------- structural holes
def _weight_flag(name: str, weight) -> bool:
    """networkx's `weight` argument of constraint / effective_size: None = every edge counts 1, 'weight' = the
    attribute the adapters read (a CSRGraph's weight array; a missing attribute counts 1)."""
    if weight is None:
        return False
    if isinstance(weight, str) and weight == 'weight':
        return True
    raise NotImplementedError(f"nx.{name}(G, weight={weight!r}): the graph adapters read the edge attribute 'weight' "
                              f"only; pass weight=None or weight='weight', or use networkx")


def _host_arcs(g):
    """(src, dst, weights or None) of the host CSRGraph `g` as rows of the sorted labels: its edge arrays, or -- when it
    carries an explicit neighbour order -- the arcs of its host CSR (an undirected edge then from both ends)."""
    edges = g.edge_arrays()
    if edges is not None:
        return edges
    rows = np.repeat(np.arange(g.n, dtype=np.int64), np.diff(g.row_ptr))
    return rows, np.asarray(g.col, dtype=np.int64), g.w


def _weight_refusals(graph, weighted: bool, parallel_edges: str, bad_weight: str):
    """What the row-intersection measures refuse, read from the host edge arrays (no device work): parallel edges
    (NotImplementedError with the caller's `parallel_edges`) and, with `weighted`, a weight that is not finite or is
    negative (ValueError with the caller's `bad_weight`).  Returns the host weights that were checked, or None."""
    if _has_parallel_edges(graph):
        raise NotImplementedError(parallel_edges)
    w = _host_arcs(graph.to_csr())[2] if weighted else None
    if w is not None and len(w) and (not np.all(np.isfinite(w)) or np.min(w) < 0):
        raise ValueError(bad_weight)
    return w


def _structural_hole_refusals(graph, name: str, weighted: bool) -> None:
    """What constraint and the weighted effective size refuse."""
    _weight_refusals(graph, weighted, _unavailable('constraint', bool(graph.directed), True),
                     f'{name}: edge weights must be finite and >= 0 (networkx computes with whatever it is '
                     f'given; a negative mutual weight has no meaning as a share of attention)')


def _symmetric_union(graph, weighted: bool):
    """The structurally symmetric CSR of networkx's all_neighbors in internal row order, on the host: the union of the
    m arcs and their reverses.  Returns (row_ptr, col, inverse, vals): entry inverse[i] of the CSR holds arc i as given,
    entry inverse[m + i] the same arc seen from its head; vals[i] = its weight (1 without `weighted` or weights)."""
    g = graph.to_csr()
    src, dst, w = _host_arcs(g)
    n = g.n
    inv = np.asarray(graph._device_graph()[0].inv, dtype=np.int64)
    a, b = inv[np.asarray(src, dtype=np.int64)], inv[np.asarray(dst, dtype=np.int64)]
    vals = np.ones(len(a)) if (w is None or not weighted) else np.asarray(w, dtype=np.float64)
    key, inverse = np.unique(np.concatenate([a, b]) * np.int64(max(n, 1)) + np.concatenate([b, a]),
                             return_inverse=True)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // max(n, 1), minlength=n), out=row_ptr[1:])
    return row_ptr, (key % max(n, 1)).astype(np.int32), inverse.ravel(), vals


def _series_of(graph, name: str, nodes, existing: bool, column) -> pd.Series:
    """The float64 Series `name` behind the sorted labels, or behind the sorted members of `nodes`: the column of
    ``node_measures`` when that `existing` one serves, empty for a graph without nodes, otherwise the device column
    (internal row order) that column() computes."""
    rows = _member_rows(graph, nodes)
    if existing:
        series = measures_of(graph, [name])[name]
    elif graph.to_csr().n == 0:
        series = pd.Series([], index=pd.Index([]), dtype=np.float64, name=name)
    else:
        series = graph._frame([name], [column()], [np.dtype('float64')])[name]
    return series if rows is None else series.iloc[rows]


def _mutual_weight_csr(graph, K, weighted: bool):
    """(device CSR, z, out_row_ptr) of grx_structural_holes: the structurally symmetric CSR of networkx's
    all_neighbors in internal row order, its mutual weights z(u, v) = w(u -> v) + w(v -> u) (None = all 1) and the row
    pointers that tell len(G[u]) (None = the CSR's own).  Cached on the adapter per `weighted`."""
    cache = graph.__dict__.setdefault('_mutual_weight', {})
    if weighted in cache:
        return cache[weighted]
    host, out, _ = graph._device_graph()
    if not graph.directed:
        # networkx's mutual weight of an undirected edge is 2 w (a self-loop: 2 w(u, u) as well).  The factor 2 is a
        # power of two and cancels exactly in P = z / sum z and M = z / max z, so the out CSR's own weights serve as z
        cache[weighted] = (out, out.w if weighted else None, None)
        return cache[weighted]
    # directed: the weights of an arc and of its reverse summed -- a reciprocal pair gets w(u -> v) + w(v -> u) from both
    # ends, a loop counts twice
    row_ptr, col, inverse, vals = _symmetric_union(graph, weighted)
    z = np.bincount(inverse, weights=np.concatenate([vals, vals]), minlength=len(col))
    csr = K.DeviceCSR(row_ptr, col, z)
    cache[weighted] = (csr, csr.w, out.row_ptr)
    return cache[weighted]


def _structural_holes(graph, K, weighted: bool, want_constraint: bool, want_effective_size: bool):
    """(constraint, effective size) device columns in internal row order, None for the one not asked for."""
    csr, z, out_row_ptr = _mutual_weight_csr(graph, K, weighted)
    con, es, _ = K.structural_holes(csr, z, out_row_ptr, want_constraint=want_constraint,
                                    want_effective_size=want_effective_size)
    return con, es


def _member_rows(graph, nodes) -> Optional[np.ndarray]:
    """Rows of the sorted labels of the members of `nodes`, ascending and distinct; None for nodes=None.  A member that
    is not a node raises KeyError, as networkx's ``G[v]``."""
    if nodes is None:
        return None
    nodes = list(nodes)
    members = set(graph.get_nodes())
    for v in nodes:
        if v not in members:
            raise KeyError(v)
    return np.unique(_rows_of(graph, nodes))


def _structural_hole_series(G, name: str, nodes, weight) -> pd.Series:
    weighted = _weight_flag(name, weight)
    graph = _adapter(G)
    _structural_hole_refusals(graph, name, weighted)
    # effective size without weights or directions is networkx's ego-graph formula n - 2t/n: the existing column
    return _series_of(graph, name, nodes, name == 'effective_size' and not graph.directed and not weighted,
                      lambda: _structural_holes(graph, graph._K(), weighted, name == 'constraint',
                                                name == 'effective_size')[name == 'effective_size'])


def constraint(G, nodes=None, weight=None) -> pd.Series:
    """
    Burt's constraint of every node on the GPU -- how much of a node's attention goes to contacts that are themselves
    tied to one another; a low value marks a broker across structural holes: ``nx.constraint(G, nodes, weight)`` of
    networkx 3.4.2 (structuralholes.py) by grx_structural_holes (csrc/grx_structural_holes.hip), a row intersection
    per arc of the mutual-weight CSR.  With z(u, v) = w(u -> v) + w(v -> u), P(u, v) = z(u, v) / sum_x z(u, x):
    constraint(u) = sum_v (P(u, v) + sum_w P(u, w) P(w, v))^2 over the neighbours v, w of u in either direction.

    :param G: any graph ``node_measures`` accepts, undirected or directed, with or without self-loops
    :param nodes: None = every node; otherwise an iterable of nodes
    :param weight: None = every edge counts 1; ``'weight'`` = the edge attribute the adapters read (a ``CSRGraph``'s
      weight array; a missing attribute counts 1)
    :return: float64 Series named ``constraint`` indexed by the sorted node labels (the index of ``node_measures``) or
      by the sorted members of `nodes`; NaN for a node without an out-neighbour (networkx: ``len(G[v]) == 0``, in a
      directed graph even when the node has in-arcs)
    :raises NotImplementedError: another `weight` (a different attribute name, a callable); a multigraph or parallel
      edges
    :raises ValueError: a negative or non-finite weight
    :raises KeyError: a member of `nodes` is not a node (as networkx)

    Stated divergences: `weight` is None or ``'weight'``; a multigraph raises (networkx adds the key dictionaries of
    the parallel edges, which is not meaningful); negative and non-finite weights raise (networkx computes with them);
    ``nx.local_constraint(G, u, v)`` is not offered (pairs that are not adjacent need another access pattern; the
    kernel returns it per arc).  Values agree with networkx to 1e-12 relative, not bit for bit: every quotient and
    product is networkx's own IEEE operation, but the sums -- sum_x z(u, x) among them, whose order networkx takes from
    a set -- are added in another order.
    """
    return _structural_hole_series(G, 'constraint', nodes, weight)


def effective_size(G, nodes=None, weight=None) -> pd.Series:
    """
    Burt's effective size of every node's ego network on the GPU: ``nx.effective_size(G, nodes, weight)`` of networkx
    3.4.2 (structuralholes.py).  For an undirected graph with ``weight=None`` it is networkx's ego-graph formula
    n - 2t/n, the ``'effective_size'`` column of ``node_measures`` unchanged; with a `weight` or for a directed graph
    it is sum_v (1 - sum_w P(u, w) M(v, w)), M(v, w) = z(v, w) / max_x z(v, x), from the same kernel call as
    ``constraint`` (grx_structural_holes).

    :param G, nodes, weight: as ``constraint``
    :return: float64 Series named ``effective_size``, indexed as ``constraint``'s; NaN for a node without an
      out-neighbour
    :raises NotImplementedError, ValueError, KeyError: as ``constraint``

    Stated divergences: those of ``constraint``; the weighted form agrees with networkx to 1e-12 times the number of
    neighbours, absolute (its terms cancel).  ``node_measures(D, ['effective_size'])`` of a directed graph still
    raises: this function is the way in.
    """
    return _structural_hole_series(G, 'effective_size', nodes, weight)


# ------------------------------------------------------------------------------- weighted and directed clustering
def _clustering_refusals(graph, weighted: bool) -> None:
    """What clustering refuses."""
    w = _weight_refusals(graph, weighted,
                         f'networkx does not implement {CATALOGUE["clustering"]} for a multigraph, and parallel '
                         f'edges are merged into one arc here; merge the parallel edges first',
                         'clustering: edge weights must be finite and >= 0 (the weight of a triangle is the '
                         'cube root of the product of its three normalised weights)')
    if w is not None and len(w) and np.max(w) == 0:
        raise ValueError('clustering: every edge weight is 0, so the weights cannot be divided by their maximum '
                         '(networkx raises ZeroDivisionError)')


def _max_weight(graph, weighted: bool) -> float:
    """networkx's max_weight: the largest weight of any edge, self-loops included; 1 without weights or edges."""
    w = _host_arcs(graph.to_csr())[2] if weighted else None
    return float(np.max(w)) if w is not None and len(w) else 1.0


def _directional_csr(graph, K, weighted: bool):
    """(device CSR, fwd, bwd) of grx_clustering for a directed graph: the structurally symmetric CSR of networkx's
    all_neighbors in internal row order, with the weight of u -> v (fwd) and of v -> u (bwd) at arc (u, v), -1 where
    that direction is absent; without `weighted` a present direction is 1.  Cached on the adapter per `weighted`."""
    cache = graph.__dict__.setdefault('_directional', {})
    if weighted in cache:
        return cache[weighted]
    row_ptr, col, inverse, vals = _symmetric_union(graph, weighted)
    fwd = np.full(len(col), -1.0)
    bwd = np.full(len(col), -1.0)
    fwd[inverse[:len(vals)]] = vals                             # arc (u, v) as given
    bwd[inverse[len(vals):]] = vals                             # and seen from its head
    csr = K.DeviceCSR(row_ptr, col, fwd)
    cache[weighted] = (csr, csr.w, K.to_device(bwd if len(bwd) else np.zeros(1)))
    return cache[weighted]


def _clustering_column(graph, K, weighted: bool):
    """The device column of grx_clustering in internal row order (not the undirected graph without weights, which is
    the triangle-count column)."""
    if graph.directed:
        csr, fwd, bwd = _directional_csr(graph, K, weighted)
    else:
        csr = graph._device_graph()[1]
        fwd, bwd = (csr.w if weighted else None), None
    return K.clustering(csr, fwd, bwd, _max_weight(graph, weighted and fwd is not None))[0]


def clustering(G, nodes=None, weight=None) -> pd.Series:
    """
    The clustering coefficient of every node on the GPU -- how many of the triangles a node could close with its
    neighbours exist, by weight and by direction: ``nx.clustering(G, nodes, weight)`` of networkx 3.4.2 (cluster.py) in
    its four forms.  For an undirected graph with ``weight=None`` it is the ``'clustering'`` column of
    ``node_measures`` unchanged (triangle counts); a directed graph (Fagiolo's coefficient), a `weight` (Onnela's
    geometric mean of the three normalised weights of each triangle) or both go through grx_clustering
    (csrc/grx_clustering.hip): with s(u, v) = cbrt(w(u -> v) / max_weight) + cbrt(w(v -> u) / max_weight) over the
    neighbours in either direction, t(u) = sum_v s(u, v) sum_w s(u, w) s(v, w) over the triangles (u, v, w), divided by
    d (d - 1) resp. 2 (dt (dt - 1) - 2 db).

    :param G: any graph ``node_measures`` accepts, undirected or directed; self-loops are ignored, as networkx
    :param nodes: None = every node; otherwise an iterable of nodes
    :param weight: None = every edge counts 1; ``'weight'`` = the edge attribute the adapters read (a ``CSRGraph``'s
      weight array; a missing attribute counts 1).  Every weight is divided by the largest one, self-loops included
    :return: float64 Series named ``clustering`` indexed by the sorted node labels (the index of ``node_measures``) or
      by the sorted members of `nodes`
    :raises NotImplementedError: another `weight` (a different attribute name, a callable); a multigraph or parallel
      edges (networkx: not implemented for multigraphs)
    :raises ValueError: a negative or non-finite weight; weights that are all zero
    :raises KeyError: a member of `nodes` is not a node

    Without weights the result equals networkx bit for bit, directed or not (every quantity is an integer), and
    constant weights give those same bits.  Otherwise values agree with networkx to 1e-12 relative: the cube root is
    taken per arc and the three roots are multiplied, where networkx multiplies three quotients and takes one root, and
    the sums run in another order.  Stated divergences: `weight` is None or ``'weight'``; negative and non-finite
    weights raise (networkx computes with them); weights that are all zero raise ValueError (networkx:
    ZeroDivisionError); a zero result is the float 0.0 (networkx: the int 0); weights so small that networkx's product
    of three normalised weights underflows are outside the comparison.  ``triangles`` of a directed graph,
    ``transitivity`` and ``generalized_degree`` are not offered; ``square_clustering`` is a function of its own.
    """
    weighted = _weight_flag('clustering', weight)
    graph = _adapter(G)
    _clustering_refusals(graph, weighted)
    # undirected without weights: the triangle-count column, unchanged
    return _series_of(graph, 'clustering', nodes, not graph.directed and not weighted,
                      lambda: _clustering_column(graph, graph._K(), weighted))


def average_clustering(G, nodes=None, weight=None, count_zeros: bool = True) -> float:
    """
    ``nx.average_clustering(G, nodes, weight, count_zeros)``: the mean of ``clustering(G, nodes, weight)`` on the host;
    with ``count_zeros=False`` the mean of its non-zero values.

    :raises ZeroDivisionError: there is no value to average (no node; with ``count_zeros=False`` no non-zero value), as
      networkx
    :raises NotImplementedError, ValueError, KeyError: as ``clustering``
    """
    values = clustering(G, nodes=nodes, weight=weight).to_numpy()
    if not count_zeros:
        values = values[values != 0]
    if not len(values):
        raise ZeroDivisionError('division by zero')
    return math.fsum(values) / len(values)


# ------------------------------------------------------------------------------------------------ square clustering
def square_clustering(G, nodes=None):
    """
    The square clustering coefficient of every node on the GPU -- the probability that two neighbours of a node share
    a common neighbour other than that node (Lind et al. 2005, Zhang et al. 2008): ``nx.square_clustering(G, nodes)``
    of networkx 3.4.2 (cluster.py).  Triangle clustering is 0 on every bipartite graph; this measure tells a node
    inside a dense bipartite block (near 1) from a star centre or a tree node (0).  grx_square_clustering
    (csrc/grx_square_clustering.hip) counts, for every node v, how many neighbours of v each two-hop neighbour x has --
    row v of A^2 -- in an LDS hash table; networkx's sums over the pairs of neighbours collapse to
    squares = sum_x C(c(x), 2) and potential = (d - 1) (sum_u k_u - d) - 2 T - squares, T the adjacent pairs among the
    neighbours, and the value is squares / potential (squares itself when potential <= 0, as networkx leaves it:
    that is 0 unless self-loops are involved).

    :param G: any undirected graph ``node_measures`` accepts; multigraph edges count once (networkx: ``G[u]`` holds
      distinct neighbours); self-loops are handled as networkx handles them
    :param nodes: None = every node; a node = that node only; otherwise the members of the iterable that are nodes
      (networkx's ``G.nbunch_iter``: others are dropped)
    :return: float64 Series named ``square_clustering`` indexed by the sorted node labels (the index of
      ``node_measures``, so ``M['square_clustering'] = square_clustering(G)`` adds the column to a table for
      ``sense_making``) or by the sorted members of `nodes`; a float for a single node
    :raises NotImplementedError: a directed graph -- networkx's value there depends on the insertion order of the
      adjacency (it tests ``w in G[u]`` for one orientation of each pair only), so there is nothing to restate

    Equal to networkx bit for bit while squares and potential are below 2^53: both are exact integers and the quotient
    is Python's ``int / int``.  Stated divergence: a zero result is the float 0.0 (networkx: the int 0).  The name is
    not in ``CATALOGUE``: this function is the way in.
    """
    graph = _adapter(G)
    if graph.directed:
        raise NotImplementedError('square_clustering of a directed graph is not computed here: networkx\'s value there '
                                  'depends on the insertion order of the adjacency (nx.square_clustering tests '
                                  '`w in G[u]` for one orientation of each pair of neighbours only)')
    single = False
    if nodes is not None:
        try:
            single = nodes in set(graph.get_nodes())
        except TypeError:                                      # unhashable: a container of nodes
            pass
    targets = _node_set(graph, nodes)
    if not targets:                                             # the empty graph, or no member in `nodes`
        return pd.Series([], index=pd.Index([]), dtype=np.float64, name='square_clustering')
    column = graph._K().square_clustering(graph._structure_csrs()[0])[0]
    series = graph._frame(['square_clustering'], [column], [np.dtype('float64')])['square_clustering']
    if nodes is None:
        return series
    series = series.iloc[np.sort(_rows_of(graph, targets))]
    return float(series.iloc[0]) if single else series


# ---------------------------------------------------------------------------------------------------- truss numbers
def _truss_refusals(graph, what: str) -> None:
    """networkx's own limits of k_truss: a directed graph, a multigraph (by the adapter's flag or by parallel edges in
    its edge list) and a self-loop.  Read from the adapter and the host CSR: no device work."""
    if graph.directed:
        raise NotImplementedError(f'networkx does not implement nx.k_truss(G, k) for a directed graph; {what} is not '
                                  f'computed there')
    multi = bool(getattr(graph, '_multi', False))
    g = graph.to_csr()
    if not multi and hasattr(graph, '_is_simple') and not graph._is_simple():
        multi = graph.get_num_edges() != g.num_edges
    if multi:
        raise NotImplementedError(f'networkx does not implement nx.k_truss(G, k) for a multigraph; {what} is not '
                                  f'computed there')
    if getattr(g, 'n_loops', 1) > 0:
        raise NotImplementedError(f'networkx does not implement nx.k_truss(G, k) for a graph with self-loops; remove '
                                  f'them first: G.remove_edges_from(nx.selfloop_edges(G))')


def _on_host(K, array) -> np.ndarray:
    return array if isinstance(array, np.ndarray) else np.asarray(K.to_host(array))


def truss_number(G) -> pd.Series:
    """
    The truss number of every edge on the GPU -- the largest k such that the edge belongs to the k-truss, the maximal
    subgraph in which every edge lies in at least k - 2 triangles of that subgraph (Cohen 2008): the largest k with the
    edge in ``nx.k_truss(G, k)`` of networkx 3.4.2 (core.py), at least 2.  One call of grx_truss_numbers
    (csrc/grx_truss.hip) gives every k at once: the triangle support of every edge by one row intersection per edge,
    then a level-synchronous peeling of the edges (PKT, Kabir and Madduri 2017) in which every triangle is taken away
    exactly once, also when two of its edges leave in the same round.

    :param G: any undirected graph ``node_measures`` accepts
    :return: int64 Series named ``truss_number``, one entry per edge, indexed by a two-level MultiIndex (levels ``u``,
      ``v``) of the edge's node labels with u before v in the order of the ``node_measures`` index (the sorted labels)
      and the rows in lexicographic order of that; ``.attrs['rounds']`` = the peeling rounds run, ``.attrs['levels']``
      = the distinct truss numbers assigned.  Equal to networkx (integers)
    :raises NotImplementedError: G is directed, a multigraph or has a self-loop (remove them with
      ``G.remove_edges_from(nx.selfloop_edges(G))``): networkx implements k_truss for none of them -- its own limits,
      not divergences

    The name is not in ``CATALOGUE``: edges are not rows of the node table; ``node_truss_number`` is the node column.
    """
    graph = _adapter(G)
    _truss_refusals(graph, 'truss_number')
    g = graph.to_csr()
    if g.n == 0 or g.num_edges == 0:
        series = pd.Series(np.zeros(0, dtype=np.int64), name='truss_number',
                           index=pd.MultiIndex.from_arrays([[], []], names=['u', 'v']))
        series.attrs.update(rounds=0, levels=0)
        return series
    K = graph._K()
    host = graph._device_graph()[0]
    csr = graph._structure_csrs()[0]
    arc, _, rounds, levels = K.truss_numbers(csr, want_node=False)
    row_ptr = np.asarray(_row_ptr_of(K, csr), dtype=np.int64)
    nnz = int(row_ptr[-1])
    perm = np.asarray(host.perm, dtype=np.int64)                # internal row -> row of the sorted labels
    u = perm[np.repeat(np.arange(host.n, dtype=np.int64), np.diff(row_ptr))]
    v = perm[_on_host(K, csr.col)[:nnz].astype(np.int64)]
    t = _on_host(K, arc)[:nnz].astype(np.int64)
    once = np.nonzero(u < v)[0]
    once = once[np.lexsort((v[once], u[once]))]
    labels = _label_index(graph)
    if isinstance(labels, pd.MultiIndex):                       # tuple labels: each level holds the tuples themselves
        values = np.empty(len(labels), dtype=object)
        values[:] = list(labels)
        ends = [values[u[once]], values[v[once]]]
    else:
        ends = [labels.take(u[once]), labels.take(v[once])]
    series = pd.Series(t[once], name='truss_number', index=pd.MultiIndex.from_arrays(ends, names=['u', 'v']))
    series.attrs.update(rounds=rounds, levels=levels)
    return series


def _row_ptr_of(K, csr) -> np.ndarray:
    """The row pointers of a device CSR on the host (kernels.DeviceCSR keeps a copy there)."""
    host = getattr(csr, '_host', None)
    return _on_host(K, csr.row_ptr) if host is None else host[0]


def node_truss_number(G) -> pd.Series:
    """
    The truss number of every node on the GPU -- the largest k such that the node belongs to ``nx.k_truss(G, k)``: the
    largest truss number of an edge at it, and 0 for a node without an edge (networkx drops isolated nodes from every
    truss, k = 2 included).  From the same kernel call as ``truss_number``.  It tells the member of a cohesive group
    from a node that is merely well connected: every node of a complete bipartite block K(5, 5) has core number 5, as
    the nodes of a 6-clique have, but truss number 2 against the clique's 6.

    :param G: any undirected graph ``node_measures`` accepts
    :return: int64 Series named ``node_truss_number`` indexed by the sorted node labels (the index of
      ``node_measures``, so ``M['truss_number'] = node_truss_number(G)`` adds the column to a table for
      ``sense_making``); ``.attrs['rounds']`` and ``.attrs['levels']`` as in ``truss_number``.  Equal to networkx
    :raises NotImplementedError: as ``truss_number``

    The name is not in ``CATALOGUE``: this function is the way in.
    """
    graph = _adapter(G)
    _truss_refusals(graph, 'node_truss_number')
    g = graph.to_csr()
    if g.n == 0 or g.num_edges == 0:
        index = _label_index(graph) if g.n else pd.Index([])
        series = pd.Series(np.zeros(g.n, dtype=np.int64), index=index, name='node_truss_number')
        series.attrs.update(rounds=0, levels=0)
        return series
    _, node, rounds, levels = graph._K().truss_numbers(graph._structure_csrs()[0], want_node=True)
    series = graph._frame(['node_truss_number'], [node], [np.dtype('int64')])['node_truss_number']
    series.attrs.update(rounds=rounds, levels=levels)
    return series


def k_truss(G, k):
    """
    The k-truss of a networkx graph as ``nx.k_truss(G, k)``: the maximal subgraph in which every edge lies in at least
    k - 2 triangles of the subgraph, built from the device truss numbers -- an edge-subgraph copy of the edges with
    ``truss_number >= k`` (graph, node and edge attributes copied; nodes without such an edge dropped, as networkx
    drops them) -- instead of networkx's repeated Python pass over all edges.

    :param G: an undirected ``networkx.Graph`` without parallel edges and self-loops
    :param k: the order of the truss
    :return: a new graph of G's class; ``nx.utils.graphs_equal(k_truss(G, k), nx.k_truss(G, k))`` holds
    :raises TypeError: G is not a networkx graph: there is no graph to copy -- use ``truss_number(G)`` and select the
      edges with a value >= k
    :raises NotImplementedError: as ``truss_number``
    """
    import networkx as nx
    if not isinstance(G, nx.Graph):
        raise TypeError(f'k_truss returns a networkx graph and takes one (got {type(G).__name__}); for another graph '
                        f'library use truss_number(G) and keep the edges with a value >= k')
    t = truss_number(G)
    return G.edge_subgraph(t.index[t.to_numpy() >= k].tolist()).copy()


# ------------------------------------------------------------------------------------------ graphlet degree vectors
#: the nine connected graphs on 2, 3 and 4 nodes: name -> (an orbit of the graphlet, how often a copy holds it)
_GRAPHLETS = {'edge': (0, 2), 'path3': (2, 1), 'triangle': (3, 3), 'path4': (4, 2), 'star4': (7, 1), 'cycle4': (8, 4),
              'paw': (9, 1), 'diamond': (13, 2), 'clique4': (14, 4)}
_ORBIT_COLUMNS = [f'orbit_{k}' for k in range(15)]


def _graphlet_refusals(graph, what: str) -> None:
    """Graphlets are defined on a simple undirected graph: a directed graph, a multigraph (by the adapter's flag or by
    parallel edges in its edge list) and a self-loop are refused, each with its remedy.  Read from the adapter and the
    host CSR: no device work."""
    if graph.directed:
        raise NotImplementedError(f'{what}: graphlet orbits 0-14 are those of an undirected graph; a directed graph is '
                                  f'not computed here: pass G.to_undirected()')
    multi = bool(getattr(graph, '_multi', False))
    g = graph.to_csr()
    if not multi and hasattr(graph, '_is_simple') and not graph._is_simple():
        multi = graph.get_num_edges() != g.num_edges
    if multi:
        raise NotImplementedError(f'{what}: graphlet orbits count induced subgraphs of a simple graph; a multigraph is '
                                  f'not computed here: pass nx.Graph(G), which merges the parallel edges')
    if getattr(g, 'n_loops', 1) > 0:
        raise NotImplementedError(f'{what}: graphlet orbits count induced subgraphs of a graph without self-loops; '
                                  f'remove them first: G.remove_edges_from(nx.selfloop_edges(G))')


def _graphlet_totals(frame: pd.DataFrame) -> dict:
    return {name: int(frame[f'orbit_{orbit}'].to_numpy().sum()) // times for name, (orbit, times) in _GRAPHLETS.items()}


def graphlet_degree_vectors(G, nodes=None):
    """
    The graphlet degree vector of every node on the GPU (Przulj 2007): for each of the 15 automorphism orbits of the
    connected graphs on 2, 3 and 4 nodes, the number of induced subgraphs that touch the node at that orbit -- the
    standard signature of a node's local structure, of which ``clustering``, ``square_clustering``, ``truss_number``
    and the structural-hole measures are scalar summaries.  Orbit 0: an edge (the degree); 1, 2: end and middle of a
    path on 3; 3: triangle; 4, 5: end and interior of a path on 4; 6, 7: leaf and centre of a claw; 8: 4-cycle; 9, 10,
    11: the paw's pendant, its triangle nodes off the tail, its triangle node carrying the tail; 12, 13: the diamond's
    degree-2 and degree-3 (chord) nodes; 14: 4-clique.  It separates a star centre (orbit 7) from the interior of a path
    (orbit 5), the tail of a paw from its attachment node, the rim of a diamond from its chord, and counts 4-cliques.

    One call of grx_graphlet_orbits (csrc/grx_graphlets.hip): no induced subgraph is enumerated; the non-induced counts
    come from degrees, triangles per edge, the 4-cycles of grx_square_clustering and a 4-clique listing on the
    degree-oriented graph, and the orbits follow by integer back-substitution.

    :param G: any undirected graph ``node_measures`` accepts, without parallel edges and self-loops
    :param nodes: None = every node; a node = that node only; otherwise the members of the iterable that are nodes
      (as ``square_clustering``)
    :return: DataFrame of int64 columns ``orbit_0`` ... ``orbit_14`` indexed by the sorted node labels (the index of
      ``node_measures``, so ``M = M.join(graphlet_degree_vectors(G))`` adds the columns to a table for
      ``sense_making``) or by the sorted members of `nodes`; a Series (index = the column names) for a single node.
      ``.attrs['graphlets']`` = the nine induced graphlet totals of the WHOLE graph (``graphlet_counts``) as a dict
    :raises NotImplementedError: G is directed (pass ``G.to_undirected()``), a multigraph (pass ``nx.Graph(G)``) or has
      a self-loop (``G.remove_edges_from(nx.selfloop_edges(G))``)

    Exact (integers; equal to brute-force enumeration) while every non-induced count is below 2^53; the same bits in
    every run and for every relabelling.  No orbit is in ``CATALOGUE``: this function is the way in.
    """
    graph = _adapter(G)
    _graphlet_refusals(graph, 'graphlet_degree_vectors')
    g = graph.to_csr()
    if g.n == 0 or g.num_edges == 0:
        index = _label_index(graph) if g.n else pd.Index([])
        frame = pd.DataFrame(np.zeros((g.n, 15), dtype=np.int64), index=index, columns=_ORBIT_COLUMNS)
    else:
        orbits = graph._K().graphlet_orbits(graph._structure_csrs()[0])[0]
        frame = graph._frame(_ORBIT_COLUMNS, [orbits[k] for k in range(15)], [np.dtype('int64')] * 15)
    totals = _graphlet_totals(frame)
    if nodes is not None:
        single = False
        try:
            single = nodes in set(graph.get_nodes())
        except TypeError:                                      # unhashable: a container of nodes
            pass
        targets = _node_set(graph, nodes)
        frame = frame.iloc[np.sort(_rows_of(graph, targets))] if targets else frame.iloc[:0]
        if single:
            frame = frame.iloc[0]
    frame.attrs['graphlets'] = totals
    return frame


def graphlet_counts(G) -> pd.Series:
    """
    The number of induced copies of each of the nine connected graphs on 2, 3 and 4 nodes in G, from the column sums of
    ``graphlet_degree_vectors(G)``: the sum of an orbit divided by the number of nodes of a copy that lie on it.

    :param G: as ``graphlet_degree_vectors``
    :return: int64 Series named ``graphlet_counts`` indexed ``edge, path3, triangle, path4, star4, cycle4, paw,
      diamond, clique4``
    :raises NotImplementedError: as ``graphlet_degree_vectors``
    """
    totals = graphlet_degree_vectors(G).attrs['graphlets']
    return pd.Series([totals[name] for name in _GRAPHLETS], index=pd.Index(list(_GRAPHLETS)), dtype=np.int64,
                     name='graphlet_counts')


# ------------------------------------------------------------------------------------------------- triad census
#: networkx's TRIAD_NAMES, in its order: the 16 isomorphism classes of three nodes with their arcs
TRIAD_NAMES = ('003', '012', '102', '021D', '021U', '021C', '111D', '111U', '030T', '030C', '201', '120D', '120U',
               '120C', '210', '300')
_TRIAD_COLUMNS = [f'triad_{name}' for name in TRIAD_NAMES]


def _triad_refusals(graph, what: str) -> None:
    """The triad census is defined on a simple directed graph: an undirected graph, a multigraph (by the adapter's flag
    or by parallel arcs in its edge list) and a self-loop are refused, each with its remedy.  Read from the adapter and
    the host CSR: no device work."""
    if not graph.directed:
        raise NotImplementedError(f'{what}: networkx does not implement nx.triadic_census(G) for an undirected graph; '
                                  f'pass G.to_directed(), as its docstring advises (only 003, 102, 201 and 300 occur '
                                  f'then)')
    if _has_parallel_edges(graph):
        raise NotImplementedError(f'{what}: a triad is classified by the arcs present, not by how many; a multigraph '
                                  f'or a graph with parallel arcs is not computed here: pass nx.DiGraph(G), which '
                                  f'merges them')
    if getattr(graph.to_csr(), 'n_loops', 1) > 0:
        raise NotImplementedError(f'{what}: a graph with a self-loop is not computed here (networkx\'s own nodelist '
                                  f'path miscounts there, so there is no authority); remove them first: '
                                  f'G.remove_edges_from(nx.selfloop_edges(G))')


def _code_csr(n: int, a: np.ndarray, b: np.ndarray):
    """(row_ptr int64, col int32, codes uint8) of the distinct arcs a -> b (no self-loops) on the rows 0 .. n - 1: the
    structurally symmetric all-neighbours CSR and the direction code of every slot (u, v): 1 = only u -> v, 2 = only
    v -> u, 3 = both."""
    key, inverse = np.unique(np.concatenate([a, b]) * np.int64(max(n, 1)) + np.concatenate([b, a]), return_inverse=True)
    inverse = inverse.ravel()
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // max(n, 1), minlength=n), out=row_ptr[1:])
    codes = np.zeros(len(key), dtype=np.uint8)
    codes[inverse[:len(a)]] |= 1                                # the arc at its tail's slot
    codes[inverse[len(a):]] |= 2                                # and seen from its head
    return row_ptr, (key % max(n, 1)).astype(np.int32), codes


def _triad_csr(graph, K):
    """(device CSR, codes uint8 device tensor, (row_ptr, col, codes) on the host) of grx_triad_census: the structurally
    symmetric CSR of networkx's all_neighbors in internal row order (no diagonal entry: self-loops are refused before)
    and the direction code of every slot.  Cached on the adapter."""
    cached = graph.__dict__.get('_triad')
    if cached is None:
        row_ptr, col, inverse, vals = _symmetric_union(graph, False)
        codes = np.zeros(len(col), dtype=np.uint8)
        codes[inverse[:len(vals)]] |= 1                         # arc (u, v) as given
        codes[inverse[len(vals):]] |= 2                         # and seen from its head
        csr = K.DeviceCSR(row_ptr, col)
        cached = graph.__dict__['_triad'] = (csr, K.to_device(codes if len(codes) else np.zeros(1, dtype=np.uint8)),
                                             (row_ptr, col, codes))
    return cached


def _triad_totals(K, csr, codes) -> List[int]:
    """The census of the graph from one call: the 16 totals, 128 bytes read back."""
    return [int(x) for x in np.asarray(K.to_host(K.triad_census(csr, codes, want_totals=True)[1]))[:16]]


def _edgeless_census(n: int) -> List[int]:
    return [n * (n - 1) * (n - 2) // 6] + [0] * 15


def _triadic_census(graph, removed: Optional[np.ndarray] = None) -> List[int]:
    """The census of the graph, or of what is left of it without the rows `removed` of the sorted labels (the induced
    subgraph, built on the host from the arcs)."""
    g = graph.to_csr()
    if g.n == 0 or g.num_edges == 0:
        return _edgeless_census(g.n - (0 if removed is None else len(removed)))
    K = graph._K()
    csr, codes, (row_ptr, col, host_codes) = _triad_csr(graph, K)
    if removed is None:
        return _triad_totals(K, csr, codes)
    keep = np.ones(g.n, dtype=bool)
    keep[np.asarray(graph._device_graph()[0].inv, dtype=np.int64)[removed]] = False
    new_row = np.cumsum(keep) - 1
    rows = np.repeat(np.arange(g.n, dtype=np.int64), np.diff(row_ptr))
    arc = (host_codes & 1).astype(bool) & keep[rows] & keep[col]
    left = int(keep.sum())
    if not arc.any():
        return _edgeless_census(left)
    sub_ptr, sub_col, sub_codes = _code_csr(left, new_row[rows[arc]], new_row[col[arc].astype(np.int64)])
    return _triad_totals(K, K.DeviceCSR(sub_ptr, sub_col), K.to_device(sub_codes))


def triadic_census(G, nodelist=None) -> dict:
    """
    The triad census of a directed graph on the GPU -- how many of the 16 isomorphism classes of three nodes with
    their arcs (Holland and Leinhardt 1970) occur: ``nx.triadic_census(G, nodelist)`` of networkx 3.4.2 (triads.py).
    The names say Mutual, Asymmetric and Null pairs, then Down, Up, Cyclic or Transitive: ``003`` (no arc), ``012``,
    ``102``, ``021D``, ``021U``, ``021C``, ``111D``, ``111U``, ``030T``, ``030C``, ``201``, ``120D``, ``120U``,
    ``120C``, ``210``, ``300`` (the mutual clique).  One call of grx_triad_census (csrc/grx_triads.hip); only the
    totals, 128 bytes, come back.

    :param G: any directed graph ``node_measures`` accepts, without parallel arcs and self-loops
    :param nodelist: None = every triad; otherwise a list of distinct nodes: only the triads with at least one member
      in it count.  Computed as the census of G minus the census of G without the listed nodes (a triad with no listed
      member is a triad of that induced subgraph): two device calls
    :return: dict name -> Python int, the 16 names in networkx's order; equal to networkx
    :raises NotImplementedError: G is undirected (pass ``G.to_directed()``), a multigraph or has parallel arcs (pass
      ``nx.DiGraph(G)``) or has a self-loop (``G.remove_edges_from(nx.selfloop_edges(G))``)
    :raises ValueError: `nodelist` holds a node twice or something that is not a node, as networkx

    Exact (integers) while C(n - 1, 2) is below 2^53.  ``node_triad_census`` is the per-node table.
    """
    graph = _adapter(G)
    _triad_refusals(graph, 'triadic_census')
    removed = None
    if nodelist is not None:
        nodelist = list(nodelist)
        members = set(graph.get_nodes())
        try:
            listed = {v for v in nodelist if v in members}
        except TypeError:                                      # unhashable: not a node
            listed = set()
        if len(listed) != len(nodelist):
            raise ValueError('nodelist includes duplicate nodes or nodes not in G')
        if not nodelist:                                       # no triad has a member in an empty list
            return dict.fromkeys(TRIAD_NAMES, 0)
        removed = _rows_of(graph, nodelist)
    whole = _triadic_census(graph)
    if removed is not None:
        whole = [a - b for a, b in zip(whole, _triadic_census(graph, removed))]
    return dict(zip(TRIAD_NAMES, whole))


def node_triad_census(G, nodes=None):
    """
    The triad census of every node of a directed graph on the GPU: for each of the 16 triad types, the number of
    triads of that type that contain the node -- ``nx.triadic_census(G, nodelist=[v])`` for every v at once, the
    directed counterpart of orbits 0-3 of ``graphlet_degree_vectors`` and the classical signature of a node's role in
    a directed network.  It separates a broadcaster (many ``021D`` around it) from a sink (``021U``), a relay
    (``021C``), a member of a feed-forward hierarchy (``030T``), of a cycle (``030C``) and of a mutual clique
    (``300``), which Fagiolo's ``clustering(D)`` folds into one number.

    One call of grx_triad_census (csrc/grx_triads.hip): only the closed triads are enumerated, by one row intersection
    per adjacent pair; the open ones follow from the classes of every node's neighbours (out-only, in-only, mutual) by
    a fixed 7 x 6 integer matrix, the dyadic ones from degrees and common neighbours, ``003`` from the rest.

    :param G: any directed graph ``node_measures`` accepts, without parallel arcs and self-loops
    :param nodes: None = every node; a node = that node only; otherwise the members of the iterable, each of which
      must be a node
    :return: DataFrame of int64 columns ``triad_003`` ... ``triad_300`` indexed by the sorted node labels (the index of
      ``node_measures``, so ``M = M.join(node_triad_census(D))`` adds the columns to a table for ``sense_making``) or
      by the sorted members of `nodes`; a Series (index = the column names) for a single node.  ``.attrs['census']`` =
      the census of the WHOLE graph (``triadic_census(G)``) as a dict: every column sums to three times its entry
    :raises NotImplementedError: as ``triadic_census``
    :raises KeyError: a member of `nodes` is not a node

    Exact (integers; equal to networkx and to enumeration of all 3-subsets) while C(n - 1, 2) is below 2^53; the same
    bits in every run and for every relabelling.  No column is in ``CATALOGUE``: this function is the way in.
    """
    graph = _adapter(G)
    _triad_refusals(graph, 'node_triad_census')
    single, rows = False, None
    if nodes is not None:
        try:
            single = nodes in set(graph.get_nodes())
        except TypeError:                                      # unhashable: a container of nodes
            pass
        rows = _member_rows(graph, [nodes] if single else nodes)
    g = graph.to_csr()
    if g.n == 0 or g.num_edges == 0:
        index = _label_index(graph) if g.n else pd.Index([])
        frame = pd.DataFrame(np.zeros((g.n, 16), dtype=np.int64), index=index, columns=_TRIAD_COLUMNS)
        frame['triad_003'] = (g.n - 1) * (g.n - 2) // 2
        census = _edgeless_census(g.n)
    else:
        K = graph._K()
        csr, codes, _ = _triad_csr(graph, K)
        columns, totals, _ = K.triad_census(csr, codes, want_totals=True)
        frame = graph._frame(_TRIAD_COLUMNS, [columns[k] for k in range(16)], [np.dtype('int64')] * 16)
        census = [int(x) for x in np.asarray(K.to_host(totals))[:16]]
    if rows is not None:
        frame = frame.iloc[rows]
        if single:
            frame = frame.iloc[0]
    frame.attrs['census'] = dict(zip(TRIAD_NAMES, census))
    return frame


# ----------------------------------------------------------------------------------------------- NeighborSense
#: most membership columns of ``neighbor_roles`` (GRX_MAX_ROLES of include/grx.h)
MAX_ROLES = 32


def _neighbor_arguments(what: str, mode: str, direction: str) -> None:
    if mode not in ('mean', 'sum'):
        raise ValueError(f"{what}: mode must be 'mean' or 'sum' (got {mode!r})")
    if direction not in ('out', 'in', 'all'):
        raise ValueError(f"{what}: direction must be 'out', 'in' or 'all' (got {direction!r})")


def _membership_values(graph, memberships, what: str) -> np.ndarray:
    """The node x role table as float64 rows of the sorted labels, matched by label as ``sense_making`` matches its
    measures; every refusal of the table is raised here, on the host."""
    if not isinstance(memberships, pd.DataFrame):
        raise ValueError(f'{what}: memberships must be a pandas DataFrame (got {type(memberships).__name__})')
    r = memberships.shape[1]
    if r < 1 or r > MAX_ROLES:
        raise ValueError(f'{what}: memberships must have 1 .. {MAX_ROLES} role columns (GRX_MAX_ROLES); got {r}')
    n = graph.to_csr().n
    index = _label_index(graph) if n else pd.Index([])
    if memberships.index.has_duplicates:
        raise ValueError(f'{what}: memberships has duplicate row labels')
    if len(memberships.index) != len(index) or not memberships.index.isin(index).all():
        raise ValueError(f'{what}: memberships must have one row per node of the graph (the same labels)')
    if not memberships.index.equals(index):
        memberships = memberships.reindex(index)
    values = np.empty(memberships.shape, dtype=np.float64)
    for j, name in enumerate(memberships.columns):
        column = memberships.iloc[:, j]
        if not (pd.api.types.is_numeric_dtype(column.dtype) or pd.api.types.is_bool_dtype(column.dtype)):
            raise ValueError(f'{what}: role {name!r} is not numeric (dtype {column.dtype})')
        col = column.to_numpy(dtype=np.float64, na_value=np.nan)
        bad = int(np.count_nonzero(~np.isfinite(col)))
        if bad:
            raise ValueError(f'{what}: role {name!r} has {bad} non-finite entries (NaN or inf)')
        values[:, j] = col
    return values


def _neighbor_refusals(graph, what: str, weighted: bool) -> None:
    _weight_refusals(graph, weighted,
                     f'{what}: a multigraph or a graph with parallel edges is not computed here (their weights are '
                     f'merged into one arc); merge the parallel edges first',
                     f'{what}: edge weights must be finite and >= 0 (a neighbour share by a negative weight has no '
                     f'meaning)')


def _neighbor_csr(graph, K, weighted: bool, direction: str, what: str):
    """(device CSR, its weights or None) the neighbour-role pass walks: the out-adjacency, the in-adjacency or -- 'all' on
    a directed graph -- the symmetric union A + A^T of ``_mutual_weight_csr``.  An undirected graph has one adjacency."""
    _, out, _ = graph._device_graph()
    if not graph.directed or direction == 'out':
        return out, (out.w if weighted else None)
    if direction == 'in':
        tr = _weighted_pull(graph, f"{what}(direction='in')")
        return tr, (tr.w if weighted else None)
    csr, z, _ = _mutual_weight_csr(graph, K, weighted)
    return csr, z


def _neighbor_stack(graph, values: np.ndarray, weighted: bool, mode: str, direction: str, what: str,
                    ones: bool = False):
    """(K, X, host graph): the device block X = [P^T ; N (; 1)] of 2 r (+ 1) feature-major rows of n entries in INTERNAL
    row order -- P uploaded once, transposed into the upper half (grx_transpose), N = op(A) P written under it by
    grx_neighbor_roles, and a row of ones when the column sums of N are wanted from the same Gram pass."""
    K = graph._K()
    host = graph._device_graph()[0]
    n, r = values.shape
    csr, w = _neighbor_csr(graph, K, weighted, direction, what)
    P = K.to_device(host.to_internal(values))
    X = K.empty((2 * r + int(ones), n))
    K.transpose(P, n, r, out=X[:r])
    K.neighbor_roles(csr, P, mode, w, out=X[r:2 * r])
    if ones:
        K.upload_into(X[2 * r], np.ones(n))
    return K, X, host


def neighbor_roles(G, memberships: pd.DataFrame, *, weight=None, mode: str = 'mean',
                   direction: str = 'out') -> pd.DataFrame:
    """
    The neighbour-role table N of RolX NeighborSense (Henderson et al., KDD 2012, section 4) on the GPU: for every node
    the memberships of its neighbours, N = op(A) P -- summed, or averaged by the weight of the arcs -- the table that
    ``RoleExtractor.neighbor_sense`` explains by Q >= 0 with P Q ~ N.  One call of grx_neighbor_roles
    (csrc/grx_neighbor_sense.hip): a gather of one membership row per arc, a fixed summation order per row, the same
    bits in every run.

    :param G: any graph ``node_measures`` accepts, without parallel edges
    :param memberships: node x role DataFrame, e.g. ``node_role_factor``, ``role_percentage``, ``transform(features_b)``
      or one-hot hard roles; rows are matched to the nodes by label (any order, the same label set), entries numeric
      and finite, 1 .. 32 columns
    :param weight: None = every arc counts 1; ``'weight'`` = the edge attribute the adapters read
    :param mode: ``'mean'`` (the weighted average over the neighbours: rows of a row-stochastic P stay stochastic; a
      node without neighbours or of zero strength gets zeros) or ``'sum'`` (A P itself)
    :param direction: for a directed graph ``'out'`` = successors (``G[node]``, what ReFeX aggregates over), ``'in'`` =
      predecessors, ``'all'`` = both, A + A^T: a reciprocal pair's weights add (it counts twice without weights) and so
      does a self-loop; on an undirected graph all three are the one adjacency, where a self-loop makes the node its own
      neighbour once, as ``G[u]`` does
    :return: float64 DataFrame indexed by the sorted node labels (the index of ``node_measures``) with the columns of
      `memberships`; empty for a graph without nodes
    :raises ValueError: a bad `mode` / `direction` / `memberships`, a negative or non-finite weight
    :raises NotImplementedError: a multigraph or parallel edges; another `weight` name; ``direction='in'`` on an adapter
      without an in-adjacency
    """
    what = 'neighbor_roles'
    _neighbor_arguments(what, mode, direction)
    weighted = _weight_flag(what, weight)
    graph = _adapter(G)
    _neighbor_refusals(graph, what, weighted)
    values = _membership_values(graph, memberships, what)
    n, r = values.shape
    if n == 0:
        return pd.DataFrame(np.zeros((0, r)), index=pd.Index([]), columns=memberships.columns)
    K = graph._K()
    host = graph._device_graph()[0]
    csr, w = _neighbor_csr(graph, K, weighted, direction, what)
    N = K.neighbor_roles(csr, K.to_device(host.to_internal(values)), mode, w)
    table = host.to_label_order(K.to_host(N)).T
    return pd.DataFrame(np.ascontiguousarray(table), index=_label_index(graph), columns=memberships.columns)


def _neighbor_normal_equations(G, memberships: pd.DataFrame, weight, mode: str, direction: str, what: str,
                               normalize: bool = False):
    """(K, P^T P, P^T N, the squared column norms of N) from ONE Gram pass over [P | N] on the device; with `normalize`
    every column of N is divided by its mean over the nodes (a column of mean 0 becomes zeros) -- applied to the normal
    equations, the column sums coming from the same pass through a row of ones.  K is None for a graph without nodes
    (all zeros then)."""
    _neighbor_arguments(what, mode, direction)
    weighted = _weight_flag(what, weight)
    graph = _adapter(G)
    _neighbor_refusals(graph, what, weighted)
    values = _membership_values(graph, memberships, what)
    n, r = values.shape
    if n == 0:
        return None, np.zeros((r, r)), np.zeros((r, r)), np.zeros(r)
    K, X, _ = _neighbor_stack(graph, values, weighted, mode, direction, what, ones=normalize)
    gram = K.gram(X, n)[0]
    PtP, PtN, nn = gram[:r, :r].copy(), gram[:r, r:2 * r].copy(), np.diag(gram)[r:2 * r].copy()
    if normalize:
        means = gram[2 * r, r:2 * r] / n
        scale = np.where(means != 0, 1.0 / np.where(means != 0, means, 1.0), 0.0)
        PtN *= scale[None, :]
        nn *= scale * scale
    return K, PtP, PtN, nn


def role_mixing_matrix(G, memberships: pd.DataFrame, *, weight=None, direction: str = 'out') -> pd.DataFrame:
    """
    The role x role table P^T op(A) P: the edge mass between roles, entry (a, b) = the sum over the arcs u -> v of
    w(u, v) P[u, a] P[v, b].  With one-hot memberships it is the block-model arc count between hard roles; an undirected
    edge counts from both ends, so a diagonal entry is twice the edges inside a role (a self-loop counts once).  It is
    the off-diagonal block of the Gram pass of ``RoleExtractor.neighbor_sense`` with ``mode='sum'``: grx_neighbor_roles,
    then grx_gram over [P | A P].  Sums of small integers are exact.

    :param G, memberships, weight, direction: as ``neighbor_roles``
    :return: float64 DataFrame, index = the role of the node, columns = the role of its neighbour, both labelled by the
      columns of `memberships`
    """
    _, _, PtN, _ = _neighbor_normal_equations(G, memberships, weight, 'sum', direction, 'role_mixing_matrix')
    return pd.DataFrame(PtN, index=memberships.columns, columns=memberships.columns)
