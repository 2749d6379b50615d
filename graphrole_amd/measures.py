"""
Node measures for RolX sense making (Henderson et al., KDD 2012, section 4): the node x measure table M that
``RoleExtractor.sense_making`` explains by E >= 0 with G E ~ M.  Every measure restates networkx 3.4.2 with its
default arguments and is computed on the device CSR the feature extractor uses (graph/interface/base.py
``_device_graph``): degrees by grx_row_sums, clustering and effective size by grx_local_structure_measures on the
triangle counts of grx_triangle_counts, PageRank and eigenvector centrality by the power iterations of
csrc/grx_measures.hip.
"""
from __future__ import annotations

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
    'pagerank': "nx.pagerank(G, alpha, weight='weight', tol=tol, max_iter=max_iter)",
    'eigenvector': "nx.eigenvector_centrality(G, max_iter=max_iter, tol=tol, weight='weight')",
}


def _unavailable(name: str, directed: bool, multi: bool) -> Optional[str]:
    """Why `name` is not computed for this kind of graph (None = it is)."""
    kind = ('directed ' if directed else 'undirected ') + ('multigraph' if multi else 'graph')
    if name in ('in_degree', 'out_degree') and not directed:
        return f'{name} is defined for directed graphs only'
    if name in ('clustering', 'effective_size'):
        if multi and name == 'clustering':
            return f'networkx does not implement {CATALOGUE[name]} for a multigraph'
        if directed or multi:
            return (f'{name} of a {kind} is not computed here (only undirected graphs without parallel edges); '
                    f'use {CATALOGUE[name]} from networkx')
    if name == 'eigenvector' and multi:
        return f'networkx does not implement {CATALOGUE[name]} for a multigraph'
    return None


def available_measures(directed: bool, multi: bool) -> List[str]:
    """The catalogue entries defined for a graph of this kind, in catalogue order."""
    return [name for name in CATALOGUE if _unavailable(name, directed, multi) is None]


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
                  max_iter: int = 100) -> pd.DataFrame:
    """
    Node x measure table of well-known graph measures, computed on the GPU.

    :param G: any graph ``RecursiveFeatureExtractor`` accepts (networkx graph or multigraph, CSRGraph, igraph)
    :param measures: names from ``CATALOGUE`` in the order of the columns; None = every measure defined for the
      graph's kind (``available_measures``)
    :param alpha, tol, max_iter: networkx's arguments of pagerank (alpha, tol, max_iter) and eigenvector_centrality
      (tol, max_iter)
    :return: DataFrame indexed by the sorted node labels (the index of ``extract_features()``);
      ``.attrs['iterations']`` holds the power-iteration counts
    :raises ValueError: an unknown measure name
    :raises NotImplementedError: a measure that networkx does not implement for this kind of graph, or that is
      outside this implementation's scope (directed / multigraph clustering and effective size)
    :raises ConvergenceError: PageRank or eigenvector centrality did not converge within max_iter iterations

    Stated divergence: ``effective_size`` of a node whose only neighbour is itself is NaN (networkx raises
    ZeroDivisionError).
    """
    return measures_of(_adapter(G), measures, alpha=alpha, tol=tol, max_iter=max_iter)


def measures_of(graph, measures: Optional[Sequence[str]] = None, *, alpha: float = 0.85, tol: float = 1e-6,
                max_iter: int = 100) -> pd.DataFrame:
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
        for nm in names:
            why = _unavailable(nm, directed, multi)
            if why is not None:
                raise NotImplementedError(why)
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
        elif nm == 'clustering':
            col, dt = local()[0], np.dtype('float64')
        elif nm == 'effective_size':
            col, dt = local()[1], np.dtype('float64')
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
    return frame
