"""
RolX role extraction (reference: graphrole/roles/extract.py).  Same class, constructor,
properties and error behaviour as the reference's ``RoleExtractor``; NMF, quantisation and the
MDL costs of the model-selection grid run on the GPU (roles/factor.py), the grid loop and the
cost rescaling / arg-min follow the reference on the host.
"""
from __future__ import annotations

from collections import defaultdict
from typing import Dict, Optional, Tuple

import numpy as np
import pandas as pd

from graphrole_amd.roles import factor
from graphrole_amd.types import DataFrameLike, FactorTuple, Node


class RoleExtractor:

    """RolX: factor the node-feature table into node-role and role-feature parts (GPU-resident NMF)."""

    N_ROLE_RANGE = (2, 8)
    MAX_ROLES = 32          # GRX_MAX_ROLES of include/grx.h (17 .. 32 roles run a slower composed update)
    N_BIT_RANGE = (1, 8)
    #: 'kmeans' = the reference's quantiser reproduced (sklearn KMeans(random_state=1) as scikit-learn >= 1.4 runs it:
    #: one k-means++ initialisation, n_init='auto'; pinned on 1.7.2 -- grx_kmeans1d);
    #: 'lloyd_max' = the deterministic Lloyd-Max solver (lower error, other numbers).  Class attribute: set it
    #: on the class or on an instance before fitting.
    quantizer = 'kmeans'

    def __init__(
        self,
        n_roles: Optional[int] = None,
        n_role_range: Optional[Tuple[int, int]] = None,
        n_bit_range: Optional[Tuple[int, int]] = None,
        distributed=None,
    ) -> None:
        """
        n_roles fixes the rank of the factorisation; when it is None the rank and the code length are
        picked by minimum description length over the grid n_role_range x n_bit_range (inclusive
        (low, high) pairs, defaults N_ROLE_RANGE / N_BIT_RANGE).
        distributed (new; the reference is single-process): True / a torch.distributed process group -- every rank
        passes the SAME feature table and seeds numpy alike; the row passes of every factorisation (Gram matrices,
        projection, multiplicative updates, residuals, the KL error cost of a grid cell) cover the rank's rows only
        and are summed over the ranks, the small quantisation runs replicated; every rank ends with the same factors.
        """
        self.n_roles = n_roles
        self.distributed = distributed

        self.min_roles, self.max_roles = n_role_range if n_role_range else self.N_ROLE_RANGE
        self.min_bits, self.max_bits = n_bit_range if n_bit_range else self.N_BIT_RANGE
        # the device kernels factor with at most MAX_ROLES roles (GRX_MAX_ROLES, include/grx.h; the reference accepts
        # any rank, its default grid is 2..8): say so here, not in the middle of a grid search
        too_many = [r for r in (n_roles, self.max_roles if not n_roles else None) if r is not None and r > self.MAX_ROLES]
        if too_many:
            raise ValueError(f'graphrole_amd factors with at most {self.MAX_ROLES} roles (GRX_MAX_ROLES); '
                             f'got {too_many[0]} -- there is no CPU fallback')

        self.node_role_factor: Optional[pd.DataFrame] = None
        self.role_feature_factor: Optional[pd.DataFrame] = None
        self.role_measure_factor: Optional[pd.DataFrame] = None
        self.role_affinity_factor: Optional[pd.DataFrame] = None
        self.model_selection_ = None

    @property
    def roles(self) -> Optional[Dict[Node, float]]:
        """node -> label of its dominant role (first maximum wins), None before fitting (:38-47).
        The arg-max runs on the device (grx_role_argmax); the dict itself is the reference's return type and is
        built from the int32 column with one vectorised label take (a 5 M-entry dict costs ~0.5 s of Python,
        ``dominant_role_index()`` returns the array without it)."""
        if self.node_role_factor is None:
            return None
        frame = self.node_role_factor
        first = self.dominant_role_index()
        labels = np.asarray(frame.columns, dtype=object)[np.maximum(first, 0)]
        if (first < 0).any():                                  # a row of NaNs only: pandas answers NaN
            labels[first < 0] = np.nan
        return dict(zip(frame.index.tolist(), labels.tolist()))

    def dominant_role_index(self) -> Optional[np.ndarray]:
        """New (array-native twin of ``roles``): int32 position of every node's dominant role in
        ``node_role_factor.columns``, rows in the factor's order; -1 for a row of NaNs only."""
        if self.node_role_factor is None:
            return None
        K, G = self._factor_on_device()
        return K.to_host(K.role_argmax(G)) if G is not None else np.zeros(0, dtype=np.int32)

    @property
    def role_percentage(self) -> Optional[DataFrameLike]:
        """row-normalised node-role factor, None before fitting (:49-57): every row divided by its sum, summed in
        the order the reference's per-row ``row.sum()`` adds (grx_row_normalise) -- one upload, one download"""
        if self.node_role_factor is None:
            return None
        frame = self.node_role_factor
        K, G = self._factor_on_device()
        share = K.to_host(K.row_normalise(G)) if G is not None else np.empty(frame.shape, dtype=np.float64)
        return pd.DataFrame(share, index=frame.index, columns=frame.columns)

    def _factor_on_device(self):
        """The CURRENT values of node_role_factor as an n x r fp64 device matrix (the frame is the caller's to
        edit, so it is read at every call: an upload of 8 r bytes per node, ~15 ms at 5 M x 6)."""
        from graphrole_amd import backend
        K = backend.get()
        values = np.ascontiguousarray(self.node_role_factor.to_numpy(dtype=np.float64))
        if values.ndim != 2 or values.shape[1] == 0 or values.shape[0] == 0:
            return K, None
        return K, K.to_device(values)

    def extract_role_factors(self, features: pd.DataFrame) -> None:
        """
        Fit on a node x feature table (rows = nodes).  Fills ``node_role_factor`` (index = the table's
        index, columns role_0 ...) and ``role_feature_factor`` (index role_0 ..., columns = the table's).
        """
        if self.n_roles:
            # the two factors hold n_roles * (n_nodes + n_features) values; encode them with
            # about log2(n_roles * min(shape)) bits (:69-72)
            n_bits = int(np.log2(self.n_roles * min(features.shape)))
            node_role, role_feature = self._get_encoded_role_factors(features, self.n_roles, n_bits, self.quantizer,
                                                                     self._plan(features.shape[0]))
        else:
            node_role, role_feature = self._select_model(features)

        role_labels = [f'role_{i}' for i in range(node_role.shape[1])]
        self.node_role_factor = pd.DataFrame(node_role, index=features.index, columns=role_labels)
        self.role_feature_factor = pd.DataFrame(role_feature, index=role_labels, columns=features.columns)

    def transform(self, features: pd.DataFrame, tol: float = factor.NMF_TOL, max_iter: int = factor.NMF_MAX_ITER) -> pd.DataFrame:
        """
        New (role transfer, Henderson et al. 2012, section 5): the node x role memberships of ANOTHER feature table
        under the fitted role x feature factor, which stays fixed -- ``model.transform(X)`` of the sklearn
        ``NMF(solver='mu')`` the reference fits (roles/factor.py:19): W0 = sqrt(X.mean() / r), multiplicative updates
        of W only, sklearn's stopping rule.

        :param features: node x feature DataFrame whose columns are exactly ``role_feature_factor.columns`` (any order,
          matched by label), e.g. ``RecursiveFeatureExtractor(G_b).replay_features(features_a.columns)``; non-negative
          and without NaN, like the table of a fit
        :return: DataFrame index = ``features.index``, columns role_0 ...; ``.attrs['n_iter']`` holds the iterations run

        H is the CURRENT content of ``role_feature_factor`` (the encoded factor ``extract_role_factors`` stored; the
        frame is the caller's to edit).  Nothing fitted is changed.  One device call (grx_nmf_transform); a table that
        ``extract_features()`` / ``replay_features()`` returned unmodified, with its columns in the factor's order, is
        read from its device copy.
        """
        return self._transform(features, tol, max_iter)[0]

    def _transform(self, features: pd.DataFrame, tol: float, max_iter: int):
        """(the frame ``transform`` returns, its n x r device matrix or None for a table without rows)"""
        if self.node_role_factor is None or self.role_feature_factor is None:
            raise ValueError('transform needs fitted roles: call extract_role_factors first')
        if self.distributed:
            raise NotImplementedError('transform is not sharded: use an extractor without distributed=')
        if not isinstance(features, pd.DataFrame):
            raise ValueError(f'features must be a pandas DataFrame (got {type(features).__name__})')
        wanted = self.role_feature_factor.columns
        if features.columns.has_duplicates:
            raise ValueError('features has duplicate column labels')
        missing = [c for c in wanted if c not in features.columns]
        extra = [c for c in features.columns if c not in wanted]
        if missing or extra:
            raise ValueError(f'features must have exactly the columns of role_feature_factor: missing {missing}, '
                             f'unexpected {extra}')
        if not features.columns.equals(wanted):
            features = features[list(wanted)]
        H = np.ascontiguousarray(self.role_feature_factor.to_numpy(dtype=np.float64))
        if not np.isfinite(H).all() or (H < 0).any():
            raise ValueError('role_feature_factor must hold finite non-negative numbers')
        roles = list(self.role_feature_factor.index)
        from graphrole_amd import backend
        K = backend.get()
        Xd, (n, F) = factor.device_matrix(features)
        if n == 0:
            frame = pd.DataFrame(np.zeros((0, len(roles))), index=features.index, columns=roles)
            frame.attrs['n_iter'] = 0
            return frame, None
        W, info = K.nmf_transform(Xd, n, H, tol, max_iter)
        G = K.transpose(W, len(roles), n)                      # n x r row-major, the layout of the result
        frame = pd.DataFrame(K.to_host(G), index=features.index, columns=roles)
        frame.attrs['n_iter'] = int(info.n_iter)
        return frame, G

    def transform_roles(self, features: pd.DataFrame, tol: float = factor.NMF_TOL,
                        max_iter: int = factor.NMF_MAX_ITER) -> Dict[Node, str]:
        """New: node -> label of the dominant role of ``transform(features, tol, max_iter)`` (first maximum wins, as
        ``roles``; the arg-max runs on the device: grx_role_argmax)."""
        frame, G = self._transform(features, tol, max_iter)
        if G is None:
            return {}
        from graphrole_amd import backend
        K = backend.get()
        first = K.to_host(K.role_argmax(G))
        labels = np.asarray(frame.columns, dtype=object)[np.maximum(first, 0)]
        if (first < 0).any():
            labels[first < 0] = np.nan
        return dict(zip(frame.index.tolist(), labels.tolist()))

    def explain(self):
        raise NotImplementedError('Role explanation ("sense making") is not yet implemented.')

    def sense_making(self, measures: pd.DataFrame, normalize: bool = False) -> pd.DataFrame:
        """
        New (RolX sense making, Henderson et al., KDD 2012): the non-negative role x measure table E with
        node_role_factor @ E ~ measures, column by column min ||G e - m|| over e >= 0.

        :param measures: node x measure table, e.g. ``graphrole_amd.node_measures(G)`` (with
          ``'betweenness_centrality'``, ``'closeness_centrality'``, ``'harmonic_centrality'``,
          ``'biconnected_components'``, ``'core_number'``, ``'onion_layer'``, ``'eccentricity'`` or ``'constraint'``
          named, ``clustering_weight='weight'`` for the weighted clustering column, or
          ``graphrole_amd.betweenness_centrality(G)``, ``graphrole_amd.effective_size(G, weight='weight')`` or
          ``graphrole_amd.clustering(G, weight='weight')`` -- the way in for a directed graph -- added as a column, or
          ``M['square_clustering'] = graphrole_amd.square_clustering(G)``, which has no catalogue name), a
          user-computed column, or the feature table itself; rows are matched to ``node_role_factor.index`` by label (any
          order, the same label set).  Every entry must be a finite number: fill gaps first, e.g.
          ``sense_making(measures.fillna(0))``
        :param normalize: divide every measure by its mean over the nodes first (a measure with mean 0 gives a
          column of zeros), so that measures of different scales compare across columns
        :return: DataFrame index role_0 ..., columns = the measures'; also stored as ``role_measure_factor``

        G^T G and G^T M come from one device pass over [G | M] (grx_gram); the NNLS is grx_host_nnls.  A
        ``distributed`` extractor runs this replicated: every rank holds the same factors.  ``explain()`` is the
        reference's stub and still raises NotImplementedError: this method is the sense-making entry point.
        """
        if self.node_role_factor is None:
            raise ValueError('sense_making needs fitted roles: call extract_role_factors first')
        if not isinstance(measures, pd.DataFrame):
            raise ValueError(f'measures must be a pandas DataFrame (got {type(measures).__name__})')
        index = self.node_role_factor.index
        if measures.index.has_duplicates:
            raise ValueError('measures has duplicate row labels')
        if len(measures.index) != len(index) or not measures.index.isin(index).all():
            raise ValueError('measures must have one row per node of node_role_factor (the same labels)')
        if not measures.index.equals(index):
            measures = measures.reindex(index)
        values = np.empty(measures.shape, dtype=np.float64)
        for j, name in enumerate(measures.columns):
            column = measures.iloc[:, j]
            if not (pd.api.types.is_numeric_dtype(column.dtype) or pd.api.types.is_bool_dtype(column.dtype)):
                raise ValueError(f'measure {name!r} is not numeric (dtype {column.dtype})')
            col = column.to_numpy(dtype=np.float64, na_value=np.nan)
            bad = int(np.count_nonzero(~np.isfinite(col)))
            if bad:
                raise ValueError(f'measure {name!r} has {bad} non-finite entries (NaN or inf); fill them first, '
                                 f'e.g. measures.fillna(0)')
            values[:, j] = col
        if normalize and values.shape[0]:
            means = values.mean(axis=0)
            nonzero = means != 0
            values[:, nonzero] /= means[nonzero]
            values[:, ~nonzero] = 0.0
        from graphrole_amd import backend
        K = backend.get()
        G = np.ascontiguousarray(self.node_role_factor.to_numpy(dtype=np.float64))
        if values.shape[1] == 0:
            E = np.zeros((G.shape[1], 0))
        else:
            GtG, GtM, mm = K.sense_normal_equations(G, values)
            E = K.nnls(GtG, GtM, mm)
        self.role_measure_factor = pd.DataFrame(E, index=self.node_role_factor.columns, columns=measures.columns)
        return self.role_measure_factor

    def neighbor_sense(self, G, memberships: Optional[pd.DataFrame] = None, *, weight=None, mode: str = 'mean',
                       direction: str = 'out', normalize: bool = False) -> pd.DataFrame:
        """
        New (RolX NeighborSense, Henderson et al., KDD 2012, section 4): the non-negative role x role table Q with
        P Q ~ N, column by column min ||P q - n|| over q >= 0, where P holds the memberships and
        N = ``graphrole_amd.neighbor_roles(G, P, ...)`` the memberships of every node's neighbours.  Row a of Q tells
        which roles the neighbours of a role-a node have: do hubs attach to hubs or to the periphery, which role
        bridges which others.  For one-hot memberships with no empty role and ``mode='mean'`` Q is the row-stochastic
        role-to-role neighbour share.

        :param G: the graph the memberships belong to (any graph ``node_measures`` accepts, without parallel edges)
        :param memberships: node x role DataFrame matched to the nodes of G by label; None = ``node_role_factor``.  A
          frame such as ``transform(features_b)`` together with graph B gives the affinities of the LEARNED roles on
          the second graph, to compare with those of the graph they were learned on.  Nothing fitted is changed
        :param weight, mode, direction: as ``neighbor_roles``
        :param normalize: divide every column of N by its mean over the nodes first (a column with mean 0 gives a
          column of zeros), as ``sense_making`` does, so that a rare role compares with a common one
        :return: DataFrame, index = the node's role, columns = its neighbours' role (the labels of `memberships`);
          also stored as ``role_affinity_factor``

        P is uploaded once; grx_neighbor_roles writes N under P^T in one feature-major block, one grx_gram pass over it
        gives P^T P and P^T N, and the NNLS is grx_host_nnls.  A ``distributed`` extractor runs this replicated: every
        rank holds the same factors.  ``explain()`` is the reference's stub and still raises NotImplementedError.
        """
        if memberships is None:
            if self.node_role_factor is None:
                raise ValueError('neighbor_sense needs fitted roles (call extract_role_factors first) or a memberships '
                                 'table')
            memberships = self.node_role_factor
        from graphrole_amd import measures
        K, PtP, PtN, nn = measures._neighbor_normal_equations(G, memberships, weight, mode, direction, 'neighbor_sense',
                                                              normalize=bool(normalize))
        Q = np.zeros_like(PtN) if K is None else K.nnls(PtP, PtN, nn)
        self.role_affinity_factor = pd.DataFrame(Q, index=memberships.columns, columns=memberships.columns)
        return self.role_affinity_factor

    def similar_nodes(self, nodes=None, k: int = 10, metric: str = 'cosine', include_self: bool = False,
                      memberships: Optional[pd.DataFrame] = None, candidates: Optional[pd.DataFrame] = None):
        """
        New (RolX structural similarity, Henderson et al., KDD 2012, section 5.2): the k nodes that play the role mix of
        `nodes` most closely -- ``graphrole_amd.nearest_nodes`` on the memberships, an exact search on the device
        (grx_similar_rows).

        :param nodes, k, metric, include_self, candidates: as ``nearest_nodes``; ``candidates=transform(features_b)``
          asks which nodes of a second graph resemble a node of the fitted one
        :param memberships: the node x role table the queries come from; None = the CURRENT ``node_role_factor`` (the
          frame is the caller's to edit, so it is uploaded at every call, as ``roles`` does)
        :return: what ``nearest_nodes`` returns: a Series for a single node, otherwise ``(neighbors, scores)``

        Nothing fitted is changed.
        """
        if memberships is None:
            if self.node_role_factor is None:
                raise ValueError('similar_nodes needs fitted roles (call extract_role_factors first) or a memberships '
                                 'table')
            memberships = self.node_role_factor
        from graphrole_amd import similarity
        return similarity.nearest_nodes(memberships, nodes, k=k, metric=metric, include_self=include_self,
                                        candidates=candidates)

    def _plan(self, n_rows: int):
        """Row shards of the feature table (equal row counts: every row of the NMF passes costs the same)."""
        if not self.distributed:
            return None
        from graphrole_amd import parallel
        return parallel.maybe_plan(np.zeros(n_rows + 1, dtype=np.int64), self.distributed)

    def _select_model(self, features: pd.DataFrame) -> FactorTuple:
        """
        Grid search over (n_roles, n_bits) scored by minimum description length (:98-142).
        Like the reference, the NMF is recomputed for every cell, so numpy's global RNG is
        consumed in the same order (one Gaussian test matrix per cell).  The feature matrix is
        uploaded once; factorisation, quantisation and both MDL costs of every cell are computed
        in HBM, only the winning factor pair is copied back.
        """
        from graphrole_amd import backend
        K = backend.get()
        Vd, V = factor.device_matrix(features)             # V = (n, F): the table itself stays in HBM
        plan = self._plan(V[0])
        rb, re = (0, V[0]) if plan is None else (plan.row_begin, plan.row_end)
        bit_stop = self.max_bits + 1
        role_stop = min(min(features.shape), self.max_roles) + 1
        encoding_costs = np.full((role_stop, bit_stop), np.nan)
        error_costs = np.full((role_stop, bit_stop), np.nan)
        factors = defaultdict(dict)

        for roles in range(self.min_roles, role_stop):
            for bits in range(self.min_bits, bit_stop):
                try:
                    state, Wq, Hq, uniq_g, uniq_f = factor.encoded_factors_device(Vd, V, roles, bits, self.quantizer,
                                                                                  plan)
                except factor.TooFewSamples:
                    # more bins requested than there are factor entries to quantise (the reference swallows
                    # KMeans' ValueError here, roles/extract.py:127-129); any other error surfaces
                    continue
                # description_length.py:32-41 / :44-61 on the device-resident factors
                encoding_costs[roles, bits] = np.ceil(np.log2(max(uniq_g, uniq_f))) * (Wq.numel() + Hq.numel())
                cost = state.kl_cost(Wq, Hq, rb, re)
                if plan is not None:
                    cost = float(plan.all_reduce_sum_host(np.array([cost]))[0])
                error_costs[roles, bits] = cost
                factors[roles][bits] = (Wq, Hq)

        costs = self._rescale_costs(encoding_costs) + self._rescale_costs(error_costs)
        best_roles, best_bits = np.argwhere(costs == np.nanmin(costs))[0]
        #: diagnostics of the last grid search: both cost grids and the selected (n_roles, n_bits) cell
        self.model_selection_ = {'encoding_costs': encoding_costs, 'error_costs': error_costs,
                                 'selected': (int(best_roles), int(best_bits))}
        Wq, Hq = factors[best_roles][best_bits]
        # transposed to the n x r layout of the result in HBM: a strided host transpose of the factor costs more
        # than the copy itself
        return K.to_host(K.transpose(Wq, int(best_roles), V[0])), K.to_host(Hq).copy()

    @staticmethod
    def _get_encoded_role_factors(features: pd.DataFrame, n_roles: int, n_bits: int,
                                  quantizer: Optional[str] = None, plan=None) -> FactorTuple:
        """NMF of the feature matrix with both factors quantised to 2**n_bits levels (:144-161)"""
        from graphrole_amd import backend
        K = backend.get()
        Vd, V = factor.device_matrix(features)
        _, Gq, Hq, _, _ = factor.encoded_factors_device(Vd, V, n_roles, n_bits, quantizer or RoleExtractor.quantizer,
                                                        plan, want_node_major=True)
        # Gq is already the n x r row-major matrix the reference returns: one copy out, no host transpose
        return K.to_host(Gq.contiguous() if hasattr(Gq, 'contiguous') else Gq).reshape(V[0], n_roles), K.to_host(Hq).copy()

    @staticmethod
    def _rescale_costs(costs: np.ndarray) -> np.ndarray:
        """row-wise L2 normalisation that ignores NaN cells (:163-173)"""
        norms = np.sqrt(np.nansum(np.square(costs), axis=1))
        return costs / norms.reshape(costs.shape[0], 1)
