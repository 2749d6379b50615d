"""
Structural similarity (Henderson et al., KDD 2012, section 5.2): which nodes play the same role as this one?  The
answer is a comparison of the rows of a node x column table -- memberships, ReFeX features or the output of
``RoleExtractor.transform`` -- and the rows are compared on the device: grx_similar_rows (csrc/grx_similarity.hip), an
exact k-nearest search by cosine similarity or Euclidean distance.  This module is the host side: labels, refusals and
frames.  No reference counterpart (the reference stops at the factors).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import pandas as pd

#: most columns of a table (GRX_MAX_ROLES of include/grx.h)
MAX_COLUMNS = 32
#: most neighbours per query (GRX_MAX_TOPK of include/grx.h)
MAX_TOPK = 64
METRICS = ('cosine', 'euclidean')


def _table_values(table, what: str, name: str) -> np.ndarray:
    """The table as contiguous float64 rows; every refusal of its content is raised here, on the host."""
    if not isinstance(table, pd.DataFrame):
        raise ValueError(f'{what}: {name} must be a pandas DataFrame (got {type(table).__name__})')
    c = table.shape[1]
    if c < 1 or c > MAX_COLUMNS:
        raise ValueError(f'{what}: {name} must have 1 .. {MAX_COLUMNS} columns (GRX_MAX_ROLES); got {c} -- select the '
                         f'columns to compare first')
    if table.index.has_duplicates:
        raise ValueError(f'{what}: {name} has duplicate row labels; drop or relabel them first')
    values = np.empty(table.shape, dtype=np.float64)
    for j, label in enumerate(table.columns):
        column = table.iloc[:, j]
        if not (pd.api.types.is_numeric_dtype(column.dtype) or pd.api.types.is_bool_dtype(column.dtype)):
            raise ValueError(f'{what}: column {label!r} of {name} is not numeric (dtype {column.dtype})')
        col = column.to_numpy(dtype=np.float64, na_value=np.nan)
        bad = int(np.count_nonzero(~np.isfinite(col)))
        if bad:
            raise ValueError(f'{what}: column {label!r} of {name} has {bad} non-finite entries (NaN or inf); fill them '
                             f'first, e.g. {name}.fillna(0)')
        values[:, j] = col
    return values


def _frames(neighbors, scores, index, k: int, metric: str):
    columns = pd.RangeIndex(k)
    out = (pd.DataFrame(neighbors, index=index, columns=columns),
           pd.DataFrame(scores, index=index, columns=columns, dtype=np.float64))
    for frame in out:
        frame.attrs['metric'] = metric
        frame.attrs['k'] = k
    return out


def nearest_nodes(table: pd.DataFrame, nodes=None, k: int = 10, metric: str = 'cosine', include_self: bool = False,
                  candidates: Optional[pd.DataFrame] = None):
    """
    The k nodes whose rows of `table` are nearest to those of `nodes`, exactly, on the GPU: one call of
    grx_similar_rows.  Ties are broken by the position of the candidate's row (the earlier row first), so the result is
    unique and the same in every run.

    :param table: node x column DataFrame: ``node_role_factor``, ``role_percentage``, the ReFeX feature table (select
      at most 32 columns) or ``transform(features_b)``; entries numeric and finite
    :param nodes: None = every row of `table`; a single label = that node; otherwise an iterable of labels (an unknown
      label raises KeyError, as ``table.loc`` does)
    :param k: neighbours per query, 1 .. 64 (GRX_MAX_TOPK) and at most the number of admissible candidates
    :param metric: ``'cosine'`` -- dot product of the rows scaled to unit length, larger is nearer, a row of zeros scores
      0 with everything -- or ``'euclidean'`` -- the distance, smaller is nearer
    :param include_self: False leaves out the query's own row, by position: another node with the very same row is
      still a neighbour (score 1.0 resp. distance 0.0).  Without effect when `candidates` is given
    :param candidates: a second table with the same column labels (any order; matched by label).  The neighbours are
      then searched among ITS rows, the queries still come from `table`, and nothing is left out: which nodes of graph B
      resemble node x of graph A is ``nearest_nodes(P_a, [x], candidates=role_extractor.transform(features_b))``
    :return: for a single label a float64 Series named `metric`, indexed by the neighbours' labels in rank order;
      otherwise ``(neighbors, scores)``, two frames indexed by the query labels with the columns 0 .. k - 1 --
      `neighbors` holds labels of the candidate table, `scores` float64 -- and ``.attrs`` ``metric`` and ``k``.  An
      empty table (or no query) gives empty frames
    :raises ValueError: non-finite or non-numeric entries, more than 32 columns, duplicate labels, `k` out of range,
      another `metric`, columns of `candidates` that differ
    :raises KeyError: an unknown label in `nodes`
    """
    what = 'nearest_nodes'
    if metric not in METRICS:
        raise ValueError(f"{what}: metric must be 'cosine' or 'euclidean' (got {metric!r})")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f'{what}: k must be an integer >= 1 (got {k!r})')
    k = int(k)
    if k > MAX_TOPK:
        raise ValueError(f'{what}: k = {k} is above GRX_MAX_TOPK = {MAX_TOPK}; ask for at most {MAX_TOPK} neighbours per '
                         f'node')
    values = _table_values(table, what, 'table')
    pool, pool_index = values, table.index
    if candidates is not None:
        if not isinstance(candidates, pd.DataFrame):
            raise ValueError(f'{what}: candidates must be a pandas DataFrame (got {type(candidates).__name__})')
        if candidates.columns.has_duplicates or table.columns.has_duplicates:
            raise ValueError(f'{what}: duplicate column labels; the columns of table and candidates are matched by label')
        missing = [col for col in table.columns if col not in candidates.columns]
        extra = [col for col in candidates.columns if col not in table.columns]
        if missing or extra:
            raise ValueError(f'{what}: candidates must have exactly the columns of table: missing {missing}, unexpected '
                             f'{extra}')
        if not candidates.columns.equals(table.columns):
            candidates = candidates[list(table.columns)]
        pool, pool_index = _table_values(candidates, what, 'candidates'), candidates.index

    single = False
    if nodes is None:
        rows = np.arange(len(table), dtype=np.int64)
    else:
        try:
            single = nodes in table.index
        except TypeError:                                      # unhashable: a container of labels
            single = False
        labels = [nodes] if single else list(nodes)
        rows = table.index.get_indexer(labels) if labels else np.zeros(0, dtype=np.int64)
        if (rows < 0).any():
            raise KeyError(f'{[lab for lab, r in zip(labels, rows) if r < 0]} not in the index of table')
    queries = table.index[rows]
    if len(rows) == 0 or len(table) == 0:
        if single:
            return pd.Series([], index=pool_index[:0], dtype=np.float64, name=metric)
        return _frames(np.empty((0, k), dtype=pool_index.to_numpy().dtype), np.empty((0, k)), queries, k, metric)
    exclude = candidates is None and not include_self
    admissible = len(pool) - int(exclude)
    if k > admissible:
        raise ValueError(f'{what}: k = {k} neighbours asked for, but only {admissible} candidates are admissible '
                         f'({len(pool)} rows{", the query itself left out" if exclude else ""}); lower k'
                         f'{" or pass include_self=True" if exclude else ""}')

    from graphrole_amd import backend
    K = backend.get()
    X = K.to_device(pool)
    whole = candidates is None and nodes is None
    Q = None if whole else K.to_device(np.ascontiguousarray(values[rows]))
    self_rows = K.to_device(rows.astype(np.int32)) if exclude else None
    if whole and not exclude:                                   # every row queries the table, itself included
        Q = X
    index, score = K.similar_rows(X, Q, self_rows, k=k, metric=metric)
    index, score = np.asarray(K.to_host(index)), np.asarray(K.to_host(score))
    neighbors = pool_index.to_numpy()[index]
    if single:
        return pd.Series(score[0], index=pd.Index(neighbors[0], name=pool_index.name), dtype=np.float64, name=metric)
    return _frames(neighbors, score, queries, k, metric)
