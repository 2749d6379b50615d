"""
Expected results of ``RecursiveFeatureExtractor.replay_features``: the chains the name parser must find, and the plain
aggregation chain of a named column -- generation g is ``agg`` over ``G[node]`` of its generation g - 1 parent, no
pruning -- over the aggregate restatements of oracle/refex.py (``_agg_one``: the numpy calls pandas' nanops make, in
adjacency order, integer columns in wrapping int64).  No reference code.
"""
import re

import numpy as np

from oracle import refex

#: (name, generation-0 names, expected (base, chain) or None)
PARSER_CASES = [
    ('degree', ['degree', 'internal_edges', 'external_edges'], ('degree', [])),
    ('external_edges(sum)(mean)', ['degree', 'internal_edges', 'external_edges'], ('external_edges', ['sum', 'mean'])),
    ('degree(mean)(mean)(sum)', ['degree', 'internal_edges', 'external_edges'], ('degree', ['mean', 'mean', 'sum'])),
    ('total_degree(max)', ['in_degree', 'out_degree', 'total_degree', 'internal_edges', 'external_edges'],
     ('total_degree', ['max'])),
    # an attribute whose own name ends in parentheses: it resolves as a whole, before anything is peeled
    ('attribute_f(x)', ['degree', 'attribute_f(x)', 'internal_edges', 'external_edges'], ('attribute_f(x)', [])),
    ('attribute_f(x)(sum)', ['degree', 'attribute_f(x)', 'internal_edges', 'external_edges'], ('attribute_f(x)', ['sum'])),
    ('attribute_a(b)(c)(mean)(sum)', ['degree', 'attribute_a(b)(c)', 'internal_edges', 'external_edges'],
     ('attribute_a(b)(c)', ['mean', 'sum'])),
    # ... and 'attribute_f' alone is no column of that graph
    ('attribute_f(sum)', ['degree', 'attribute_f(x)', 'internal_edges', 'external_edges'], None),
    ('in_degree(sum)', ['degree', 'internal_edges', 'external_edges'], None),          # a directed name, undirected graph
    ('degree(sum', ['degree', 'internal_edges', 'external_edges'], None),
    ('(sum)', ['degree', 'internal_edges', 'external_edges'], None),
    ('', ['degree', 'internal_edges', 'external_edges'], None),
]

_SUFFIX = re.compile(r'^(.*)\(([^()]*)\)$', re.S)


def parse(name, gen0_names):
    rest, chain = name, []
    while rest not in gen0_names:
        m = _SUFFIX.match(rest)
        if m is None:
            return None
        rest, chain = m.group(1), [m.group(2)] + chain
    return rest, chain


def replay(g, names0, cols0, columns, aggs=('sum', 'mean')):
    """{name: column} for the requested names on the OracleGraph g; cols0 are the generation-0 columns with the
    reference's dtypes.  A column of an integer parent stays int64 under the rule of refex.extract_features_typed
    (no float aggregation in ``aggs``, no node without neighbours unless every aggregation is an integer on nothing)."""
    n = g.n
    no_empty = bool(n == 0 or np.diff(g.row_ptr).min() > 0)
    keeps = not (set(refex.FLOAT_AGGS) & set(aggs)) and (no_empty or set(aggs) <= set(refex.INT_SAFE_ON_EMPTY))
    known = {nm: np.asarray(c) for nm, c in zip(names0, cols0)}

    def column(name):
        if name not in known:
            base, chain = parse(name, list(names0))
            parent = column(base + ''.join(f'({a})' for a in chain[:-1]))
            out = np.empty(n, dtype=np.int64 if keeps and parent.dtype.kind in 'iu' else np.float64)
            for v in range(n):
                val = refex._agg_one(parent[g.adj_row(v)], chain[-1])
                out[v] = 0 if isinstance(val, float) and val != val else val      # fillna(0)
            known[name] = out
        return known[name]

    return {name: column(name) for name in columns}
