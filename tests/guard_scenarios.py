"""
The scenario table of tests/test_gpu_guard_bands.py: one entry per kernel family of graphrole_amd.kernels.

A scenario has a name, the entry points it covers (``covers``; tests/test_guarded_alloc_cpu.py checks that the union
of these and its exclusion list is the whole ABI), ``run(K)`` -- which drives the wrappers on the smallest shapes that
still reach every launch shape and returns {key: host array}, every array cut to its DEFINED region ([:n], [:nnz],
out[:, :n]; padding up to ld and the max(n, 1) slot are left out on purpose: poison legitimately survives there) --
and, where the family has an array-level oracle next to the tests, ``want()``: {key: (expected array, how)} for some
or all of the keys, compared as the family's own test compares them (``how``: EXACT, or (rtol, atol) copied from that
test, or a callable(got, want)).  Inputs come from what the tests already have (tests/graphs.py,
tests/rowjoin_graphs.py, the *_oracle.py modules); nothing here draws from an unseeded generator.

``repeatable=False`` marks a family whose bits may differ between two runs (none today: every family documents "the
same bits in every run"); such a scenario is compared with want() only.
"""
import functools
from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np

from tests import graphs, rowjoin_graphs as rg, square_clustering_oracle as sqo

EXACT = 'exact'
LANES = (4, 32)                       # the hub launch (rows above 128 arcs) and the lane-group launch
ROW_COUNTS = (1, 63, 65, 257, 1037)   # never a multiple of the block
SYM_GRAPHS = ('n1', 'star200', 'K70', 'wheel1500', 'ba2000')


class Scenario(NamedTuple):
    name: str
    covers: Tuple[str, ...]
    run: Callable
    want: Optional[Callable] = None
    repeatable: bool = True


SCENARIOS = []


def scenario(name, covers, want=None, repeatable=True):
    def register(run):
        SCENARIOS.append(Scenario(name, tuple(covers), run, want, repeatable))
        return run
    return register


# ---- graphs -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sym(key):
    """(n, row_ptr int64, col int32) of the symmetric CSR of a named undirected graph.  star200: a centre with 200
    leaves plus a ring (with chords) on the leaves -- a hub row at lanes = 4, longer than 32 x 4."""
    n, pairs = rg._threshold_pairs(200) if key == 'star200' else rg._named_pairs(key)
    row_ptr, col = sqo.csr_from_pairs(n, pairs)
    row_ptr.setflags(write=False)
    col.setflags(write=False)
    return n, row_ptr, col


def arc_values(row_ptr, col, kind):
    """fp64[nnz] symmetric arc values of rowjoin_graphs.WEIGHTS[kind] (None for 'unweighted')."""
    f = rg.WEIGHTS[kind]
    if f is None:
        return None
    rows = np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr))
    c = col.astype(np.int64)
    return np.asarray(f(np.minimum(rows, c), np.maximum(rows, c)), dtype=np.float64)


@functools.lru_cache(maxsize=None)
def dw300():
    """The directed weighted graph: gnm(300, 1200) with reciprocal pairs and two loops (tests/graphs.py)."""
    G = graphs.directed_weighted_attrs(300, 1200, 3)[0]
    assert any(G.has_edge(v, u) for u, v in G.edges if u != v) and G.has_edge(5, 5)
    return G


@functools.lru_cache(maxsize=None)
def dw300_arrays():
    G = dw300()
    src = np.array([u for u, v in G.edges], dtype=np.int64)
    dst = np.array([v for u, v in G.edges], dtype=np.int64)
    w = np.array([G[u][v]['weight'] for u, v in G.edges], dtype=np.float64)
    return G.number_of_nodes(), src, dst, w


def with_lanes(K, csr, lanes):
    """The CSR with the hub list of another lane width (what the lanes= argument of the measures does)."""
    _, n_hubs, lanes_per_row, hub_rows = K._hubs_for(csr, lanes)
    csr.hub_rows, csr.n_hubs, csr.lanes_per_row = hub_rows, n_hubs, lanes_per_row
    return csr


def host(K, t, *cut):
    """Host copy of a device tensor cut to its defined region."""
    a = K.to_host(t)
    for axis, k in enumerate(cut):
        if k is not None:
            a = a[(slice(None),) * axis + (slice(0, k),)]
    return np.ascontiguousarray(a).copy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def exact(d):
    return {k: (v, EXACT) for k, v in d.items()}


def _oracle_graph(n, src, dst, w, directed):
    from oracle import refex
    return refex.graph_from_arrays(n, src, dst, w, directed)


def _features(n, f, seed):
    return np.abs(np.random.default_rng(seed).standard_normal((n, f))) * 10.0 ** np.arange(f).clip(0, 6)


# ---- generation 0: row sums, ego-net, triangle counts, small movers ----------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gen0_graphs():
    from tests import util
    out = {}
    n, src, dst, w = dw300_arrays()
    out['dw300'] = (_oracle_graph(n, src, dst, w, True), True)
    s, d, w = util.random_graph(300, 2000, 2, False, True, 5)
    out['uw300'] = (_oracle_graph(300, s, d, w, False), False)
    for key in SYM_GRAPHS:
        n, row_ptr, col = sym(key)
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
        keep = rows < col
        out[key] = (_oracle_graph(n, rows[keep], col[keep].astype(np.int64), None, False), False)
    return out


def _run_gen0(K):
    out = {}
    for name, (og, directed) in _gen0_graphs().items():
        n = og.n
        csr = K.DeviceCSR(og.row_ptr, og.col, og.w, agg_col=og.adj_col)
        out[f'{name}/rowsum'] = host(K, K.row_sums(csr, not directed), n)
        rb, re = n // 3, n - n // 4
        out[f'{name}/rowsum_part'] = host(K, K.row_sums(csr, False, rb, re), n)          # zeros outside [rb, re)
        out[f'{name}/rowcount'] = host(K, K.row_counts(csr, False), n)
        for L in (LANES if og.w is None and not directed else (None,)):
            if L is not None:
                with_lanes(K, csr, L)
            tag = f'{name}/L{L}'
            i, e = K.egonet_features(csr, directed)
            out[f'{tag}/internal'], out[f'{tag}/external'] = host(K, i, n), host(K, e, n)
            i, e = K.egonet_features(csr, directed, row_begin=rb, row_end=re)           # partial: zeros outside
            out[f'{tag}/internal_part'], out[f'{tag}/external_part'] = host(K, i, n), host(K, e, n)
            i, e = K.egonet_features_general(csr, directed)
            out[f'{tag}/internal_general'], out[f'{tag}/external_general'] = host(K, i, n), host(K, e, n)
        if og.w is None and not directed:
            T = K.triangle_counts(csr)
            out[f'{name}/T'] = host(K, T, n)
            out[f'{name}/T_part'] = host(K, K.triangle_counts(csr, rb, re), n)
            i, e = K.egonet_from_triangles(csr, T)
            out[f'{name}/internal_T'], out[f'{name}/external_T'] = host(K, i, n), host(K, e, n)
    return out


def _want_gen0():
    from oracle import refex
    want = {}
    for name, (og, directed) in _gen0_graphs().items():
        ego = refex.egonet_features_c(og)
        loc = refex.local_features_c(og)
        # tests/test_gpu_kernels.py:57-70: rtol 1e-12 on the sums and the internal weight, 1e-11 on the external
        # weight, == on unweighted graphs
        weighted = og.w is not None
        want[f'{name}/rowsum'] = (loc['out_degree'] if directed else loc['degree'], (1e-12, 0.0) if weighted else EXACT)
        for L in (LANES if not weighted and not directed else (None,)):
            for suffix in ('', '_general'):
                want[f'{name}/L{L}/internal{suffix}'] = (ego['internal_edges'], (1e-12, 0.0) if weighted else EXACT)
                want[f'{name}/L{L}/external{suffix}'] = (ego['external_edges'], (1e-11, 0.0) if weighted else EXACT)
        if not weighted and not directed:
            want[f'{name}/internal_T'] = (ego['internal_edges'], EXACT)
            want[f'{name}/external_T'] = (ego['external_edges'], EXACT)
    return want


scenario('gen0', ('grx_row_sums', 'grx_egonet_features', 'grx_triangle_counts', 'grx_egonet_unweighted', 'grx_memset'),
         _want_gen0)(_run_gen0)


def _mover_inputs():
    rng = np.random.default_rng(21)
    return {n: (rng.standard_normal((9, n)), rng.permutation(n).astype(np.int32)) for n in ROW_COUNTS}


def _run_movers(K):
    out = {}
    for n, (X, index) in _mover_inputs().items():
        Xd = K.to_device(X)
        cols = [Xd[c] for c in range(X.shape[0])]
        out[f'{n}/add'] = host(K, K.add_columns(cols[0], cols[1]))
        out[f'{n}/gather'] = host(K, K.gather_columns(cols, n), None, n)
        out[f'{n}/permute'] = host(K, K.permute_columns(cols, K.to_device(index), n))
        out[f'{n}/transpose'] = host(K, K.transpose(Xd, 9, n))
        out[f'{n}/min'] = np.array([K.min_value(Xd, n)])
        out[f'{n}/i64_to_f64'] = host(K, K.convert_i64_to_f64(K.to_device(_i64(n).view(np.float64))))
        out[f'{n}/f64_to_i64'] = bits(host(K, K.convert_f64_to_i64(K.to_device(_i64(n).astype(np.float64)))))
        for f in (1, 3, 9):
            rows, ldr = K.pack_rows(cols[:f], n)
            out[f'{n}/pack{f}'] = host(K, rows, n)                                       # pad columns are written zeros
    return out


def _i64(n):
    return np.random.default_rng(n).integers(-2 ** 40, 2 ** 40, size=n)


def _want_movers():
    want = {}
    for n, (X, index) in _mover_inputs().items():
        want[f'{n}/add'] = X[0] + X[1]
        want[f'{n}/gather'] = X
        want[f'{n}/permute'] = X[:, index]
        want[f'{n}/transpose'] = np.ascontiguousarray(X.T)
        want[f'{n}/min'] = np.array([X.min()])
        want[f'{n}/i64_to_f64'] = _i64(n).astype(np.float64)
        want[f'{n}/f64_to_i64'] = _i64(n)
    return exact(want)


scenario('movers', ('grx_add_columns', 'grx_gather_columns', 'grx_permute_columns', 'grx_transpose', 'grx_min_value',
                    'grx_convert_i64_to_f64', 'grx_convert_f64_to_i64', 'grx_pack_rows'), _want_movers)(_run_movers)


# ---- pack_rows / pack_rows_i32 -------------------------------------------------------------------------------------------

PACK_F = (1, 3, 9, 23, 130)


def _run_pack(K):
    out = {}
    for n in (1, 65, 1037):
        rng = np.random.default_rng(n)
        X = rng.standard_normal((max(PACK_F), n))
        Xi = rng.integers(0, 2 ** 31, size=(8, n)).astype(np.float64)
        Xd, Xid = K.to_device(X), K.to_device(Xi)
        for f in PACK_F:
            rows, ldr = K.pack_rows([Xd[c] for c in range(f)], n)
            out[f'{n}/f{f}'] = host(K, rows, n)
            if f <= 8:
                rows, ldi = K.pack_rows_i32([Xid[c] for c in range(f)], n)
                out[f'{n}/i32_f{f}'] = host(K, rows, n, f)                               # the pad columns are not defined
    return out


def _want_pack():
    want = {}
    for n in (1, 65, 1037):
        rng = np.random.default_rng(n)
        X = rng.standard_normal((max(PACK_F), n))
        Xi = rng.integers(0, 2 ** 31, size=(8, n)).astype(np.float64)
        for f in PACK_F:
            want[f'{n}/f{f}'] = (lambda got, w, f=f: (np.array_equal(got[:, :f], w) and not got[:, f:].any()), X[:f].T)
            if f <= 8:
                want[f'{n}/i32_f{f}'] = (EXACT, Xi[:f].T.astype(np.int32))
    return {k: (w, how) for k, (how, w) in want.items()}


scenario('pack_rows', ('grx_pack_rows', 'grx_pack_rows_i32'), _want_pack)(_run_pack)


# ---- the aggregate kernels --------------------------------------------------------------------------------------------

AGG_F = (1, 5, 17)


@functools.lru_cache(maxsize=None)
def _agg_graphs():
    """name -> OracleGraph (adjacency order = order of appearance) of the symmetric graphs, three dangling rows added."""
    out = {}
    for key in SYM_GRAPHS:
        og = _gen0_graphs()[key][0]
        og = _oracle_graph(og.n, *_edges_of(og), None, False)
        if key != 'n1':
            og.row_ptr = np.concatenate([og.row_ptr, np.full(3, og.row_ptr[-1])])
        out[key] = og
    return out


def _edges_of(og):
    rows = np.repeat(np.arange(og.n, dtype=np.int64), np.diff(og.row_ptr))
    keep = rows < og.col
    return rows[keep], og.col[keep].astype(np.int64)


def _agg_range(n):
    return (n // 5, n - n // 7) if n > 3 else (0, n)


def _run_aggregate(K):
    out = {}
    for name, og in _agg_graphs().items():
        n = og.n
        rb, re = _agg_range(n)
        for L in LANES:
            csr = K.DeviceCSR(og.row_ptr, og.col, None, agg_col=og.adj_col)
            csr.plan().set_lanes(L)
            for f in AGG_F:
                tag = f'{name}/L{L}/f{f}'
                X = _features(n, f, f)
                X[:, 0] *= np.where(np.random.default_rng(1).random(n) < 0.3, -1.0, 1.0)
                Xd = K.to_device(np.ascontiguousarray(X.T))
                rows, ldr = K.pack_rows([Xd[c] for c in range(f)], n)
                blk = K.aggregate(csr, rows, f, ldr)
                out[f'{tag}/sum_mean'] = host(K, blk)
                out[f'{tag}/sum_mean_part'] = host(K, K.aggregate(csr, rows, f, ldr, rb, re))     # zeros outside
                out[f'{tag}/mean_only'] = host(K, K.aggregate(csr, rows, f, ldr, want_sum=False))
                mean = blk[f:].contiguous()
                out[f'{tag}/var_std'] = host(K, K.aggregate_var(csr, rows, f, ldr, mean))
                out[f'{tag}/var_std_part'] = host(K, K.aggregate_var(csr, rows, f, ldr, mean, rb, re, want_var=False))
                out[f'{tag}/minmax'] = host(K, K.aggregate_minmax(csr, rows, f, ldr))
                out[f'{tag}/minmax_part'] = host(K, K.aggregate_minmax(csr, rows, f, ldr, rb, re, want_min=False))
                out[f'{tag}/prod'] = host(K, K.aggregate_prod(csr, rows, f, ldr))
                out[f'{tag}/prod_part'] = host(K, K.aggregate_prod(csr, rows, f, ldr, rb, re))[:, rb:re]
                if f <= 8:
                    Xi = np.random.default_rng(40 + f).integers(0, 2 ** 31, size=(n, f)).astype(np.float64)
                    Xid = K.to_device(np.ascontiguousarray(Xi.T))
                    irows, ldi = K.pack_rows_i32([Xid[c] for c in range(f)], n)
                    out[f'{tag}/i32'] = host(K, K.aggregate_i32(csr, irows, f, ldi))
                    out[f'{tag}/i32_part'] = host(K, K.aggregate_i32(csr, irows, f, ldi, rb, re))[:, rb:re]
    return out


def _want_aggregate():
    from oracle import ckernels
    want = {}
    for name, og in _agg_graphs().items():
        n = og.n
        rb, re = _agg_range(n)
        for f in AGG_F:
            X = _features(n, f, f)
            X[:, 0] *= np.where(np.random.default_rng(1).random(n) < 0.3, -1.0, 1.0)
            S, M = ckernels.aggregate(og.row_ptr, og.adj_col, X)
            V, D = ckernels.aggregate_var(og.row_ptr, og.adj_col, X)
            lo, hi = ckernels.aggregate_minmax(og.row_ptr, og.adj_col, X)
            P = ckernels.aggregate_prod(og.row_ptr, og.adj_col, X)
            part = np.zeros((1, n))
            part[:, rb:re] = 1.0
            for L in LANES:                                     # tests/test_gpu_kernels.py: every one of these with ==
                tag = f'{name}/L{L}/f{f}'
                want[f'{tag}/sum_mean'] = np.vstack([S.T, M.T])
                want[f'{tag}/sum_mean_part'] = np.vstack([S.T, M.T]) * part
                want[f'{tag}/mean_only'] = np.vstack([0 * S.T, M.T])
                want[f'{tag}/var_std'] = np.vstack([V.T, D.T])
                want[f'{tag}/var_std_part'] = np.vstack([0 * V.T, D.T * part])
                want[f'{tag}/minmax'] = np.vstack([lo.T, hi.T])
                want[f'{tag}/minmax_part'] = np.vstack([0 * lo.T, hi.T * part])
                want[f'{tag}/prod'] = P.T
                want[f'{tag}/prod_part'] = P.T[:, rb:re]
                if f <= 8:
                    Xi = np.random.default_rng(40 + f).integers(0, 2 ** 31, size=(n, f)).astype(np.float64)
                    Si, Mi = ckernels.aggregate(og.row_ptr, og.adj_col, Xi)
                    want[f'{tag}/i32'] = np.vstack([Si.T, Mi.T])
                    want[f'{tag}/i32_part'] = np.vstack([Si.T, Mi.T])[:, rb:re]
    return {k: (v + 0.0, EXACT) for k, v in want.items()}       # (+ 0.0: the 0 * x blocks hold -0.0 where x < 0)


scenario('aggregate', ('grx_aggregate', 'grx_aggregate_var', 'grx_aggregate_minmax', 'grx_aggregate_prod',
                       'grx_aggregate_i32', 'grx_pack_rows', 'grx_pack_rows_i32', 'grx_memset'),
         _want_aggregate)(_run_aggregate)


def _aggx_values(name, f):
    from tests import aggx_oracle as ao
    return ao.median_values(name)[:, :f], ao.i64_values(name)[:, :f]


def _run_aggx(K):
    from tests import aggx_oracle as ao
    out = {}
    for name in ('classes', 'powerlaw'):
        row_ptr, adj = ao.graph(name)
        n = len(row_ptr) - 1
        rb, re = ao.ROW_RANGES[name]
        for L in LANES:
            csr = K.DeviceCSR(row_ptr, ao.sorted_col(row_ptr, adj), agg_col=adj)
            csr.plan().set_lanes(L)
            for f in AGG_F:
                if f > min(ao.median_values(name).shape[1], ao.i64_values(name).shape[1]):
                    continue
                tag = f'{name}/L{L}/f{f}'
                Xm, Xi = _aggx_values(name, f)
                rows, ldr = K.pack_rows([K.to_device(np.ascontiguousarray(Xm[:, c])) for c in range(f)], n)
                out[f'{tag}/median'] = host(K, K.aggregate_median(csr, rows, f, ldr))
                out[f'{tag}/median_part'] = host(K, K.aggregate_median(csr, rows, f, ldr, rb, re))[:, rb:re]
                cols = [K.to_device(np.ascontiguousarray(Xi[:, c]).view(np.float64)) for c in range(f)]
                rows, ldr = K.pack_rows(cols, n)
                for agg, t in K.aggregate_i64(csr, rows, f, ldr).items():
                    out[f'{tag}/i64_{agg}'] = bits(host(K, t))
                for agg, t in K.aggregate_i64(csr, rows, f, ldr, rb, re).items():
                    out[f'{tag}/i64_{agg}_part'] = bits(host(K, t))[:, rb:re]
                for as_i64 in (False, True):
                    out[f'{tag}/count{int(as_i64)}'] = bits(host(K, K.aggregate_count(csr, f, as_i64=as_i64)))
                    out[f'{tag}/count{int(as_i64)}_part'] = bits(host(K, K.aggregate_count(csr, f, rb, re, as_i64)))[:, rb:re]
    return out


def _want_aggx():
    from tests import aggx_oracle as ao
    want = {}
    for name in ('classes', 'powerlaw'):
        row_ptr, adj = ao.graph(name)
        rb, re = ao.ROW_RANGES[name]
        for f in AGG_F:
            if f > min(ao.median_values(name).shape[1], ao.i64_values(name).shape[1]):
                continue
            Xm, Xi = _aggx_values(name, f)
            med = ao.median(row_ptr, adj, Xm)
            i64 = ao.aggregate_i64(row_ptr, adj, Xi)
            for L in LANES:                                     # tests/test_gpu_aggx_kernels.py compares bit patterns
                tag = f'{name}/L{L}/f{f}'
                want[f'{tag}/median'] = (med, _same_bits_or_nan)
                want[f'{tag}/median_part'] = (med[:, rb:re], _same_bits_or_nan)
                for agg, w in i64.items():
                    want[f'{tag}/i64_{agg}'] = (w, EXACT)
                    want[f'{tag}/i64_{agg}_part'] = (w[:, rb:re], EXACT)
                for as_i64 in (False, True):
                    c = ao.count(row_ptr, f, as_i64=as_i64)
                    c = c if as_i64 else bits(c)
                    want[f'{tag}/count{int(as_i64)}'] = (c, EXACT)
                    want[f'{tag}/count{int(as_i64)}_part'] = (c[:, rb:re], EXACT)
    return want


def _same_bits_or_nan(got, want):
    return np.array_equal(got, want, equal_nan=True)


scenario('aggx', ('grx_aggregate_median', 'grx_aggregate_i64', 'grx_aggregate_count', 'grx_pack_rows'),
         _want_aggx)(_run_aggx)


def _run_packed(K):
    """grx_column_bits, grx_pack_fields, grx_aggregate_packed as tests/test_gpu_packed.py chains them: the packed sums
    and means must be the bits of grx_aggregate on the fp64 columns (which the 'aggregate' scenario holds to the oracle)."""
    out = {}
    for name, og in _agg_graphs().items():
        n = og.n
        rb, re = _agg_range(n)
        for L in LANES:
            csr = K.DeviceCSR(og.row_ptr, og.col, None, agg_col=og.adj_col)
            csr.plan().set_lanes(L)
            for f in (1, 5):
                tag = f'{name}/L{L}/f{f}'
                Xi = np.random.default_rng(70 + f).integers(0, 1 << 9, size=(f, n)).astype(np.float64)
                Xd = K.to_device(Xi)
                cols = [Xd[c] for c in range(f)]
                block = K.gather_columns(cols, n)
                width = K.column_bits(block, n, (1 << f) - 1)
                out[f'{tag}/bits'] = host(K, width)
                out[f'{tag}/bits_part'] = host(K, K.column_bits(block, n, (1 << f) - 1, rb, re))
                field_bits = [int(b) for b in out[f'{tag}/bits']]
                deg_bits = max(int(np.diff(og.row_ptr).max()).bit_length(), 1)
                layout, row_bytes = K.packed_layout(field_bits, deg_bits, list(range(f)) + [0], [False] * f + [True])
                assert row_bytes in (8, 16), (tag, field_bits, deg_bits)
                rows = K.pack_fields(csr, layout, row_bytes, cols)
                out[f'{tag}/rows'] = host(K, rows, n * row_bytes)
                out[f'{tag}/packed'] = host(K, K.aggregate_packed(csr, layout, rows))
                out[f'{tag}/packed_part'] = host(K, K.aggregate_packed(csr, layout, rows, rb, re))
    return out


def _want_packed():
    from oracle import ckernels
    want = {}
    for name, og in _agg_graphs().items():
        n = og.n
        rb, re = _agg_range(n)
        cnt = np.diff(og.row_ptr).astype(np.float64)
        for f in (1, 5):
            Xi = np.random.default_rng(70 + f).integers(0, 1 << 9, size=(f, n)).astype(np.float64)
            # the parents the layout describes: the f integer columns, then the mean column fl(field 0 / degree)
            parents = np.vstack([Xi, np.where(cnt > 0, Xi[0] / np.where(cnt > 0, cnt, 1.0), 0.0)])
            S, M = ckernels.aggregate(og.row_ptr, og.adj_col, np.ascontiguousarray(parents.T))
            full = np.vstack([S.T, M.T])
            part = np.zeros((1, n))
            part[:, rb:re] = 1.0
            for L in LANES:                                     # tests/test_gpu_packed.py:118: the bits of grx_aggregate
                tag = f'{name}/L{L}/f{f}'
                want[f'{tag}/bits'] = np.array([max(int(x.max()).bit_length(), 1) for x in Xi], dtype=np.int32)
                want[f'{tag}/packed'] = full
                want[f'{tag}/packed_part'] = full * part + 0.0
    return exact(want)


scenario('packed', ('grx_column_bits', 'grx_pack_fields', 'grx_aggregate_packed', 'grx_gather_columns', 'grx_memset'),
         _want_packed)(_run_packed)


# ---- sort, binning, chebyshev -----------------------------------------------------------------------------------------

def _sort_block(ncols, n):
    rng = np.random.default_rng(1000 * ncols + n)
    cols = [rng.standard_normal(n) * 1e3, rng.integers(-5, 6, size=n).astype(np.float64),
            np.abs(rng.standard_normal(n)) * 10.0 ** rng.integers(-300, 300, size=n)]
    return np.stack(cols[:ncols])


def _run_sort(K):
    return {f'{ncols}x{n}': host(K, K.sort_columns(K.to_device(_sort_block(ncols, n))))
            for ncols in (1, 3) for n in (1, 65, 4097)}


def _want_sort():
    return exact({f'{ncols}x{n}': np.sort(_sort_block(ncols, n), axis=1) for ncols in (1, 3) for n in (1, 65, 4097)})


scenario('sort_columns', ('grx_sort_columns',), _want_sort)(_run_sort)


def _bin_columns(n):
    rng = np.random.default_rng(n)
    return [rng.pareto(1.5, n).round(2), rng.integers(0, 30, n).astype(np.float64), rng.standard_normal(n), np.zeros(n),
            np.where(rng.random(n) < 0.9, 0.0, rng.random(n)), np.arange(n, dtype=np.float64)[::-1].copy()]


def _bin_i64_columns(n):
    rng = np.random.default_rng(n + 1)
    return [rng.integers(-2 ** 62, 2 ** 62, n), rng.integers(0, 40, n)]


def _run_log_bin(K):
    out = {}
    for n in (70, 5000):
        cols = _bin_columns(n)
        bins, nb = K.vertical_log_bin(K.to_device(np.stack(cols)))
        out[f'{n}/bins'], out[f'{n}/nbins'] = host(K, bins), host(K, nb)
        typed = np.stack([c.view(np.float64) for c in _bin_i64_columns(n)] + cols[:2])
        bins, nb = K.vertical_log_bin(K.to_device(typed), 0.5, is_i64=[True, True, False, False])
        out[f'{n}/typed_bins'], out[f'{n}/typed_nbins'] = host(K, bins), host(K, nb)
    return out


def _want_log_bin():
    from oracle import ckernels
    want = {}
    for n in (70, 5000):
        cols = _bin_columns(n)
        exp = np.stack([ckernels.vertical_log_binning(c) for c in cols])
        want[f'{n}/bins'] = exp.astype(np.uint8)
        want[f'{n}/nbins'] = (exp.max(axis=1) + 1).astype(np.int32)
        # an int64 column is binned by its integer order: the ranks of its values as fp64 give the same bins
        ranked = [np.searchsorted(np.unique(c), c).astype(np.float64) for c in _bin_i64_columns(n)]
        exp = np.stack([ckernels.vertical_log_binning(c) for c in ranked + cols[:2]])
        want[f'{n}/typed_bins'] = exp.astype(np.uint8)
        want[f'{n}/typed_nbins'] = (exp.max(axis=1) + 1).astype(np.int32)
    return exact(want)


scenario('vertical_log_bin', ('grx_vertical_log_bin_typed', 'grx_memset'), _want_log_bin)(_run_log_bin)


def _run_log_bin_plain(K):
    """grx_vertical_log_bin (the entry point without type flags; the wrapper always takes the typed one)."""
    import ctypes
    out = {}
    for n in (70, 5000):
        block = K.to_device(np.stack(_bin_columns(n)))
        ncols = block.shape[0]
        bins = K.zeros((ncols, n), dtype=K.torch.uint8)
        nbins = K.zeros(ncols, dtype=K.torch.int32)
        ws, ws_bytes = K._workspace('grx_log_bin_workspace_bytes', n, ncols)
        K._lib.call('grx_vertical_log_bin', n, ncols, K._ptr(block), block.stride(0), ctypes.c_double(0.5), K._ptr(bins),
                    bins.stride(0), K._ptr(nbins), K._ptr(ws), ws_bytes, K._stream())
        out[f'{n}/bins'], out[f'{n}/nbins'] = host(K, bins), host(K, nbins)
    return out


def _want_log_bin_plain():
    return {k: v for k, v in _want_log_bin().items() if 'typed' not in k}


scenario('vertical_log_bin_plain', ('grx_vertical_log_bin', 'grx_memset'), _want_log_bin_plain)(_run_log_bin_plain)


def _cheb_bins():
    F, n = 97, 2000
    rng = np.random.default_rng(F)
    base = rng.integers(0, 20, size=(8, n)).astype(np.uint8)
    B = np.empty((F, n), dtype=np.uint8)
    for j in range(F):
        B[j] = base[j % 8]
        flip = rng.integers(0, n, size=(j // 8) * 3)
        B[j, flip] = np.minimum(B[j, flip] + (j // 8) % 4, 127)
    return B


def _run_chebyshev(K):
    B = _cheb_bins()
    F, n = B.shape
    Bd = K.to_device(B)
    cols = [Bd[j] for j in range(F)]
    h = n // 2 + 7
    return {'full': host(K, K.chebyshev(cols, n)), 'lo': host(K, K.chebyshev(cols, n, row_begin=0, row_end=h)),
            'hi': host(K, K.chebyshev(cols, n, row_begin=h, row_end=n)),
            'new': host(K, K.chebyshev(cols, n, first_new=90)), 'few': host(K, K.chebyshev(cols[:5], n))}


def _want_chebyshev():
    B = _cheb_bins().astype(np.int32)
    n = B.shape[1]
    h = n // 2 + 7

    def dist(X):
        return np.abs(X[:, None, :] - X[None, :, :]).max(axis=2).astype(np.int32)
    full = dist(B)
    mask = np.zeros_like(full, dtype=bool)
    mask[:, 90:] = True
    mask[90:, :] = True
    np.fill_diagonal(mask, False)
    want = exact({'full': full, 'lo': dist(B[:, :h]), 'hi': dist(B[:, h:]), 'few': dist(B[:5])})
    # first_new: the pairs with a column >= first_new are computed; above 96 columns whole 48-column groups are, so
    # the other entries are not defined
    want['new'] = (full, lambda got, w: np.array_equal(got[mask], w[mask]))
    return want


scenario('chebyshev', ('grx_chebyshev', 'grx_memset'), _want_chebyshev)(_run_chebyshev)


# ---- NMF --------------------------------------------------------------------------------------------------------------

NMF_SHAPES = ((17, 1, 1), (1001, 17, 3), (130, 113, 4), (300, 40, 32), (257, 480, 16))


def _nmf_inputs(shape):
    n, F, r = shape
    rng = np.random.default_rng(n + F)
    X = np.abs(rng.standard_normal((n, F))) * np.linspace(1, 50, F)
    T = rng.standard_normal((F, max(1, F - 2)))
    Z = rng.standard_normal((F, r))
    W0 = np.abs(rng.standard_normal((n, r))) + 0.1
    H0 = np.abs(rng.standard_normal((r, F))) + 0.1
    W0[::17, 1 % r] = 0.0
    W0[::29, :] = 0.0
    return X, T, Z, W0, H0


def _run_nmf_blocks(K):
    out = {}
    for shape in NMF_SHAPES:
        n, F, r = shape
        tag = f'{n}x{F}r{r}'
        X, T, Z, W0, H0 = _nmf_inputs(shape)
        Xd = K.to_device(np.ascontiguousarray(X.T))
        G, xsum = K.gram(Xd, n)
        out[f'{tag}/gram'], out[f'{tag}/xsum'] = G, np.array([xsum])
        out[f'{tag}/gram_T'] = K.gram(Xd, n, T)[0]
        out[f'{tag}/gram_lo'] = K.gram(Xd, n, None, 0, n // 2)[0]
        out[f'{tag}/gram_hi'] = K.gram(Xd, n, None, n // 2, n)[0]
        U, stats = K.project(Xd, n, Z)
        out[f'{tag}/project'], out[f'{tag}/stats'] = host(K, U, None, n), stats
        sign = np.where(np.arange(r) % 3 == 0, 0.0, np.where(np.arange(r) % 3 == 1, 1.0, -1.0))
        K.nndsvd_apply(U, n, sign, np.linspace(0.5, 3.0, r), 1e-6, 0.123)
        out[f'{tag}/nndsvd'] = host(K, U, None, n)
        st = K.NmfState(Xd, n, K.to_device(np.ascontiguousarray(W0.T)), H0)
        st.w_pass()
        out[f'{tag}/W1'], out[f'{tag}/AB'] = host(K, st.W, None, n), host(K, st.AB)
        st.h_update()
        out[f'{tag}/H1'] = host(K, st.H)
        out[f'{tag}/err'] = host(K, st.residual_sq())
        st.w_pass_next()
        out[f'{tag}/W2'], out[f'{tag}/H2'] = host(K, st.W, None, n), host(K, st.H)
        out[f'{tag}/kl'] = np.array([st.kl_cost(st.W, st.H)])
        st.iterate(3)
        out[f'{tag}/W5'], out[f'{tag}/H5'], out[f'{tag}/err5'] = host(K, st.W, None, n), host(K, st.H), host(K, st.err)
    return out


def _want_nmf_blocks():
    from oracle import rolx
    want = {}
    for shape in NMF_SHAPES:                                    # tolerances: tests/test_gpu_kernels.py:876-916
        n, F, r = shape
        tag = f'{n}x{F}r{r}'
        X, T, Z, W0, H0 = _nmf_inputs(shape)
        G = X.T @ X
        Y = X @ T
        want[f'{tag}/gram'] = (G, (1e-12, 0.0))
        want[f'{tag}/xsum'] = (np.array([X.sum()]), (1e-12, 0.0))
        want[f'{tag}/gram_T'] = (Y.T @ Y, (1e-10, 1e-10 * np.abs(Y.T @ Y).max()))
        want[f'{tag}/gram_lo'] = (X[:n // 2].T @ X[:n // 2], (1e-12, 0.0))
        want[f'{tag}/gram_hi'] = (X[n // 2:].T @ X[n // 2:], (1e-12, 0.0))
        Ue = X @ Z
        want[f'{tag}/project'] = (Ue.T, (1e-11, 1e-11 * np.abs(Ue).max()))
        den = W0 @ (H0 @ H0.T)
        W1 = W0 * ((X @ H0.T) / np.where(den == 0, rolx.EPSILON, den))
        want[f'{tag}/W1'] = (W1.T, (1e-12, 0.0))
        want[f'{tag}/AB'] = (np.concatenate([(W1.T @ X).ravel(), (W1.T @ W1).ravel()]), (1e-12, 0.0))
        den = (W1.T @ W1) @ H0
        H1 = H0 * ((W1.T @ X) / np.where(den == 0, rolx.EPSILON, den))
        want[f'{tag}/H1'] = (H1, (1e-12, 0.0))
        want[f'{tag}/err'] = (np.array([((X - W1 @ H1) ** 2).sum()]), (1e-11, 0.0))
    return want


scenario('nmf_blocks', ('grx_gram', 'grx_project', 'grx_nndsvd_apply', 'grx_nmf_w_pass', 'grx_nmf_w_pass_next',
                        'grx_nmf_h_update', 'grx_nmf_residual', 'grx_nmf_kl_cost', 'grx_nmf_iterate', 'grx_memset'),
         _want_nmf_blocks)(_run_nmf_blocks)


FIT_SHAPES = tuple(s for s in NMF_SHAPES if s[0] >= s[1])        # grx_nmf_init / grx_nmf_fit need n >= F


def _fit_inputs(shape):
    from oracle import rolx
    n, F, r = shape
    rng = np.random.default_rng(7 * n + F)
    X = rng.gamma(1.0, 1.0, size=(n, r)) @ rng.uniform(0.0, 2.0, size=(r, F)) + rng.uniform(0.0, 0.3, size=(n, F))
    omega = rolx.draw_omega(X.shape, r, np.random.RandomState(n))
    return X, omega


def _run_nmf_fit(K):
    out = {}
    for shape in FIT_SHAPES:
        n, F, r = shape
        tag = f'{n}x{F}r{r}'
        X, omega = _fit_inputs(shape)
        Xd = K.to_device(np.ascontiguousarray(X.T))
        W, H, xx = K.nmf_init(Xd, n, r, omega)
        out[f'{tag}/W0'], out[f'{tag}/H0'], out[f'{tag}/xx'] = host(K, W, None, n), host(K, H), np.array([xx])
        st = K.NmfState(Xd, n, W, H, x_sq_norm=xx)
        it = K.nmf_mu(st, 1e-4, 30)
        out[f'{tag}/W_mu'], out[f'{tag}/H_mu'], out[f'{tag}/it_mu'] = host(K, st.W, None, n), host(K, st.H), np.array([it])
        st, it = K.nmf_fit(Xd, n, r, omega, 1e-4, 30)
        out[f'{tag}/W_fit'], out[f'{tag}/H_fit'] = host(K, st.W, None, n), host(K, st.H)
        out[f'{tag}/it_fit'] = np.array([it])
        # grx_nmf_iterate_rows: a block of MU iterations on a row range (the sharded driver's step), no communicator
        st2 = K.NmfState(Xd, n, K.to_device(out[f'{tag}/W0']), out[f'{tag}/H0'])
        K._lib.call('grx_nmf_iterate_rows', n, F, r, K._ptr(st2.X), K._ld(st2.X), K._ptr(st2.W), K._ld(st2.W), 0, n,
                    K._ptr(st2.H), K._ptr(st2.AB), 2, None, K._ptr(st2.ws), st2.ws_bytes, K._stream())       # comm = NULL
        out[f'{tag}/W_rows'], out[f'{tag}/H_rows'] = host(K, st2.W, None, n), host(K, st2.H)
    return out


def _want_nmf_fit():
    from oracle import rolx
    want = {}
    for shape in FIT_SHAPES:
        n, F, r = shape
        tag = f'{n}x{F}r{r}'
        X, omega = _fit_inputs(shape)
        We, He, it = rolx.nmf(X, r, omega, 1e-4, 30)
        # FACTOR_RTOL = 1e-8 of tests/test_gpu_rolx.py: largest difference over largest entry; iteration counts ==
        want[f'{tag}/W_fit'] = (We.T, _relmax(1e-8))
        want[f'{tag}/H_fit'] = (He, _relmax(1e-8))
        want[f'{tag}/W_mu'] = (We.T, _relmax(1e-8))
        want[f'{tag}/H_mu'] = (He, _relmax(1e-8))
        if _fit_decided(X, r, omega, 1e-4, 30):
            want[f'{tag}/it_fit'] = (np.array([it]), EXACT)
            want[f'{tag}/it_mu'] = (np.array([it]), EXACT)
        want[f'{tag}/xx'] = (np.array([(X * X).sum()]), (1e-12, 0.0))
    return want


def _fit_decided(X, r, omega, tol, max_iter, min_margin=1e-6):
    """Is the iteration count of the oracle's fit a property of the input?  The stopping rule compares
    (prev - err) / err_init with tol every ten iterations.  The device's errors differ from numpy's by rounding (~1e-13
    relative), so a decision within min_margin (relative to tol, the MIN_MARGIN of tests/test_gpu_transform.py) of tol
    could go either way -- and on a table the start already factorises exactly (F = 1: any column is rank one) err_init
    is itself rounding noise (below min_margin of ||X||), and every decision is noise over noise."""
    from oracle import rolx
    W, H = rolx.nndsvda_init(X, r, omega)
    err_init = prev = rolx.frobenius_error(X, W, H)
    if err_init <= min_margin * float(np.sqrt((X * X).sum())):
        return False
    for _ in range(10, max_iter + 1, 10):
        W, H, _ = rolx.mu_iterations(X, W, H, 0.0, 10)
        err = rolx.frobenius_error(X, W, H)
        ratio = (prev - err) / err_init
        if abs(ratio - tol) <= min_margin * tol:
            return False
        if ratio < tol:
            break
        prev = err
    return True


def _relmax(bound):
    def close(got, want):
        return np.abs(got - want).max() / max(np.abs(want).max(), 1e-300) < bound
    return close


scenario('nmf_fit', ('grx_nmf_init', 'grx_nmf_mu', 'grx_nmf_fit', 'grx_nmf_iterate_rows', 'grx_memset'),
         _want_nmf_fit)(_run_nmf_fit)


TRANSFORM_SHAPES = ((17, 1, 1), (1001, 17, 3), (130, 113, 4), (300, 40, 32), (257, 480, 16))


def _transform_inputs(shape):
    n, F, r = shape
    rng = np.random.default_rng(100 * r + n)
    H = rng.uniform(0.0, 2.0, size=(r, F)) * (rng.uniform(size=(r, F)) < 0.6)
    H[:, 0] += 0.5
    X = rng.gamma(1.0, 1.0, size=(n, r)) @ H + rng.uniform(0.0, 0.3, size=(n, F))
    return X, H


def _run_transform(K):
    out = {}
    for shape in TRANSFORM_SHAPES:
        n, F, r = shape
        tag = f'{n}x{F}r{r}'
        X, H = _transform_inputs(shape)
        W, info = K.nmf_transform(K.to_device(np.ascontiguousarray(X.T)), n, H, 1e-4, 40)
        out[f'{tag}/W'], out[f'{tag}/it'] = host(K, W, None, n), np.array([info.n_iter])
    return out


def _want_transform():
    from tests import transform_oracle
    want = {}
    for shape in TRANSFORM_SHAPES:
        n, F, r = shape
        X, H = _transform_inputs(shape)
        Wo, it, info = transform_oracle.transform(X, H, 1e-4, 40)
        want[f'{n}x{F}r{r}/W'] = (Wo.T, _relmax(1e-8))          # FACTOR_RTOL of tests/test_gpu_transform.py:19
        if info['margin'] > 1e-6:                               # MIN_MARGIN there: the stopping decision is not a tie
            want[f'{n}x{F}r{r}/it'] = (np.array([it]), EXACT)
    return want


scenario('nmf_transform', ('grx_nmf_transform', 'grx_memset'), _want_transform)(_run_transform)


# ---- encode and roles ---------------------------------------------------------------------------------------------------

def _run_encode(K):
    out = {}
    for m in (1, 1000, 70001):
        v = np.abs(np.random.default_rng(m).standard_normal(m)) * np.random.default_rng(m + 1).choice([1e-3, 1.0, 40.0], m)
        for name, fn, k in (('lloyd', K.lloyd_max, 16), ('kmeans', K.kmeans1d, 8)):
            k = min(k, m)
            q, centers, info = fn(K.to_device(v), k)
            out[f'{m}/{name}_q'], out[f'{m}/{name}_c'] = host(K, q), host(K, centers, k)
            out[f'{m}/{name}_info'] = host(K, info)
    return out


scenario('encode', ('grx_lloyd_max', 'grx_kmeans1d', 'grx_memset'))(_run_encode)


ROLE_SHAPES = ((1, 1), (129, 9), (257, 32))


def _role_factor(n, r):
    rng = np.random.default_rng(n + r)
    G = rng.gamma(0.7, 1.0, size=(n, r))
    G[::7] = G[::7, :1]                                         # ties: the first maximum wins
    return G


def _run_roles(K):
    out = {}
    for n, r in ROLE_SHAPES:
        Gd = K.to_device(_role_factor(n, r))
        out[f'{n}x{r}/argmax'], out[f'{n}x{r}/share'] = host(K, K.role_argmax(Gd)), host(K, K.row_normalise(Gd))
    return out


def _want_roles():
    from oracle import rolx
    want = {}
    for n, r in ROLE_SHAPES:
        G = _role_factor(n, r)
        want[f'{n}x{r}/argmax'] = (rolx.dominant_role_index(G).astype(np.int32), EXACT)
        want[f'{n}x{r}/share'] = (rolx.role_percentage(G), EXACT)
    return want


scenario('roles', ('grx_role_argmax', 'grx_row_normalise'), _want_roles)(_run_roles)


NEIGHBOR_R = (1, 5, 32)


@functools.lru_cache(maxsize=None)
def _neighbor_graphs():
    from tests import neighbor_sense_oracle as nso
    out = {}
    for key in SYM_GRAPHS:
        n, row_ptr, col = sym(key)
        out[key] = (row_ptr, col, arc_values(row_ptr, col, 'float'))
    out['dw300'] = nso.csr_of(nso.adjacency(dw300(), True, 'out'), True)
    return out


def _run_neighbor_roles(K):
    from tests import neighbor_sense_oracle as nso
    out = {}
    for name, (row_ptr, col, w) in _neighbor_graphs().items():
        n = len(row_ptr) - 1
        csr = K.DeviceCSR(row_ptr, col, w)
        for r in NEIGHBOR_R:
            P = nso.memberships(n, r)
            Pd = K.to_device(P)
            for mode in ('sum', 'mean'):
                for weights in (None, csr.w):
                    tag = f'{name}/r{r}/{mode}/{"w" if weights is not None else "1"}'
                    out[tag] = host(K, K.neighbor_roles(csr, Pd, mode, weights))
            block = K.empty((2 * r, n))                         # the out= form: [P^T | N] for one Gram pass
            K.transpose(Pd, n, r, out=block[:r])
            K.neighbor_roles(csr, Pd, 'mean', out=block[r:2 * r])
            out[f'{name}/r{r}/block'] = host(K, block)
    return out


def _want_neighbor_roles():
    from tests import neighbor_sense_oracle as nso
    want = {}
    for name, (row_ptr, col, w) in _neighbor_graphs().items():
        n = len(row_ptr) - 1
        for r in NEIGHBOR_R:
            P = nso.memberships(n, r)
            for mode in ('sum', 'mean'):                        # tests/test_gpu_neighbor_sense.py: bit for bit
                want[f'{name}/r{r}/{mode}/w'] = nso.neighbor_roles(row_ptr, col, w, P, mode)
                want[f'{name}/r{r}/{mode}/1'] = nso.neighbor_roles(row_ptr, col, None, P, mode)
            want[f'{name}/r{r}/block'] = np.vstack([P.T, want[f'{name}/r{r}/mean/1']])
    return exact(want)


scenario('neighbor_roles', ('grx_neighbor_roles', 'grx_transpose'), _want_neighbor_roles)(_run_neighbor_roles)


# ---- ingest -------------------------------------------------------------------------------------------------------------

INGEST_CASES = ('n1_loop', 'n1_loop_w', 'path3_w', 'all_loops300_w', 'loops100_edges100', 'slots4096_n257',
                'dslots4097_n257', 'ring2049_iso')


def _ingest_arrays(K, result, nnz, m):
    perm, inv, row_ptr, out, tr = result
    got = {'perm': host(K, perm).astype(np.int64), 'inv': host(K, inv).astype(np.int64), 'row_ptr': np.asarray(row_ptr),
           'd_row_ptr': host(K, out.row_ptr), 'col': host(K, out.col, nnz), 'agg_col': host(K, out.agg_col, nnz)}
    if out.w is not None:
        got['w'] = bits(host(K, out.w, nnz))
    if tr is not None:
        got['t_row_ptr'], got['t_col'] = host(K, tr.row_ptr), host(K, tr.col, m)
        if tr.w is not None:
            got['t_w'] = bits(host(K, tr.w, m))
    return got


def _dup_edges(directed):
    """(n, src, dst, w) with every 7th edge listed twice, with the same weight: a duplicate writes one slot of the
    weight arrays only and the other stays as allocated -- the reason device_ingest zero-fills them."""
    if directed:
        n, src, dst, w = dw300_arrays()
    else:
        from tests import util
        n = 300
        src, dst, w = util.random_graph(300, 2000, 2, False, True, 5)
    again = np.arange(0, len(src), 7)
    return n, np.concatenate([src, src[again]]), np.concatenate([dst, dst[again]]), np.concatenate([w, w[again]])


def _run_ingest(K):
    from tests import ingest_oracle as io
    out = {}
    for name in INGEST_CASES:
        n, src, dst, w, directed = io.graph(name)
        ref = io.expected(name)
        result = K.device_ingest(n, src, dst, w, directed, ref.nnz)
        for key, a in _ingest_arrays(K, result, ref.nnz, ref.m).items():
            out[f'{name}/{key}'] = a
        if not directed:                                        # no host columns: oriented() is the device path
            o = result[3].oriented()
            o_nnz = int(io.expected_oriented(name).row_ptr[-1])
            out[f'{name}/o_row_ptr'], out[f'{name}/o_col'] = host(K, o.row_ptr), host(K, o.col, o_nnz)
            out[f'{name}/o_arc'] = host(K, o.arc, o_nnz)
    for directed in (True, False):
        n, src, dst, w = _dup_edges(directed)
        nnz = len(src) if directed else 2 * len(src) - int((src == dst).sum())
        result = K.device_ingest(n, src, dst, w, directed, nnz)
        for key, a in _ingest_arrays(K, result, nnz, len(src)).items():
            out[f'dup{int(directed)}/{key}'] = a
    return out


def _want_ingest():
    from tests import ingest_oracle as io
    want = {}
    for name in INGEST_CASES:                                   # tests/test_gpu_ingest_kernels.py: np.array_equal on all
        ref = io.expected(name)
        w = {'perm': ref.perm, 'inv': ref.inv, 'row_ptr': ref.row_ptr, 'd_row_ptr': ref.row_ptr, 'col': ref.col,
             'agg_col': ref.agg_col}
        if ref.w is not None:
            w['w'] = io.bits(ref.w)
        if ref.directed:
            w.update(t_row_ptr=ref.t_row_ptr, t_col=ref.t_col)
            if ref.t_w is not None:
                w['t_w'] = io.bits(ref.t_w)
        else:
            o = io.expected_oriented(name)
            w.update(o_row_ptr=o.row_ptr, o_col=o.col, o_arc=o.arc)
        for key, a in w.items():
            want[f'{name}/{key}'] = a
    return exact(want)


scenario('ingest', ('grx_ingest', 'grx_orient_count', 'grx_orient_fill', 'grx_memset'), _want_ingest)(_run_ingest)


# ---- measures: power iterations and local structure -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _power_graphs():
    from tests import measures_oracle as mo
    out = {}
    for key in SYM_GRAPHS:
        n, row_ptr, col = sym(key)
        out[key] = mo.CSR(row_ptr, col, None)
        out[key + '_w'] = mo.CSR(row_ptr, col, arc_values(row_ptr, col, 'float'))
    n, src, dst, w = dw300_arrays()
    out['dw300'] = mo.csr_from_arcs(n, src, dst, w)
    return out


def _run_power(K):
    from tests import measures_oracle as mo
    out = {}
    for name, g in _power_graphs().items():
        csr = K.DeviceCSR(g.row_ptr, g.col, g.w)
        S = K.to_device(mo.out_weight(g))
        for L in LANES:
            x, it = K.pagerank(csr, S, 0.85, 1e-10, 500, lanes=L)
            out[f'{name}/L{L}/pagerank'], out[f'{name}/L{L}/pagerank_it'] = host(K, x, g.n), np.array([it])
            if name == 'dw300':
                continue                                        # no eigenvector on this digraph: it need not converge
            x, it = K.eigenvector_centrality(csr, 1e-10, 2000, lanes=L)
            out[f'{name}/L{L}/eigenvector'], out[f'{name}/L{L}/eigenvector_it'] = host(K, x, g.n), np.array([it])
    return out


def _want_power():
    from tests import measures_oracle as mo
    want = {}
    for name, g in _power_graphs().items():
        pr, pr_it, pr_errs = mo.pagerank_ld(g.row_ptr, g.col, g.w, 0.85, 1e-10, 500)
        ev = None if name == 'dw300' else mo.eigenvector_ld(g.row_ptr, g.col, g.w, 1e-10, 2000)
        for L in LANES:                                         # tests/test_gpu_measures_kernels.py:53-55: mo.RTOL, atol 0
            want[f'{name}/L{L}/pagerank'] = (pr.astype(np.float64), (mo.RTOL, 0.0))
            if _decided(pr_errs, g.n * 1e-10):
                want[f'{name}/L{L}/pagerank_it'] = (np.array([pr_it]), EXACT)
            if ev is not None:
                want[f'{name}/L{L}/eigenvector'] = (ev[0].astype(np.float64), (mo.RTOL, 0.0))
                if _decided(ev[2], g.n * 1e-10):
                    want[f'{name}/L{L}/eigenvector_it'] = (np.array([ev[1]]), EXACT)
    return want


def _decided(errs, thresh):
    """No stopping decision of the long-double run is within 1e-6 relative of the threshold: fp64 rounding (1e-13
    relative, tests/test_measures_oracle_cpu.py) cannot move the iteration count."""
    errs = np.asarray(errs, dtype=np.float64)
    return bool(np.all(np.abs(errs - thresh) > 1e-6 * thresh))


scenario('power_iterations', ('grx_pagerank', 'grx_eigenvector_centrality'), _want_power)(_run_power)


@functools.lru_cache(maxsize=None)
def _local_graphs():
    from tests import measures_oracle as mo
    return {f'{n}/{int(loops)}': mo.local_graph(70 + n % 50, n, loops) for n in ROW_COUNTS for loops in (False, True)}


def _local_T(g, seed):
    from tests import measures_oracle as mo
    rng = np.random.default_rng(seed)
    own, _ = mo.loop_counts(g.row_ptr, g.col)
    dp = np.diff(g.row_ptr) - own
    T = rng.integers(0, np.maximum(dp * (dp - 1) // 2, 0) + 1)
    T[rng.random(g.n) < 0.2] = 0
    return T.astype(np.int64)


def _run_local(K):
    out = {}
    for name, g in _local_graphs().items():
        loops = name.endswith('/1')
        cl, es = K.local_structure(K.DeviceCSR(g.row_ptr, g.col), K.to_device(_local_T(g, g.n)), loops)
        out[f'{name}/clustering'], out[f'{name}/effective_size'] = host(K, cl, g.n), host(K, es, g.n)
    return out


def _want_local():
    from tests import measures_oracle as mo
    want = {}
    for name, g in _local_graphs().items():                     # tests/test_gpu_measures_kernels.py:156-160: bit equal
        own, nl = mo.loop_counts(g.row_ptr, g.col)
        cl, es = mo.local_measures(np.diff(g.row_ptr), own, _local_T(g, g.n), nl)
        want[f'{name}/clustering'], want[f'{name}/effective_size'] = (cl, _same_bits_or_nan), (es, _same_bits_or_nan)
    return want


scenario('local_structure', ('grx_local_structure_measures',), _want_local)(_run_local)


# ---- measures: BFS and shortest paths by weight -----------------------------------------------------------------------

def _sources(n):
    """{tag: sources}: one source, and 65 (one more than a 64-source batch or word) where the graph has them."""
    order = np.random.default_rng(9).permutation(n)
    return {'s1': order[:1], 's65': order[:65]} if n >= 65 else {'s1': order[:1]}


@functools.lru_cache(maxsize=None)
def _path_graphs():
    """name -> (out CSR, in CSR or None), each (row_ptr, col int64, w) with 'integer' weights (exact sums)."""
    from tests import weighted_betweenness_oracle as wo
    out = {}
    for key in SYM_GRAPHS:
        n, row_ptr, col = sym(key)
        out[key] = ((row_ptr, col.astype(np.int64), arc_values(row_ptr, col, 'integer')), None)
    _, o, i = wo.csr_pair(dw300())
    out['dw300'] = (o, i)
    return out


def _dev_pair(K, o, i, weighted, L):
    out = with_lanes(K, K.DeviceCSR(o[0], o[1], o[2] if weighted else None), L)
    tr = None if i is None else with_lanes(K, K.DeviceCSR(i[0], i[1], i[2] if weighted else None), L)
    return out, tr


def _run_bfs(K):
    out = {}
    for name, (o, i) in _path_graphs().items():
        n = len(o[0]) - 1
        for L in LANES:
            d_out, d_in = _dev_pair(K, o, i, False, L)
            pull = d_out if d_in is None else d_in
            for s_tag, sources in _sources(n).items():
                tag = f'{name}/L{L}/{s_tag}'
                out[f'{tag}/bc'] = host(K, K.betweenness(d_out, d_in, sources, False, 1.0, batch=64), n)
                out[f'{tag}/bc_end'] = host(K, K.betweenness(d_out, d_in, sources, True, 0.5), n)
                for key, t in zip(('reach', 'dsum', 'harmonic'), K.distance_sums(pull, sources, words=1)):
                    out[f'{tag}/{key}'] = host(K, t, n)
                if d_in is None:                                # the bounds hold on a symmetric CSR only
                    ecc, reach, lower, upper = K.eccentricity_pass(pull, sources, 1, want_upper=True)
                    out[f'{tag}/ecc'], out[f'{tag}/ecc_reach'] = host(K, ecc), host(K, reach, n)
                    out[f'{tag}/lower'], out[f'{tag}/upper'] = host(K, lower, n), host(K, upper, n)
                    ecc2, reach2, lower2, upper2 = K.eccentricity_pass(pull, sources[::-1], 2, bounds=(lower, upper))
                    out[f'{tag}/ecc2'], out[f'{tag}/ecc_reach2'] = host(K, ecc2), host(K, reach2, n)
                    out[f'{tag}/lower2'], out[f'{tag}/upper2'] = host(K, lower2, n), host(K, upper2, n)
                    ecc3, _, lower3, upper3 = K.eccentricity_pass(pull, sources, 1)
                    assert upper3 is None
                    out[f'{tag}/ecc3'], out[f'{tag}/lower3'] = host(K, ecc3), host(K, lower3, n)
    return out


def _want_bfs():
    from tests import betweenness_oracle as bo, closeness_oracle as co, eccentricity_oracle as eo
    want = {}
    for name, (o, i) in _path_graphs().items():
        n = len(o[0]) - 1
        pull = o if i is None else i
        for s_tag, sources in _sources(n).items():
            # raw sums: directed=True, normalized=False leaves the oracle's bc unscaled (tests/test_gpu_betweenness.py:81,
            # rtol = bo.RTOL, atol 0)
            bc = bo.betweenness_arrays(o[0], o[1], sources, True, normalized=False, endpoints=False)
            bc_end = 0.5 * bo.betweenness_arrays(o[0], o[1], sources, True, normalized=False, endpoints=True)
            # the kernel pulls over `pull`: the oracle walks the transposed arcs from each source
            walk = co.transpose(pull[0], pull[1])
            reach, dsum, harm = co.distance_sums(walk[0], walk[1], sources, in_adjacency=(pull[0], pull[1]))
            harm = np.array([co.harm_to_float(h) for h in harm])
            for L in LANES:
                tag = f'{name}/L{L}/{s_tag}'
                want[f'{tag}/bc'], want[f'{tag}/bc_end'] = (bc, (bo.RTOL, 0.0)), (bc_end, (bo.RTOL, 0.0))
                # tests/test_gpu_closeness.py:205-208: == on all three
                want[f'{tag}/reach'], want[f'{tag}/dsum'], want[f'{tag}/harmonic'] = (reach, EXACT), (dsum, EXACT), (harm, EXACT)
                if i is None:                                   # tests/test_gpu_eccentricity.py `_same`: ==
                    w1 = eo.eccentricity_pass(pull[0], pull[1], sources, want_upper=True)
                    w2 = eo.eccentricity_pass(pull[0], pull[1], sources[::-1], w1[2], w1[3])
                    w3 = eo.eccentricity_pass(pull[0], pull[1], sources)
                    for key, a in (('ecc', w1[0]), ('ecc_reach', w1[1]), ('lower', w1[2]), ('upper', w1[3]), ('ecc2', w2[0]),
                                   ('ecc_reach2', w2[1]), ('lower2', w2[2]), ('upper2', w2[3]), ('ecc3', w3[0]),
                                   ('lower3', w3[2])):
                        want[f'{tag}/{key}'] = (np.asarray(a), EXACT)
    return want


scenario('bfs_measures', ('grx_betweenness', 'grx_distance_sums', 'grx_eccentricity', 'grx_memset'), _want_bfs)(_run_bfs)


def _run_weighted_paths(K):
    out = {}
    for name, (o, i) in _path_graphs().items():
        n = len(o[0]) - 1
        for L in LANES:
            d_out, d_in = _dev_pair(K, o, i, True, L)
            pull = d_out if d_in is None else d_in
            for s_tag, sources in _sources(n).items():
                tag = f'{name}/L{L}/{s_tag}'
                for matrix in (False, True):
                    reach, dsum, harmonic, far, ecc, dist, rounds = K.weighted_distances(pull, sources, 16, matrix)
                    m = '_m' if matrix else ''
                    for key, t in (('reach', reach), ('dsum', dsum), ('harmonic', harmonic), ('far', far)):
                        out[f'{tag}/{key}{m}'] = host(K, t, n)
                    out[f'{tag}/ecc{m}'], out[f'{tag}/rounds{m}'] = host(K, ecc), np.array([rounds])
                    if matrix:
                        out[f'{tag}/dist'] = host(K, dist)
                bc, rounds, levels = K.weighted_betweenness(d_out, d_in, sources, True, 0.25, 16)
                out[f'{tag}/wbc'], out[f'{tag}/wbc_info'] = host(K, bc, n), np.array([rounds, levels])
    return out


def _want_weighted_paths():
    from tests import sssp_oracle as so, weighted_betweenness_oracle as wo
    want = {}
    for name, (o, i) in _path_graphs().items():
        n = len(o[0]) - 1
        pull = o if i is None else i
        for s_tag, sources in _sources(n).items():
            w = so.weighted_distances(pull[0], pull[1], pull[2], sources, 16)
            for L in LANES:
                tag = f'{name}/L{L}/{s_tag}'
                for m in ('', '_m'):                            # tests/test_gpu_weighted_distances.py:103-105: bytes
                    for key, a in zip(('reach', 'dsum', 'harmonic', 'far', 'ecc'), w):
                        want[f'{tag}/{key}{m}'] = (a, EXACT)
                    want[f'{tag}/rounds{m}'] = (np.array([w[6]]), EXACT)
                want[f'{tag}/dist'] = (w[5], EXACT)
                # tests/test_gpu_weighted_betweenness.py:120-126: rtol = wo.RTOL, atol 0; rounds and levels ==
                inn = pull
                bc, rounds, levels = wo.betweenness_arrays(o, inn, sources, True, 0.25, 16, 32 * L, 32 * L)
                want[f'{tag}/wbc'] = (bc, (wo.RTOL, 0.0))
                want[f'{tag}/wbc_info'] = (np.array([rounds, levels]), EXACT)
    return want


scenario('weighted_paths', ('grx_weighted_distances', 'grx_weighted_betweenness'), _want_weighted_paths)(_run_weighted_paths)


# ---- measures: peeling and component structure ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _dw300_structure():
    """(out row_ptr, out col, in row_ptr, in col) of dw300's distinct arcs without self-loops."""
    from tests import kcore_oracle as ko
    G = dw300().copy()
    G.remove_edges_from([(v, v) for v in list(G) if G.has_edge(v, v)])
    return ko.graph_csrs(G)[1:]


def _run_peeling(K):
    out = {}
    for key in SYM_GRAPHS:
        n, row_ptr, col = sym(key)
        for L in LANES:
            csr = with_lanes(K, K.DeviceCSR(row_ptr, col), L)
            tag = f'{key}/L{L}'
            count, parent, label, n_comp = K.biconnected(csr)
            out[f'{tag}/bic_count'], out[f'{tag}/bic_parent'] = host(K, count, n), host(K, parent, n)
            out[f'{tag}/bic_label'], out[f'{tag}/bic_n'] = host(K, label, n), np.array([n_comp])
            out[f'{tag}/bic_count_only'] = host(K, K.biconnected(csr, want_forest=False)[0], n)
            core, onion, rounds = K.core_numbers(csr)
            out[f'{tag}/core'], out[f'{tag}/onion'], out[f'{tag}/core_rounds'] = host(K, core, n), host(K, onion, n), np.array([rounds])
            out[f'{tag}/core_only'] = host(K, K.core_numbers(csr, want_onion=False)[0], n)
            arc, node, rounds, levels = K.truss_numbers(csr, lanes=L)
            out[f'{tag}/arc_truss'], out[f'{tag}/node_truss'] = host(K, arc, int(row_ptr[-1])), host(K, node, n)
            out[f'{tag}/truss_info'] = np.array([rounds, levels])
            out[f'{tag}/arc_truss_only'] = host(K, K.truss_numbers(csr, want_node=False, lanes=L)[0], int(row_ptr[-1]))
    o_ptr, o_col, i_ptr, i_col = _dw300_structure()
    n = len(o_ptr) - 1
    for L in LANES:
        d_out, d_in = with_lanes(K, K.DeviceCSR(o_ptr, o_col), L), with_lanes(K, K.DeviceCSR(i_ptr, i_col), L)
        core, onion, rounds = K.core_numbers(d_out, d_in)
        out[f'dw300/L{L}/core'], out[f'dw300/L{L}/onion'] = host(K, core, n), host(K, onion, n)
        out[f'dw300/L{L}/core_rounds'] = np.array([rounds])
    return out


def _want_peeling():
    from tests import biconnected_oracle as bio, kcore_oracle as ko, truss_oracle as to
    want = {}
    for key in SYM_GRAPHS:
        n, row_ptr, col = sym(key)
        b = bio.biconnected(row_ptr, col.astype(np.int64))
        c = ko.core_numbers(row_ptr, col)
        t = to.truss_numbers(row_ptr, col)
        for L in LANES:
            tag = f'{key}/L{L}'
            # tests/test_gpu_biconnected.py:108-112: count and parent ==, the labels only in their sign
            want[f'{tag}/bic_count'], want[f'{tag}/bic_parent'] = b.count, b.parent
            want[f'{tag}/bic_count_only'], want[f'{tag}/bic_n'] = b.count, np.array([b.n_components])
            want[f'{tag}/core'], want[f'{tag}/onion'], want[f'{tag}/core_only'] = c.core, c.onion, c.core
            want[f'{tag}/core_rounds'] = np.array([c.n_rounds])
            want[f'{tag}/arc_truss'], want[f'{tag}/node_truss'] = t.arc_truss, t.node_truss
            want[f'{tag}/arc_truss_only'], want[f'{tag}/truss_info'] = t.arc_truss, np.array([t.n_rounds, t.n_levels])
    c = ko.core_numbers(*_dw300_structure())
    for L in LANES:
        want[f'dw300/L{L}/core'], want[f'dw300/L{L}/onion'] = c.core, c.onion
        want[f'dw300/L{L}/core_rounds'] = np.array([c.n_rounds])
    return exact(want)


scenario('peeling', ('grx_biconnected', 'grx_core_numbers', 'grx_truss_numbers'), _want_peeling)(_run_peeling)


# ---- measures: row intersections --------------------------------------------------------------------------------------

def _run_rowjoin(K):
    from tests import clustering_oracle as clo, structural_holes_oracle as sho
    out = {}
    for key in SYM_GRAPHS:
        n, row_ptr, col = sym(key)
        nnz = int(row_ptr[-1])
        for kind in ('unweighted', 'float'):
            z = arc_values(row_ptr, col, kind)
            csr = K.DeviceCSR(row_ptr, col, z)
            for L in LANES:
                tag = f'{key}/{kind}/L{L}'
                con, es, loc = K.structural_holes(csr, csr.w, None, True, True, True, lanes=L)
                out[f'{tag}/constraint'], out[f'{tag}/effective_size'] = host(K, con, n), host(K, es, n)
                out[f'{tag}/local'] = host(K, loc, nnz)
                c, t = K.clustering(csr, csr.w, None, float(z.max()) if z is not None and len(z) else 1.0, True, lanes=L)
                out[f'{tag}/clustering'], out[f'{tag}/triangles'] = host(K, c, n), host(K, t, n)
    G = dw300()
    row_ptr, col, z, out_ptr = sho.mutual_csr(G, 'weight')
    n, nnz = len(row_ptr) - 1, int(row_ptr[-1])
    csr = K.DeviceCSR(row_ptr, col, z)
    _, _, fwd, bwd, max_weight = clo.directional_csr(G, 'weight')
    for L in LANES:
        tag = f'dw300/L{L}'
        con, es, loc = K.structural_holes(csr, csr.w, K.to_device(out_ptr), True, True, True, lanes=L)
        out[f'{tag}/constraint'], out[f'{tag}/effective_size'] = host(K, con, n), host(K, es, n)
        out[f'{tag}/local'] = host(K, loc, nnz)
        c, t = K.clustering(csr, K.to_device(fwd), K.to_device(bwd), max_weight, True, lanes=L)
        out[f'{tag}/clustering'], out[f'{tag}/triangles'] = host(K, c, n), host(K, t, n)
    return out


def _want_rowjoin():
    from tests import clustering_oracle as clo, structural_holes_oracle as sho
    want = {}

    def holes(tag, w, row_ptr):
        # structural_holes_oracle.assert_close: NaNs in the same places, RTOL on constraint and local, ES_ATOL * max(d, 1)
        for k, key in enumerate(('constraint', 'effective_size', 'local')):
            want[f'{tag}/{key}'] = (w[k], lambda g, x, k=k: _passes(sho.assert_close, tuple(g if j == k else None for j in range(3)),
                                                                    tuple(x if j == k else None for j in range(3)), row_ptr))

    def clus(tag, w):                                           # clustering_oracle.assert_close: zeros in place, RTOL
        want[f'{tag}/clustering'] = (w[0], lambda g, x: _passes(clo.assert_close, g, x))
        want[f'{tag}/triangles'] = (w[1], lambda g, x: _passes(clo.assert_close, g, x))

    for key in SYM_GRAPHS:
        n, row_ptr, col = sym(key)
        for kind in ('unweighted', 'float'):
            z = arc_values(row_ptr, col, kind)
            h = sho.sparse(row_ptr, col, z)
            c = clo.sparse(row_ptr, col, z, None, float(z.max()) if z is not None and len(z) else 1.0)
            for L in LANES:
                holes(f'{key}/{kind}/L{L}', h, row_ptr)
                clus(f'{key}/{kind}/L{L}', c)
    G = dw300()
    row_ptr, col, z, out_ptr = sho.mutual_csr(G, 'weight')
    h = sho.sparse(row_ptr, col, z, out_ptr)
    c = clo.sparse(*clo.directional_csr(G, 'weight'))
    for L in LANES:
        holes(f'dw300/L{L}', h, row_ptr)
        clus(f'dw300/L{L}', c)
    return want


def _passes(check, *args):
    try:
        check(*args)
    except AssertionError:
        return False
    return True


scenario('rowjoin', ('grx_structural_holes', 'grx_clustering'), _want_rowjoin)(_run_rowjoin)


def _run_squares(K):
    out = {}
    for key in SYM_GRAPHS:
        n, row_ptr, col = sym(key)
        csr = K.DeviceCSR(row_ptr, col)
        for L in LANES:
            tag = f'{key}/L{L}'
            c, q, p = K.square_clustering(csr, want_counts=True, lanes=L)
            out[f'{tag}/c4'], out[f'{tag}/squares'], out[f'{tag}/potential'] = host(K, c, n), host(K, q, n), host(K, p, n)
            out[f'{tag}/c4_only'] = host(K, K.square_clustering(csr, lanes=L)[0], n)
            orbits, non, tri = K.graphlet_orbits(csr, True, True, lanes=L)
            out[f'{tag}/orbits'], out[f'{tag}/noninduced'] = host(K, orbits), host(K, non)
            out[f'{tag}/arc_triangles'] = host(K, tri, int(row_ptr[-1]))
            out[f'{tag}/orbits_only'] = host(K, K.graphlet_orbits(csr, lanes=L)[0])
    return out


def _want_squares():
    from tests import graphlet_oracle as go
    want = {}
    for key in SYM_GRAPHS:
        n, row_ptr, col = sym(key)
        Q, P, C = sqo.square_clustering(row_ptr, col)
        g = go.orbits(row_ptr, col)
        for L in LANES:                                         # tests/test_gpu_square_clustering.py:150-151 and
            tag = f'{key}/L{L}'                                 # tests/test_gpu_graphlets.py:140-142: ==
            want[f'{tag}/c4'], want[f'{tag}/c4_only'], want[f'{tag}/squares'], want[f'{tag}/potential'] = C, C, Q, P
            want[f'{tag}/orbits'], want[f'{tag}/orbits_only'] = g.orbits, g.orbits
            want[f'{tag}/noninduced'], want[f'{tag}/arc_triangles'] = g.noninduced, g.arc_triangles
    return exact(want)


scenario('squares_and_graphlets', ('grx_square_clustering', 'grx_graphlet_orbits'), _want_squares)(_run_squares)


# ---- n = 0 ------------------------------------------------------------------------------------------------------------

def _run_empty(K):
    """The entry points that accept n = 0 (or no columns): zero-byte allocations between their guards."""
    out = {}
    none = K.DeviceCSR(np.array([0]), np.zeros(0, np.int32))
    out['argmax'] = host(K, K.role_argmax(K.to_device(np.ones((0, 4)))))
    out['share'] = host(K, K.row_normalise(K.to_device(np.ones((0, 4)))))
    out['neighbor_roles'] = host(K, K.neighbor_roles(none, K.empty((0, 3)), 'mean'))
    bins, nb = K.vertical_log_bin(K.zeros((1, 0)))
    out['bins'], out['nbins'] = host(K, bins), host(K, nb)
    index = K.to_device(np.zeros(5, dtype=np.int32))
    out['permute'], out['gather'] = host(K, K.permute_columns([], index, 5)), host(K, K.gather_columns([], 5), None, 5)
    out['sort'] = host(K, K.sort_columns(K.zeros((0, 7))))
    H = np.abs(np.random.default_rng(3).standard_normal((2, 6)))
    W, info = K.nmf_transform(K.zeros((6, 1)), 0, H)
    out['transform_it'] = np.array([info.n_iter])
    rows = K.DeviceCSR(np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32))            # five rows, no arcs
    orbits, non, tri = K.graphlet_orbits(rows, True, True)
    out['orbits'], out['noninduced'] = host(K, orbits), host(K, non)
    X = K.to_device(np.ones((3, 5)))
    prows, ldr = K.pack_rows([X[c] for c in range(3)], 5)
    for name, t in (('median', K.aggregate_median(rows, prows, 0, ldr)), ('prod', K.aggregate_prod(rows, prows, 0, ldr)),
                    ('count', K.aggregate_count(rows, 0)), ('sum_mean', K.aggregate(rows, prows, 0, ldr))):
        out[f'f0/{name}'] = np.array(tuple(t.shape))
    return out


def _want_empty():
    return exact({'argmax': np.zeros(0, np.int32), 'share': np.zeros((0, 4)), 'neighbor_roles': np.zeros((3, 0)),
                  'bins': np.zeros((1, 0), np.uint8), 'nbins': np.array([0], np.int32), 'permute': np.zeros((0, 5)),
                  'gather': np.zeros((0, 5)), 'sort': np.zeros((0, 7)), 'transform_it': np.array([0]),
                  'orbits': np.zeros((15, 5), np.int64), 'noninduced': np.zeros((15, 5), np.int64),
                  'f0/median': np.array([0, 5]), 'f0/prod': np.array([0, 5]), 'f0/count': np.array([0, 5]),
                  'f0/sum_mean': np.array([0, 5])})


scenario('empty', ('grx_graphlet_orbits', 'grx_nmf_transform', 'grx_vertical_log_bin_typed'), _want_empty)(_run_empty)


# ---- the driver ---------------------------------------------------------------------------------------------------------

def _run_refex(K):
    """grx_refex_run through RecursiveFeatureExtractor (native loop) on karate and BA 300.  BA 300 starts from a 64 KiB
    arena, so the run grows it through the GROW_FN callback -- an allocation of kernels.py like any other."""
    from graphrole_amd import RecursiveFeatureExtractor, synth
    from tests import util
    from tests.test_gpu_refex import _graph_for
    out = {}
    g = util.load_refex('karate')
    G, kwargs = _graph_for('karate', g)
    fe = RecursiveFeatureExtractor(G, **kwargs)
    X = fe.extract_features()
    out['karate/values'], out['karate/generations'] = X.values.astype(np.float64), np.array([fe.generation_count])
    fe = RecursiveFeatureExtractor(synth.ba_graph(300, 3, seed=1), max_generations=4)
    fe._arena = [K.empty(1 << 16, dtype=K.torch.uint8)]
    X = fe.extract_features()
    assert len(fe._arena) > 1, 'the arena did not grow'
    out['ba300/values'], out['ba300/generations'] = X.values.astype(np.float64), np.array([fe.generation_count])
    return out


def _want_refex():
    from graphrole_amd import synth
    from oracle import refex
    from tests import util
    g = util.load_refex('karate')
    G = synth.ba_graph(300, 3, seed=1)
    og = refex.OracleGraph(labels=G.labels, row_ptr=G.row_ptr, col=G.col, w=None, directed=False, num_edges=G.num_edges,
                           adj_col=G.adj_col)
    ref = refex.extract_features(og, max_generations=4, fast=True)
    # tests/test_gpu_refex.py `_check_values`: == on an unweighted graph (karate's fixture is the unweighted club)
    return exact({'karate/values': g['final_values'], 'karate/generations': np.array([int(g['generation_count'])]),
                  'ba300/values': ref.values, 'ba300/generations': np.array([ref.generation_count])})


scenario('refex_run', ('grx_refex_run',), _want_refex)(_run_refex)
