"""
High-precision array oracle of csrc/grx_measures.hip and the case list of tests/test_gpu_measures_kernels.py.

pagerank_ld / eigenvector_ld run networkx 3.4.2's two loops (pagerank_alg.py::_pagerank_scipy with err < N * tol,
eigenvector.py::eigenvector_centrality; same start vector, same stop rule) on CSR arrays of the in-adjacency in
np.longdouble, so they say which side of a comparison is closer to the true value and they run at shapes networkx
cannot hold.  pagerank_f64 / eigenvector_f64 are the same statements in float64: tests/test_measures_oracle_cpu.py
uses them to show that a correct fp64 implementation stays a factor ten inside the 1e-12 the GPU tests allow.
local_measures restates the header comment of `local_measures` in the kernel file one IEEE operation at a time.
No reference code, no networkx objects.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

assert np.finfo(np.longdouble).eps < 1e-18, \
    'tests/measures_oracle.py needs an extended-precision np.longdouble (x87 80-bit or wider) on this host'

LD = np.longdouble
HUB_FACTOR = 32                                                # rows longer than HUB_FACTOR * lanes are hub rows
MS_BATCH = 8                                                   # iterations the library enqueues per read-back
RTOL = 1e-12                                                   # the project's tolerance for the two power iterations


class NotConverged(RuntimeError):
    def __init__(self, max_iter, errs):
        super().__init__(f'power iteration failed to converge within {max_iter} iterations')
        self.iterations, self.errs = max_iter, errs


class CSR(NamedTuple):
    """In-adjacency: row v lists the sources u of the arcs u -> v, ascending; w is None for an unweighted graph."""
    row_ptr: np.ndarray
    col: np.ndarray
    w: Optional[np.ndarray]

    @property
    def n(self):
        return len(self.row_ptr) - 1


def _row_sums(values, row_ptr):
    """Per-row sums of `values` (one per arc); np.add.reduceat returns a[i] for an empty segment, so only the
    non-empty rows are reduced (an empty row shares its start with the next non-empty one)."""
    n = len(row_ptr) - 1
    out = np.zeros(n, dtype=values.dtype)
    nonempty = row_ptr[1:] > row_ptr[:-1]
    if len(values) and nonempty.any():
        out[nonempty] = np.add.reduceat(values, row_ptr[:-1][nonempty])
    return out


def out_weight(csr: CSR, dtype=np.float64):
    """Out-weight of every node (networkx: S = A.sum(axis=1)) from the in-adjacency: col holds the sources."""
    w = np.ones(len(csr.col), dtype=dtype) if csr.w is None else csr.w.astype(dtype)
    out = np.zeros(csr.n, dtype=dtype)
    np.add.at(out, csr.col, w)
    return out


def _pagerank(row_ptr, col, w, alpha, tol, max_iter, dtype):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n = len(row_ptr) - 1
    wv = None if w is None else np.asarray(w).astype(dtype)
    S = out_weight(CSR(row_ptr, col, w), dtype)
    dangling = S == 0
    sinv = np.zeros(n, dtype=dtype)
    sinv[~dangling] = dtype(1) / S[~dangling]
    alpha, N = dtype(alpha), dtype(n)
    p = dtype(1) / N
    thresh = N * dtype(tol)
    x = np.full(n, p, dtype=dtype)
    errs = []
    for it in range(1, max_iter + 1):
        y = x * sinv
        contrib = y[col] if wv is None else y[col] * wv
        xn = alpha * (_row_sums(contrib, row_ptr) + x[dangling].sum() * p) + (dtype(1) - alpha) * p
        err = np.abs(xn - x).sum()
        errs.append(err)
        x = xn
        if err < thresh:
            return x, it, errs
    raise NotConverged(max_iter, errs)


def _eigenvector(row_ptr, col, w, tol, max_iter, dtype):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n = len(row_ptr) - 1
    wv = None if w is None else np.asarray(w).astype(dtype)
    N = dtype(n)
    thresh = N * dtype(tol)
    x = np.full(n, dtype(1) / N, dtype=dtype)
    errs = []
    for it in range(1, max_iter + 1):
        contrib = x[col] if wv is None else x[col] * wv
        z = x + _row_sums(contrib, row_ptr)
        norm = np.sqrt((z * z).sum())
        xn = z / (norm if norm != 0 else dtype(1))             # networkx: math.hypot(*x.values()) or 1
        err = np.abs(xn - x).sum()
        errs.append(err)
        x = xn
        if err < thresh:
            return x, it, errs
    raise NotConverged(max_iter, errs)


def pagerank_ld(row_ptr, col, w, alpha=0.85, tol=1e-6, max_iter=100):
    """(x, iterations, errs) of networkx's _pagerank_scipy over the in-adjacency, in np.longdouble."""
    return _pagerank(row_ptr, col, w, alpha, tol, max_iter, LD)


def eigenvector_ld(row_ptr, col, w, tol=1e-6, max_iter=100):
    """(x, iterations, errs) of networkx's eigenvector_centrality over the in-adjacency, in np.longdouble."""
    return _eigenvector(row_ptr, col, w, tol, max_iter, LD)


def pagerank_f64(row_ptr, col, w, alpha=0.85, tol=1e-6, max_iter=100):
    return _pagerank(row_ptr, col, w, alpha, tol, max_iter, np.float64)


def eigenvector_f64(row_ptr, col, w, tol=1e-6, max_iter=100):
    return _eigenvector(row_ptr, col, w, tol, max_iter, np.float64)


def max_rel_dev(got, want):
    """Largest |got - want| / |want| (0 / 0 counts as 0): what assert_allclose(rtol, atol=0) bounds."""
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    diff = np.abs(got - want)
    den = np.abs(want)
    ok = den > 0
    if not ok.all() and np.any(diff[~ok] != 0):
        return float('inf')
    return float((diff[ok] / den[ok]).max()) if ok.any() else 0.0


def local_measures(deg, own_loop, T, loop_neighbours):
    """(clustering, effective_size) as the kernel's `local_measures` states them, in float64, one operation each:
    d' = deg - own_loop; clustering = 0 if T == 0 else fl(2T) / fl(d' (d' - 1)); effective size = NaN if deg == 0 or
    d' == 0 else fl(d') - fl(2 (T + loop_neighbours)) / fl(d')."""
    deg = np.asarray(deg, dtype=np.int64)
    own = np.asarray(own_loop, dtype=np.int64)
    T = np.asarray(T).astype(np.int64)
    nl = np.asarray(loop_neighbours, dtype=np.int64)
    dp = deg - own
    cl = np.zeros(len(deg), dtype=np.float64)
    nz = T != 0
    cl[nz] = (2 * T[nz]).astype(np.float64) / (dp[nz] * (dp[nz] - 1)).astype(np.float64)
    es = np.full(len(deg), np.nan, dtype=np.float64)
    ok = (deg != 0) & (dp != 0)
    es[ok] = dp[ok].astype(np.float64) - (2 * (T[ok] + nl[ok])).astype(np.float64) / dp[ok].astype(np.float64)
    return cl, es


def loop_counts(row_ptr, col):
    """(own_loop, loop_neighbours) of an undirected CSR: whether v lists itself, and how many of its other
    neighbours list themselves."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n = len(row_ptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    own = np.bincount(rows[rows == col], minlength=n).astype(np.int64)
    other = rows != col
    nl = np.bincount(rows[other], weights=own[col[other]], minlength=n).astype(np.int64)
    return own, nl


# ---- synthetic graphs ------------------------------------------------------------------------------------------

def csr_from_arcs(n, src, dst, w=None):
    """In-adjacency CSR of the arcs src -> dst (duplicates dropped, the first weight kept)."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    key = dst * n + src
    key, first = np.unique(key, return_index=True)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // n, minlength=n), out=row_ptr[1:])
    return CSR(row_ptr, (key % n).astype(np.int32), None if w is None else np.asarray(w, dtype=np.float64)[first])


def synthetic_csr(seed, n, avg_degree, *, directed=False, weighted=False, hubs=(), out_hubs=(), dangling=0,
                  isolated=0, self_loops=0):
    """
    Random graph as an in-adjacency CSR.  The first len(hubs) nodes are hub rows of exactly the given lengths (their
    arcs come from distinct ordinary nodes, and nothing else points at them), the next len(out_hubs) nodes send that
    many arcs (directed graphs), the last `isolated` nodes have no arc at all and the `dangling` nodes before them
    (directed graphs) receive arcs but send none.  The ordinary nodes in between get about avg_degree * n / 2 random
    edges (undirected) or avg_degree * n random arcs (directed) on top of a ring through all of them -- the graph of
    the ordinary nodes and hubs is (strongly) connected, so no eigenvector entry decays until it underflows in
    float64 -- and the first `self_loops` of them a self-loop.  avg_degree = 0 gives no arc at all.  Weights are
    U(0.1, 4), one per undirected edge.
    """
    rng = np.random.default_rng(seed)
    first = len(hubs) + len(out_hubs)
    last = n - isolated - dangling                              # ordinary nodes: first .. last - 1
    ordinary = np.arange(first, last, dtype=np.int64)
    assert len(ordinary) >= 1 and all(h <= len(ordinary) for h in tuple(hubs) + tuple(out_hubs))
    src, dst = [], []
    if len(ordinary) > 1 and avg_degree > 0:
        src.append(ordinary)
        dst.append(np.roll(ordinary, -1))
        m = int(avg_degree * n) // (1 if directed else 2)
        receivers = np.arange(first, n - isolated, dtype=np.int64)  # dangling nodes receive
        u = rng.choice(ordinary, size=m)
        v = rng.choice(receivers if directed else ordinary, size=m)
        keep = u != v
        src.append(u[keep])
        dst.append(v[keep])
    for h, length in enumerate(hubs):
        src.append(rng.choice(ordinary, size=length, replace=False))
        dst.append(np.full(length, h, dtype=np.int64))
    for g, length in enumerate(out_hubs):
        src.append(np.full(length, len(hubs) + g, dtype=np.int64))
        dst.append(rng.choice(ordinary, size=length, replace=False))
    loops = ordinary[:self_loops]
    src.append(loops)
    dst.append(loops)
    src, dst = np.concatenate(src), np.concatenate(dst)
    if not directed:
        lo, hi = np.minimum(src, dst), np.maximum(src, dst)
        key = np.unique(lo * n + hi)
        lo, hi = key // n, key % n
        w = rng.uniform(0.1, 4.0, size=len(lo)) if weighted else None
        sym = lo != hi
        src, dst = np.concatenate([lo, hi[sym]]), np.concatenate([hi, lo[sym]])
        w = None if w is None else np.concatenate([w, w[sym]])
    else:
        w = rng.uniform(0.1, 4.0, size=len(src)) if weighted else None
    return csr_from_arcs(n, src, dst, w)


def transpose(csr: CSR) -> CSR:
    """Out-adjacency of an in-adjacency (and back)."""
    n = csr.n
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(csr.row_ptr))
    return csr_from_arcs(n, rows, csr.col.astype(np.int64), csr.w)


def natural_lanes(csr: CSR) -> int:
    """The lane-group width kernels.DeviceCSR picks from the average row length."""
    avg = len(csr.col) / max(csr.n, 1)
    return 4 if avg < 12 else 8 if avg < 24 else 16 if avg < 48 else 32


# ---- the cases of tests/test_gpu_measures_kernels.py -----------------------------------------------------------

BOUNDARY_HUBS = (128, 129, 256, 257, 512, 513, 1024, 1025)     # 32 L and 32 L + 1 for L = 4, 8, 16, 32

#: name -> synthetic_csr arguments
GRAPHS = {
    # average in-degree in each of the four tiers of DeviceCSR, no hub rows
    'tier4': dict(seed=11, n=2000, avg_degree=6),
    'tier8': dict(seed=12, n=2000, avg_degree=16, weighted=True),
    'tier16': dict(seed=13, n=2000, avg_degree=32, directed=True, weighted=True),
    'tier32': dict(seed=14, n=2000, avg_degree=64),
    # hub rows on and just past every boundary, ~300 arcs (just over one 256-thread pass) and 20 000 arcs
    'hubs': dict(seed=21, n=25000, avg_degree=6, hubs=BOUNDARY_HUBS + (300, 20000)),
    'hubs_w': dict(seed=22, n=25000, avg_degree=6, weighted=True, hubs=BOUNDARY_HUBS + (300, 20000)),
    'hubs_iso': dict(seed=25, n=25000, avg_degree=6, hubs=BOUNDARY_HUBS + (300, 20000), isolated=5),
    # directed: in-hubs, separate out-hubs, dangling and isolated nodes, a self-loop
    'hubs_dir': dict(seed=23, n=25000, avg_degree=6, directed=True, hubs=BOUNDARY_HUBS + (300, 20000),
                     out_hubs=(300, 20000), dangling=40, isolated=5, self_loops=1),
    'hubs_dir_w': dict(seed=24, n=25000, avg_degree=6, directed=True, weighted=True,
                       hubs=BOUNDARY_HUBS + (300, 20000), out_hubs=(300, 20000), dangling=40, isolated=5,
                       self_loops=1),
    # every row a hub at L = 4: 160 nodes, ~150 neighbours each
    'all_hubs': dict(seed=31, n=160, avg_degree=400),
    'all_hubs_w': dict(seed=32, n=160, avg_degree=400, weighted=True),
    # no arc at all: every node dangling, x stays 1 / N
    'all_dangling': dict(seed=33, n=1000, avg_degree=0),
    # a self-loop on every one of the first 3 ordinary nodes of a dangling-free graph
    'self_loop': dict(seed=34, n=50, avg_degree=6, self_loops=3),
    # the row loop takes a second trip (n > 2048 * 256 / L) for L = 32 and L = 4, the element loops at n > 2048 * 256
    # (the second trips of the other measures' launches: tests/test_gpu_second_trip.py, which lists all such tests)
    'rows32': dict(seed=41, n=2048 * 8 + 5, avg_degree=5),
    'rows4': dict(seed=42, n=2048 * 64 + 9, avg_degree=5, weighted=True),
    'elements': dict(seed=43, n=2048 * 256 + 77, avg_degree=4, hubs=(300,)),
}
for _L in (4, 8, 16, 32):
    for _d in (-1, 0, 1):
        GRAPHS[f'n{256 // _L + _d}'] = dict(seed=50 + _L + _d, n=256 // _L + _d, avg_degree=3)
for _n in (1, 2, 3):
    GRAPHS[f'n{_n}'] = dict(seed=60 + _n, n=_n, avg_degree=2)


@functools.lru_cache(maxsize=None)
def graph(name) -> CSR:
    return synthetic_csr(**GRAPHS[name])


class Case(NamedTuple):
    id: str
    graph: str
    measure: str                                               # 'pagerank' | 'eigenvector'
    lanes: Optional[int] = None                                # None = DeviceCSR's own choice
    alpha: float = 0.85
    tol: float = 1e-6
    stop_at: Optional[int] = None                              # tol is chosen so that the oracle stops here

    @property
    def family(self):
        return self.id.split('-')[0]


def _cases():
    out = []
    both = ('pagerank', 'eigenvector')
    for m in both:
        for g in ('tier4', 'tier8', 'tier16', 'tier32'):
            out.append(Case(f'tier-{g}-{m}', g, m))
        for g in ('hubs', 'hubs_w', 'hubs_dir', 'hubs_dir_w'):
            for L in (4, 8, 16, 32):
                out.append(Case(f'hubs-{g}-L{L}-{m}', g, m, lanes=L))
        for g in ('hubs_dir', 'hubs_dir_w'):
            out.append(Case(f'directed-{g}-{m}', g, m))
        for g in ('all_hubs', 'all_hubs_w'):
            out.append(Case(f'allhubs-{g}-{m}', g, m, lanes=4))
        # a width other than the graph's own: the hub list must follow it (tier32: rows of 65 .. 128 arcs, no hub at
        # its own 32 lanes; all_hubs_w: every row a hub at 4 lanes, none at its own 32)
        for g in ('tier32', 'all_hubs_w'):
            for L in (4, 8, 16, 32):
                out.append(Case(f'forced-{g}-L{L}-{m}', g, m, lanes=L))
        for L in (4, 8, 16, 32):
            for d in (-1, 0, 1):
                out.append(Case(f'size-n{256 // L + d}-L{L}-{m}', f'n{256 // L + d}', m, lanes=L))
        for n in (1, 2, 3):
            out.append(Case(f'size-n{n}-{m}', f'n{n}', m))
        out.append(Case(f'grid-rows32-{m}', 'rows32', m, lanes=32))
        out.append(Case(f'grid-rows4-{m}', 'rows4', m))
        out.append(Case(f'grid-elements-{m}', 'elements', m))
        for tol in (1e-3, 1e-10):
            out.append(Case(f'args-tol{tol:g}-{m}', 'tier8', m, tol=tol))
        for k in (1, 7, 8, 9, 16, 17):
            out.append(Case(f'iters-{k}-{m}', 'tier4', m, stop_at=k))
    out.append(Case('dangling-all-pagerank', 'all_dangling', 'pagerank'))
    out.append(Case('dangling-hubs_iso-pagerank', 'hubs_iso', 'pagerank'))
    out.append(Case('dangling-self_loop-pagerank', 'self_loop', 'pagerank'))
    for alpha in (0.5, 0.99):
        out.append(Case(f'args-alpha{alpha:g}-pagerank', 'tier8', 'pagerank', alpha=alpha))
    return out


CASES = _cases()
MAX_ITER = 5000                                                # never the limit: every case converges well inside


def tol_for_count(errs, k, n):
    """A tol that stops the loop at iteration k exactly: N * tol is the geometric mean of err_k and the smallest
    error before it (twice err_1 for k = 1), so both sit far from the threshold."""
    errs = [float(e) for e in errs]
    if k == 1:
        return 2.0 * errs[0] / n
    before = min(errs[:k - 1])
    assert errs[k - 1] < before, (k, errs[:k])
    return float(np.sqrt(errs[k - 1] * before)) / n


@functools.lru_cache(maxsize=None)
def _run(graph_name, measure, alpha, tol, max_iter, dtype):
    g = graph(graph_name)
    if measure == 'pagerank':
        return _pagerank(g.row_ptr, g.col, g.w, alpha, tol, max_iter, dtype)
    return _eigenvector(g.row_ptr, g.col, g.w, tol, max_iter, dtype)


def run(case: Case, tol, max_iter=MAX_ITER, dtype=LD):
    """(x, iterations, errs) of a case at `tol` in `dtype` (cached: cases that differ in `lanes` share it)."""
    return _run(case.graph, case.measure, case.alpha if case.measure == 'pagerank' else 0.0, tol, max_iter, dtype)


@functools.lru_cache(maxsize=None)
def case_tol(case: Case) -> float:
    if case.stop_at is None:
        return case.tol
    g = graph(case.graph)
    _, _, errs = run(case._replace(stop_at=None), 1e-9)        # runs past iteration 17
    assert len(errs) > case.stop_at
    return tol_for_count(errs, case.stop_at, g.n)


def expected(case: Case):
    """(x, iterations, errs) of the long-double oracle for a case."""
    return run(case, case_tol(case))


def add_edges(csr: CSR, pairs) -> CSR:
    """An unweighted undirected CSR plus the edges `pairs` ((v, v) = a self-loop)."""
    n = csr.n
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(csr.row_ptr))
    a = np.array([p[0] for p in pairs], dtype=np.int64)
    b = np.array([p[1] for p in pairs], dtype=np.int64)
    return csr_from_arcs(n, np.concatenate([csr.col.astype(np.int64), a, b]), np.concatenate([rows, b, a]))


def local_graph(seed, n, loops) -> CSR:
    """Undirected graph for grx_local_structure_measures: random edges, (n > 6000) a 5 000-neighbour hub, one
    isolated node, one node of degree 1 and -- with `loops` -- a self-loop on half of the ordinary nodes (so about
    half the hub's neighbours carry one), on the hub itself and on a node whose only neighbour is itself."""
    spare = min(3, n - 1)
    hubs = (5000,) if n > 6000 else ()
    core = n - spare - len(hubs)
    g = synthetic_csr(seed, n, 4, hubs=hubs, isolated=spare, self_loops=core // 2 if loops else 0)
    extra = []
    if spare >= 2:
        extra.append((n - 2, len(hubs)))                       # degree 1, its neighbour carries a loop
    if loops:
        extra.append((n - 1, n - 1))
        if hubs:
            extra.append((0, 0))
    return add_edges(g, extra) if extra else g
