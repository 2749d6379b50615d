"""
A plain numpy twin of the Lloyd-Max quantiser as graphrole_amd/csrc/grx_quant.hip states it, stage by stage, and
the named cases the device is compared with (tests/test_gpu_lloyd_max.py; the twin itself is pinned without a GPU by
tests/test_lloyd_max_oracle_cpu.py).

Arithmetic.  Everything is done in ``np.longdouble`` on ``s - pivot``, pivot = sorted[m // 2].  For fp64 inputs that
subtraction is exact in long double (64-bit significand) as long as the exponents of s and pivot are within 11 bits of
each other, which every case here is; all later quantities (prefix sums, costs, centres, midpoints) are functions of
the centred values alone, so the twin is translation-invariant by construction: x and x + t (t an exact shift) give the
same edges, the same centred centres, and pivots that differ by t.  ``quantise_float64`` runs the same code in
``np.float64``; the CPU test demands that the two agree on every discrete decision of every case, and that every
decision has a margin >= 1e-9 (about four orders of magnitude above m * u, u = 2**-53, for these sizes), so that the
order in which the device adds its fp64 prefix sums cannot flip one.

Stages, each returned in the result:
  1. stable ascending sort                                   -> order, pivot
  2. prefix sums P of s - pivot, P2 of (s - pivot)^2, Gp of cbrt(s[i+1] - s[i])^2 (last term 0), m + 1 entries each
  3. micro-cell edges (m <= 1024: one value per cell; 1024 < m <= 8192: the cap is 8192, one value per cell again;
     larger m: 1024 targets total * b / 1024, first i with Gp[i] >= target, clamped to [1, m - 1], made strictly
     increasing, last edge m)                                -> cell_edges, margin 'cells'
     (The upper clamp can never act: Gp[m] == Gp[m - 1] because the last term is 0 and target <= total, so the search
     ends at an index <= m - 1.  The twin asserts that.  The lower clamp acts only when total == 0: constant input.)
  4. k <= 256 or m <= 8192: dynamic programming over the cells, min(k, cells) layers, D_j[i] = min over j <= mm < i
     of D_{j-1}[mm] + max(0, (P2[i] - P2[mm]) - (P[i] - P[mm])^2 / n), the smallest mm winning ties, surplus clusters
     empty at the top                                        -> dp_edges, dp_cost, margin 'dp', dp_ties
     Layers are evaluated with the monotone-argmin divide and conquer (the cost is Monge: leftmost minimisers do not
     decrease with i), O(cells log cells) per layer instead of O(cells^2), and only over the band of (j, i) that can
     lie on a path to D_{k-1}[cells]; `dp_plain` is the O(k cells^2) statement and the CPU test compares the two.
     The arg-min of every row ON the backtracked path is then taken over the whole row, as the kernel does, which
     also gives the runner-up gap.
     otherwise (k > 256 and m > 8192): companding start, k cells of equal Gp mass (same search, same clamp; made
     non-decreasing, so duplicates are empty clusters); with m <= k: edge b = min(b, m)
  5. Lloyd: centres (P[b] - P[a]) / n, empty clusters inherit the centre below; per iteration
     nh[j] = upper_bound(s, 0.5 * (c[j] + c[j + 1])) (a value on a midpoint goes down), nh[k - 1] = m; stop when
     nh == hi, else hi = nh and the non-empty clusters get new centres (empty ones keep theirs); at most max_iter
     updates                                                 -> hi_history, c_history, iterations, margin 'lloyd'
  6. bounds = midpoints of the final centres; info = {iterations, non-empty, distinct (among non-empty, consecutive)};
     label = first boundary >= v                             -> centers, info, labels, margin 'assign'

Margins (the smallest over the case is kept, with the number of exact ties):
  cells   |target - Gp[lo - 1]| and |Gp[lo] - target|, relative to total
  dp      for every arg-min on the backtracked path, (runner-up - best) / optimum of the whole problem; a row with
          one candidate has none.  Exact ties (runner-up == best) are counted in dp_ties with their value.
  lloyd   for every boundary search of every iteration, min |s[idx - 1] - bnd|, |s[idx] - bnd| relative to s[-1] - s[0]
  assign  the same for the final bounds (they differ from the last searched midpoints when max_iter cuts the loop)

The rounding bound of the translation test.  Let x_i = s_i - pivot, S1 = sum |x_i|, S2 = sum x_i^2, R = max |x_i|.
A device prefix sum adds at most m terms, each rounded once or twice, in some order: |e_i| = |fl(P[i]) - P[i]| <=
(m + 1) u S1 and |f_i| = |fl(P2[i]) - P2[i]| <= (m + 2) u S2 to first order in u.  For a partition with edges
0 = b_0 <= ... <= b_k = m the DP minimises  F^ = sum_c (P2^[b_{c+1}] - P2^[b_c]) - (P^[b_{c+1}] - P^[b_c])^2 / n_c.
The f terms telescope to f_m - f_0, the same for every partition, so they do not influence the choice.  The e terms
give, to first order, -2 sum_c mu_c (e_{b_{c+1}} - e_{b_c}) with mu_c the centred cluster mean; summing by parts,
sum_c mu_c (e_{b_{c+1}} - e_{b_c}) = mu_last e_m - sum_j (mu_j - mu_{j-1}) e_{b_j}, and the means increase with j, so
its size is at most (|mu_last| + mu_last - mu_first) max |e| <= 3 R (m + 1) u S1.  The roundings of the O(1)
operations per cluster and of the k additions are each relative to a term <= P2[b_{c+1}] - P2[b_c], which sum to S2:
at most (k + 5) u S2 <= m u S2 for k + 5 <= m.  So |F^ - F - const| <= E = 6 (m + 1) u R S1 + m u S2 for every
partition, and the partition the device chooses is within 2 E of the optimum:
      objective(device) - optimum <= c m u S2,    c = 2 + 13 rho,   rho = R S1 / S2 >= 1
(12 (m + 1) / m <= 13 for m >= 12).  rho is a shape factor of the data, 3/2 for uniform values with the pivot in the
middle; `rounding_bound` computes it from the data.  Without the pivot the same derivation holds with x_i = s_i, and
S2 grows with the square of the offset: that is the defect the translation cases show on uncentred sums.
"""
import collections
import functools
from types import SimpleNamespace

import numpy as np

Q_CELLS = 1024
QC_BIG = 8192
Q_MAX_BINS = 256
U = 2.0 ** -53
MARGIN = 1e-9


# ------------------------------------------------------------------------------------------------ stages
def _cost(cp, cp2, cn, mm, i):
    n = cn[i] - cn[mm]
    sm = cp[i] - cp[mm]
    return np.maximum((cp2[i] - cp2[mm]) - sm * sm / n, 0)


def _equal_mass_search(Gp, m, parts, dtype):
    """first i with Gp[i] >= total * b / parts for b = 1 .. parts - 1, clamped to [1, m - 1]; the margin of the search"""
    total = Gp[m]
    b = np.arange(1, parts)
    target = total * b.astype(dtype) / dtype(parts)
    lo = np.searchsorted(Gp, target, side='left')
    if total > 0:
        assert lo.min() >= 1 and lo.max() <= m - 1, 'the clamp acts only on constant input'
        margin = float(min(((Gp[lo] - target) / total).min(), ((target - Gp[lo - 1]) / total).min())) if len(b) else np.inf
    else:
        assert not lo.any()
        margin = np.inf                                    # every target and every Gp is exactly 0
    return np.clip(lo, 1, m - 1), margin


def _cell_edges(Gp, m, dtype):
    want = QC_BIG if Q_CELLS < m <= QC_BIG else Q_CELLS
    if m <= want:
        return np.arange(m + 1, dtype=np.int64), np.inf
    e, margin = _equal_mass_search(Gp, m, want, dtype)
    ce = [0]
    for r in list(e) + [m]:
        if r > ce[-1]:
            ce.append(int(r))
    return np.array(ce, dtype=np.int64), margin


def _companding_edges(Gp, m, k, dtype):
    if m <= k:
        raw, margin = np.minimum(np.arange(1, k), m), np.inf
    else:
        raw, margin = _equal_mass_search(Gp, m, k, dtype)
    edges = np.concatenate([[0], raw, [m]]).astype(np.int64)
    return np.maximum.accumulate(edges), margin


def _monotone_layer(Dprev, Dcur, j, ilo, ihi, cp, cp2, cn):
    """Dcur[i] = min over j <= mm < i of Dprev[mm] + cost(mm, i) for ilo <= i <= ihi, leftmost minimisers, by divide and
    conquer over i, one level of the recursion at a time"""
    a, b = np.array([ilo]), np.array([ihi])
    olo, ohi = np.array([j]), np.array([ihi - 1])
    while a.size:
        mid = (a + b) // 2
        lens = np.minimum(ohi, mid - 1) - olo + 1
        starts = np.cumsum(lens) - lens
        seg = np.repeat(np.arange(a.size), lens)
        mm = np.arange(int(lens.sum())) - starts[seg] + olo[seg]
        v = Dprev[mm] + _cost(cp, cp2, cn, mm, mid[seg])
        best = np.minimum.reduceat(v, starts)
        hit = np.flatnonzero(v == best[seg])
        _, first = np.unique(seg[hit], return_index=True)
        opt = mm[hit[first]]
        Dcur[mid] = best
        L, R = a <= mid - 1, mid + 1 <= b
        a, b, olo, ohi = (np.concatenate([a[L], mid[R] + 1]), np.concatenate([mid[L] - 1, b[R]]),
                          np.concatenate([olo[L], opt[R]]), np.concatenate([opt[L], ohi[R]]))


def _dp_tables(ce, P, P2, k, dtype, plain):
    nb = len(ce) - 1
    kk = min(k, nb)
    cp, cp2, cn = P[ce], P2[ce], ce.astype(dtype)
    D = np.full(nb + 1, np.inf, dtype=dtype)
    D[0] = 0
    tables = [D]
    for j in range(kk):
        ilo, ihi = (j + 1, nb) if plain else (j + 1, nb - (kk - 1 - j))
        cur = np.full(nb + 1, np.inf, dtype=dtype)
        if j == 0:
            i = np.arange(ilo, ihi + 1)
            cur[i] = _cost(cp, cp2, cn, np.zeros_like(i), i)
        elif plain:
            for i in range(ilo, ihi + 1):
                mm = np.arange(j, i)
                cur[i] = (tables[-1][mm] + _cost(cp, cp2, cn, mm, i)).min()
        else:
            _monotone_layer(tables[-1], cur, j, ilo, ihi, cp, cp2, cn)
        tables.append(cur)
    return tables, (cp, cp2, cn), nb, kk


def _dp(ce, P, P2, k, dtype, plain=False):
    tables, (cp, cp2, cn), nb, kk = _dp_tables(ce, P, P2, k, dtype, plain)
    optimum = tables[kk][nb]
    edges = np.full(k + 1, ce[nb], dtype=np.int64)          # surplus clusters stay empty
    gaps, ties = [], []
    i = nb
    for j in range(kk - 1, -1, -1):
        mm = np.arange(j, i)
        v = tables[j][mm] + _cost(cp, cp2, cn, mm, i)
        a = int(np.argmin(v))                               # the first minimum: the smallest mm wins ties
        if len(v) > 1:
            second = np.delete(v, a).min()
            if second == v[a]:
                ties.append(float(v[a]))
            else:
                gaps.append(float((second - v[a]) / optimum) if optimum > 0 else np.inf)
        i = j + a
        edges[j] = ce[i]
    assert i == 0
    return edges, optimum, (min(gaps) if gaps else np.inf), ties


def _upper_bound_margin(s, bnd, idx, span):
    m = len(s)
    d = np.full(len(bnd), np.inf)
    below, above = idx > 0, idx < m
    d[below] = np.abs(s[idx[below] - 1] - bnd[below]).astype(np.float64)
    d[above] = np.minimum(d[above], np.abs(s[idx[above]] - bnd[above]).astype(np.float64))
    if not len(d):
        return np.inf
    if span > 0:
        return float(d.min() / float(span))
    return 0.0 if d.min() == 0 else np.inf


def _lloyd(s, P, edges, k, max_iter, dtype):
    m = len(s)
    span = s[-1] - s[0]

    def means(hi, c):
        lo = np.concatenate([[0], hi[:-1]])
        live = hi > lo
        c = c.copy()
        c[live] = (P[hi[live]] - P[lo[live]]) / (hi[live] - lo[live]).astype(dtype)
        return c, live

    hi = edges[1:].copy()
    assert hi[0] > 0, 'the first cluster of a start is never empty'
    c, live = means(hi, np.zeros(k, dtype=dtype))
    c = c[np.maximum.accumulate(np.where(live, np.arange(k), 0))]     # empty clusters inherit the centre below them
    hi_history, c_history, margin = [], [c.copy()], np.inf
    it = 0
    while it < max_iter:
        bnd = 0.5 * (c[:-1] + c[1:])
        idx = np.searchsorted(s, bnd, side='right')
        margin = min(margin, _upper_bound_margin(s, bnd, idx, span))
        nh = np.concatenate([idx, [m]]).astype(np.int64)
        if np.array_equal(nh, hi):
            break
        hi = nh
        c, live = means(hi, c)
        hi_history.append(hi.copy())
        c_history.append(c.copy())
        it += 1
    return hi, c, it, hi_history, c_history, margin


def _first_boundary_not_below(bounds, v):
    """the assign kernels' binary search: first j in [0, k - 1) with bounds[j] >= v, else k - 1"""
    lo = np.zeros(len(v), dtype=np.int64)
    up = np.full(len(v), len(bounds), dtype=np.int64)
    while True:
        act = lo < up
        if not act.any():
            return lo
        mid = (lo + up) >> 1
        less = np.zeros(len(v), dtype=bool)
        less[act] = bounds[mid[act]] < v[act]
        lo = np.where(act & less, mid + 1, lo)
        up = np.where(act & ~less, mid, up)


def quantise(values, k, max_iter=300, dtype=np.longdouble, plain_dp=False):
    """The whole quantiser on a flat fp64 array; every stage's result and every margin (module docstring)."""
    x = np.ascontiguousarray(values, dtype=np.float64).ravel()
    m = len(x)
    assert 1 <= k <= m and max_iter >= 0
    r = SimpleNamespace(m=m, k=k, max_iter=max_iter)
    r.order = np.argsort(x, kind='stable')
    raw = x[r.order]
    r.pivot = raw[m // 2]
    s = raw.astype(dtype) - dtype(r.pivot)
    gap = np.zeros(m, dtype=dtype)
    gap[:-1] = raw[1:].astype(dtype) - raw[:-1].astype(dtype)
    g = np.cbrt(gap)
    zero = np.zeros(1, dtype=dtype)
    P = np.concatenate([zero, np.cumsum(s)])
    P2 = np.concatenate([zero, np.cumsum(s * s)])
    Gp = np.concatenate([zero, np.cumsum(g * g)])
    r.s, r.P, r.P2, r.Gp = s, P, P2, Gp
    r.margins = {}
    r.dp_ties = []
    if k <= Q_MAX_BINS or m <= QC_BIG:
        r.cell_edges, r.margins['cells'] = _cell_edges(Gp, m, dtype)
        r.dp_edges, r.dp_cost, r.margins['dp'], r.dp_ties = _dp(r.cell_edges, P, P2, k, dtype, plain_dp)
        r.start_edges = r.dp_edges
    else:
        r.cell_edges = r.dp_edges = None
        r.start_edges, r.margins['cells'] = _companding_edges(Gp, m, k, dtype)
    hi, c, r.iterations, r.hi_history, r.c_history, r.margins['lloyd'] = _lloyd(s, P, r.start_edges, k, max_iter, dtype)
    r.hi = hi
    r.centers_centred = c
    r.centers = (dtype(r.pivot) + c).astype(np.float64)
    lo = np.concatenate([[0], hi[:-1]])
    r.counts = hi - lo
    live = c[r.counts > 0]
    r.nonempty = int(len(live))
    r.distinct = int(1 + np.count_nonzero(live[1:] != live[:-1])) if len(live) else 0
    r.info = (r.iterations, r.nonempty, r.distinct)
    bounds = 0.5 * (c[:-1] + c[1:])
    r.bounds_centred = bounds
    r.margins['assign'] = _upper_bound_margin(s, bounds, np.searchsorted(s, bounds, side='right'), s[-1] - s[0])
    sorted_labels = _first_boundary_not_below(bounds, s)
    r.labels = np.empty(m, dtype=np.int64)
    r.labels[r.order] = sorted_labels
    return r


def quantise_float64(values, k, max_iter=300):
    """The same code in fp64 (the sums in index order): what the device computes up to the order of its additions."""
    return quantise(values, k, max_iter, dtype=np.float64)


def dp_plain(values, k):
    """The DP stage by its O(k cells^2) statement, every (j, i): edges and optimum of the start."""
    r = quantise(values, k, 0, plain_dp=True)
    return r.dp_edges, r.dp_cost


def objective(values, labels):
    """sum of squared distances to the label means, long double on centred values"""
    x = np.ascontiguousarray(values, dtype=np.float64).ravel()
    xc = x.astype(np.longdouble) - np.longdouble(np.sort(x)[len(x) // 2])
    order = np.argsort(labels, kind='stable')
    lab = np.asarray(labels)[order]
    starts = np.flatnonzero(np.concatenate([[True], lab[1:] != lab[:-1]]))
    sums = np.add.reduceat(xc[order], starts)
    counts = np.diff(np.concatenate([starts, [len(x)]]))
    mean = np.repeat(sums / counts, counts)
    d = xc[order] - mean
    return (d * d).sum()


def rounding_bound(values):
    """c m u S2 of the module docstring, c = 2 + 13 R S1 / S2, for the fp64 prefix sums of values - pivot"""
    x = np.ascontiguousarray(values, dtype=np.float64).ravel()
    xc = np.abs(x.astype(np.longdouble) - np.longdouble(np.sort(x)[len(x) // 2]))
    S1, S2, R = xc.sum(), (xc * xc).sum(), xc.max()
    if S2 == 0:
        return np.longdouble(0)
    return (2 + 13 * R * S1 / S2) * len(x) * U * S2


# ------------------------------------------------------------------------------------------------ cases
Case = collections.namedtuple('Case', 'name recipe m k max_iter seed exact shift')
Case.__new__.__defaults__ = (300, 0, False, 0.0)


def _uniform(rng, m):
    return rng.rand(m)


def _gamma(rng, m):
    return rng.gamma(2.0, 1.0, m)


def _randint5(rng, m):
    return rng.randint(0, 5, m).astype(np.float64)


def _randint20(rng, m):
    return rng.randint(0, 20, m).astype(np.float64)


def _constant(rng, m):
    return np.full(m, 2.5)


def _grid4(rng, m):
    """the integers 0 .. N - 1 and the outlier N - 1 + 1e6, four times each, shuffled (m = 4 N + 4).  Cell edges and
    upper bounds fall between groups, so every cluster is a run of whole groups: its mean is a half-integer, every
    midpoint a quarter-integer -- exact in any binary format -- and one in four is an integer, a value of the data.
    The outlier is a cluster of its own; its gap takes most of the Gp mass, so a micro-cell holds about twelve groups
    and lies off the grid's symmetry: the DP's optimum over cells is unique and not a Lloyd fixed point."""
    n = m // 4 - 1
    return rng.permutation(np.repeat(np.concatenate([np.arange(n, dtype=np.float64), [n - 1 + 1.0e6]]), 4))


def _cubed(rng, m):
    return rng.rand(m) ** 3                                # uneven density, bounded gaps: no empty companding cell


def _signed(rng, m):
    return rng.randn(m) * 3


def _lognormal1(rng, m):
    return rng.lognormal(0, 1, m)


def _lognormal2(rng, m):
    return rng.lognormal(0, 2, m)


def _dyadic(rng, m):
    return rng.randint(0, 1 << 20, m) / 1024.0             # integers / 2**10 in [0, 1024)


def _cases():
    out = []
    # prefix tiles (Q_TILE = 2048, one wavefront scans 512): exact path, a scan error changes the partition
    for m in (1, 2, 7, 2047, 2048, 2049, 4097):
        for k in (1, 2, 5):
            if k <= m:
                out.append(Case(f'tiles_m{m}_k{k}', _uniform, m, k, seed=1))
    # cell cap 1024 -> 8192 -> micro-cells
    for m, k in ((1024, 16), (1025, 16), (8192, 4), (8193, 4)):
        out.append(Case(f'cellcap_m{m}_k{k}', _gamma, m, k, seed=2))
    # 256 -> 257 levels: exact DP into the small / the big Lloyd kernel; micro-cell DP / companding start
    for m, k in ((3000, 256), (3000, 257), (20000, 256), (20000, 257)):
        out.append(Case(f'levels_m{m}_k{k}', _gamma if m == 3000 else _cubed, m, k, seed=3 if m == 3000 else 20))
    for m in (1, 300, 1500, 10000):
        out.append(Case(f'k_eq_m_{m}', _uniform, m, m, seed=4))
    # fewer distinct values than levels (integers: all arithmetic exact, the DP's ties are exact zeros)
    out.append(Case('few_distinct_randint5_m5000_k8', _randint5, 5000, 8, seed=5, exact=True))
    out.append(Case('few_distinct_randint20_m20000_k32', _randint20, 20000, 32, seed=5, exact=True))
    out.append(Case('constant_m3000_k4', _constant, 3000, 4, exact=True))
    out.append(Case('constant_m9000_k4', _constant, 9000, 4, exact=True))      # total == 0: the lower clamp of the cells
    out.append(Case('midpoint_ties_grid_m8220_k4', _grid4, 8220, 4, seed=6, exact=True))
    out.append(Case('signed_m5000_k16', _signed, 5000, 16, seed=7))
    for it in (0, 1, 300):
        out.append(Case(f'max_iter{it}_m12000_k32', _lognormal1, 12000, 32, max_iter=it, seed=8))
    out.append(Case('heavy_tail_m30000_k64', _lognormal2, 30000, 64, seed=17))
    for m in (600, 5000):
        for e in (0, 20, 27):
            out.append(Case(f'translation_m{m}_shift2p{e}' if e else f'translation_m{m}_shift0', _dyadic, m, 8, seed=10,
                            shift=float(1 << e) if e else 0.0))
    return out


CASES = _cases()
TRANSLATION = {m: [c for c in CASES if c.name.startswith(f'translation_m{m}_')] for m in (600, 5000)}


@functools.lru_cache(maxsize=None)
def data(case):
    x = case.recipe(np.random.RandomState(case.seed), case.m) + case.shift
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(case):
    """the long-double result of a case, computed once and shared"""
    return quantise(data(case), case.k, case.max_iter)
