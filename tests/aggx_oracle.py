"""
Plain-numpy reference of csrc/grx_aggx.hip (median, wrapping int64 sum / prod, int64 min / max, neighbour counts,
the two conversions) and the case builders of tests/test_gpu_aggx_kernels.py.  tests/test_aggx_oracle_cpu.py pins the
reference to pandas and to tests/fake_kernels.py and checks that every case reaches what it is there for.  Imports
without a GPU; no reference code.

Every expected value here is selected, moved or computed in integer arithmetic, and the even-row median is the one
fp64 operation (a + b) / 2 of two selected values: the GPU tests compare with equality.
"""
import functools
from typing import Callable, NamedTuple

import numpy as np

from tests import util

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1

#: row lengths around every decision of the selection kernels: 0 / 1 / 2 / 3 (empty, odd, even, the first row with
#: two distinct middles), 63 .. 66 around the one-wavefront rank count (d <= 64), 127 .. 129 and 255 .. 257 around
#: two and four trips of the 64-lane loops of the radix branch, 1000 / 1001 an even and an odd long row
DEGREE_CLASSES = (0, 1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 1000, 1001)


# ---- graphs: (row_ptr int64[n + 1], adj_col int32[nnz]) -------------------------------------------------------------

def graph_from_degrees(deg, seed):
    """Directed graph whose row v lists exactly deg[v] distinct neighbours, in random (unsorted) order."""
    deg = np.asarray(deg, dtype=np.int64)
    n = len(deg)
    assert deg.max() <= n
    rng = np.random.default_rng(seed)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=row_ptr[1:])
    adj = np.empty(int(row_ptr[-1]), dtype=np.int32)
    for v in range(n):
        adj[row_ptr[v]:row_ptr[v + 1]] = rng.choice(n, size=int(deg[v]), replace=False)
    return row_ptr, adj


def degree_class_graph(seed=101, fill=1200, trailing_empty=7):
    """40 random-fill rows (so the classes start at an adjacency offset > 0), one row per entry of DEGREE_CLASSES, the
    rest of the random fill (lengths 0 .. 12) and `trailing_empty` rows without neighbours."""
    rng = np.random.default_rng(seed)
    filler = rng.integers(0, 13, size=fill)
    deg = np.concatenate([filler[:40], DEGREE_CLASSES, filler[40:], np.zeros(trailing_empty, dtype=np.int64)])
    return graph_from_degrees(deg, seed + 1)


def star_graph(seed=102, n=70002):
    """Undirected star: node 0 lists the 70 001 others in a random order, each of them lists node 0."""
    rng = np.random.default_rng(seed)
    row_ptr = np.concatenate([[0], np.arange(n - 1, 2 * (n - 1) + 1)]).astype(np.int64)
    adj = np.concatenate([rng.permutation(np.arange(1, n)), np.zeros(n - 1, dtype=np.int64)]).astype(np.int32)
    return row_ptr, adj


def powerlaw_csr(seed=103, n=3000, m=5):
    """util.powerlaw_graph as a symmetric adjacency; a row lists its neighbours in order of appearance."""
    src, dst, _ = util.powerlaw_graph(n, m, seed)
    rows = np.concatenate([src, dst])
    cols = np.concatenate([dst, src])
    order = np.argsort(rows, kind='stable')
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=row_ptr[1:])
    return row_ptr, cols[order].astype(np.int32)


GRAPHS = {'classes': degree_class_graph, 'powerlaw': powerlaw_csr, 'star': star_graph}
#: a row range [rb, re) per graph with rb inside the graph (its adjacency slice starts at row_ptr[rb] > 0); the one
#: of 'classes' cuts through the class rows, the one of 'star' leaves the centre out
ROW_RANGES = {'classes': (44, 60), 'powerlaw': (1000, 2500), 'star': (5, 60000)}


@functools.lru_cache(maxsize=None)
def graph(name):
    row_ptr, adj = GRAPHS[name]()
    row_ptr.setflags(write=False)
    adj.setflags(write=False)
    return row_ptr, adj


def sorted_col(row_ptr, adj):
    """The same rows with ascending neighbours (DeviceCSR.col; the aggregations read agg_col = adj)."""
    rows = np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr))
    return adj[np.lexsort((adj, rows))]


# ---- reference ------------------------------------------------------------------------------------------------------

def _by_degree(row_ptr, adj, row_begin, row_end):
    """(rows, [len(rows), d] neighbour table) for every row length d > 0 in [row_begin, row_end)."""
    deg = np.diff(row_ptr)
    rows = np.arange(row_begin, row_end, dtype=np.int64)
    for d in np.unique(deg[rows]):
        if d == 0:
            continue
        sel = rows[deg[rows] == d]
        idx = row_ptr[sel][:, None] + np.arange(d, dtype=np.int64)[None, :]
        yield sel, adj[idx]


def _range(row_ptr, row_begin, row_end):
    n = len(row_ptr) - 1
    return row_begin, (n if row_end is None else row_end)


def median(row_ptr, adj, X, row_begin=0, row_end=None):
    """[f, n] block: np.median of every row's neighbour values per column of X [n, f]; 0 for rows without
    neighbours and for rows outside [row_begin, row_end)."""
    rb, re = _range(row_ptr, row_begin, row_end)
    out = np.zeros((X.shape[1], len(row_ptr) - 1), dtype=np.float64)
    with np.errstate(invalid='ignore'):                        # (-inf + inf) / 2 of an even row: NaN on both sides
        for sel, nb in _by_degree(row_ptr, adj, rb, re):
            out[:, sel] = np.median(X[nb], axis=1).T           # X[nb]: [rows, d, f]
    return out


def aggregate_i64(row_ptr, adj, X, row_begin=0, row_end=None):
    """{'sum' | 'prod' | 'min' | 'max': int64 [f, n]} over the neighbours' values of X int64 [n, f]: sum and product
    wrap modulo 2^64; rows without neighbours give sum 0, prod 1, min 0, max 0 (rows outside the range: all 0)."""
    assert X.dtype == np.int64
    rb, re = _range(row_ptr, row_begin, row_end)
    f, n = X.shape[1], len(row_ptr) - 1
    outs = {a: np.zeros((f, n), dtype=np.int64) for a in ('sum', 'prod', 'min', 'max')}
    outs['prod'][:, rb:re] = 1
    with np.errstate(over='ignore'):
        for sel, nb in _by_degree(row_ptr, adj, rb, re):
            vals = X[nb]
            outs['sum'][:, sel] = vals.sum(axis=1).T
            outs['prod'][:, sel] = np.multiply.reduce(vals, axis=1).T
            outs['min'][:, sel] = vals.min(axis=1).T
            outs['max'][:, sel] = vals.max(axis=1).T
    return outs


def count(row_ptr, f, row_begin=0, row_end=None, as_i64=False):
    """[f, n] block of neighbour counts (int64 or float64), 0 outside [row_begin, row_end)."""
    rb, re = _range(row_ptr, row_begin, row_end)
    out = np.zeros((f, len(row_ptr) - 1), dtype=np.int64 if as_i64 else np.float64)
    out[:, rb:re] = np.diff(row_ptr)[rb:re]
    return out


def i64_to_f64(x):
    return np.asarray(x, dtype=np.int64).astype(np.float64)


def f64_to_i64(x):
    return np.asarray(x, dtype=np.float64).astype(np.int64)


def even_row_sides(row_ptr, adj, x):
    """(same, next): how many even rows have their upper middle equal to the lower middle's key (at least k + 2 values
    <= the lower middle, k = (d - 1) / 2: the kernel keeps it) and how many need the next larger value."""
    same = nxt = 0
    for sel, nb in _by_degree(row_ptr, adj, 0, len(row_ptr) - 1):
        d = nb.shape[1]
        if d & 1:
            continue
        vals = np.sort(x[nb], axis=1)
        k = (d - 1) // 2
        n_le = (vals <= vals[:, k:k + 1]).sum(axis=1)
        same += int((n_le >= k + 2).sum())
        nxt += int((n_le < k + 2).sum())
    return same, nxt


def exact_row_reductions(row_ptr, adj, x):
    """(sums, products) of every row in exact Python integers (lists of int)."""
    xs = [int(t) for t in x]
    sums, prods = [], []
    for v in range(len(row_ptr) - 1):
        s, p = 0, 1
        for u in adj[row_ptr[v]:row_ptr[v + 1]]:
            s += xs[u]
            p *= xs[u]
        sums.append(s)
        prods.append(p)
    return sums, prods


# ---- value columns for the median -----------------------------------------------------------------------------------

class Column(NamedTuple):
    name: str
    build: Callable                                            # (rng, n) -> values [n]
    sides: str                                                 # which sides of `n_le < k + 2` an even row can take


def _normal(rng, n):
    """Continuous values: every key byte varies, no ties (the upper middle is always the next key)."""
    return rng.standard_normal(n)


def _ties(rng, n):
    """Integers in [-3, 3]: runs of equal keys across the median rank."""
    return rng.integers(-3, 4, size=n).astype(np.float64)


def _low_byte(rng, n):
    """1 + k 2^-52, k < 256: the keys differ in their lowest byte only (the last radix pass decides)."""
    return 1.0 + rng.integers(0, 256, size=n) * 2.0 ** -52


def _middle_byte(rng, n):
    """Bit patterns that differ in byte 3 only (passes 7 .. 4 see one bucket, pass 3 decides, 2 .. 0 one bucket)."""
    bits = np.float64(1.5).view(np.int64) | (rng.integers(0, 256, size=n).astype(np.int64) << 24)
    return bits.view(np.float64)


def _two_valued(rng, n):
    """Two values, exactly half the nodes each: an even row whose neighbours split half and half needs the next key,
    one with more of the lower value keeps it, one with fewer has both middles on the upper value."""
    x = np.where(np.arange(n) % 2 == 0, -2.5, 7.25)
    return x[rng.permutation(n)]


def _around_zero(rng, n):
    """Values straddling zero with both zeros: -0.0 and 0.0 are one value (numpy) but two bit patterns."""
    return rng.choice(np.array([-1.0, -2.0 ** -1074, -0.0, 0.0, 2.0 ** -1074, 1.0]), size=n)


def _magnitudes(rng, n):
    """1e-300 .. 1e300 with both signs: the exponent bytes decide, negative keys are complemented."""
    return rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-300, 300, size=n)


def _constant(rng, n):
    """One value: every histogram has one bucket, n_le = d in every row."""
    return np.full(n, -3.75)


def _with_inf(rng, n):
    """Standard normal with +-inf sprinkled in (a tenth each): the extreme keys, and inf - inf in an even row."""
    x = rng.standard_normal(n)
    u = rng.random(n)
    x[u < 0.1] = -np.inf
    x[u > 0.9] = np.inf
    return x


MEDIAN_COLUMNS = (Column('normal', _normal, 'next'), Column('ties', _ties, 'both'),
                  Column('low_byte', _low_byte, 'both'), Column('middle_byte', _middle_byte, 'both'),
                  Column('two_valued', _two_valued, 'both'), Column('around_zero', _around_zero, 'both'),
                  Column('magnitudes', _magnitudes, 'next'), Column('constant', _constant, 'same'),
                  Column('with_inf', _with_inf, 'both'))
MEDIAN_F = (1, 3, 8, 9, 17)                                    # every pack_rows layout: ldr 2, 4, 8, 16, 32
MEDIAN_SEEDS = {'classes': 7, 'powerlaw': 8, 'star': 9}


@functools.lru_cache(maxsize=None)
def median_values(graph_name):
    """float64 [n, 17]: column j is MEDIAN_COLUMNS[j % 9] (the second round with another seed); the cases with f
    columns use the first f."""
    n = len(graph(graph_name)[0]) - 1
    rng = np.random.default_rng(MEDIAN_SEEDS[graph_name])
    X = np.stack([MEDIAN_COLUMNS[j % len(MEDIAN_COLUMNS)].build(rng, n) for j in range(max(MEDIAN_F))], axis=1)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def median_expected(graph_name):
    return median(*graph(graph_name), median_values(graph_name))


# ---- int64 columns --------------------------------------------------------------------------------------------------

def _small(rng, n):
    """Small values of both signs: nothing wraps in a short row."""
    return rng.integers(-9, 10, size=n, dtype=np.int64)


def _full_range(rng, n):
    """Random over the whole int64 range: sums and products wrap, min / max need the signed order."""
    return rng.integers(I64_MIN, I64_MAX, size=n, dtype=np.int64, endpoint=True)


def _near_2_62(rng, n):
    """+-2^62 plus a small offset: already a two-term sum of equal signs leaves [-2^63, 2^63)."""
    return rng.choice(np.array([-1, 1], dtype=np.int64), size=n) * (2 ** 62) + rng.integers(0, 1000, size=n, dtype=np.int64)


def _special(rng, n):
    """-1 (a NaN bit pattern), 0, 1 (a subnormal) and the two ends of the range."""
    return rng.choice(np.array([-1, 0, 1, I64_MIN, I64_MAX], dtype=np.int64), size=n)


def _odd(rng, n):
    """Odd multipliers: the product wraps but, being odd, never collapses to 0."""
    return rng.integers(-2 ** 40, 2 ** 40, size=n, dtype=np.int64) | 1


def _pow2(rng, n):
    """+-2^e, e in 0 .. 40: the product of a row whose exponents reach 64 is exactly 0."""
    return rng.choice(np.array([-1, 1], dtype=np.int64), size=n) << rng.integers(0, 41, size=n, dtype=np.int64)


I64_COLUMNS = (('small', _small), ('full_range', _full_range), ('near_2_62', _near_2_62), ('special', _special),
               ('odd', _odd), ('pow2', _pow2))
I64_F = (1, 4, 5, 8, 20)
I64_SEEDS = {'classes': 17, 'powerlaw': 18, 'star': 19}
I64_SUM_WRAP_COLUMN, I64_PROD_WRAP_COLUMN, I64_PROD_ZERO_COLUMN = 2, 4, 5


@functools.lru_cache(maxsize=None)
def i64_values(graph_name):
    """int64 [n, 20]: column j is I64_COLUMNS[j % 6]; the cases with f columns use the first f."""
    n = len(graph(graph_name)[0]) - 1
    rng = np.random.default_rng(I64_SEEDS[graph_name])
    X = np.stack([I64_COLUMNS[j % len(I64_COLUMNS)][1](rng, n) for j in range(max(I64_F))], axis=1)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def i64_expected(graph_name):
    return aggregate_i64(*graph(graph_name), i64_values(graph_name))


# ---- conversions and the column movers ------------------------------------------------------------------------------

LENGTHS = (1, 255, 256, 257, 1000003)                          # one lane, around one workgroup, a grid-stride trip

#: the largest double below 2^63: float(2^63 - 1) rounds to 2^63, which no int64 holds (a C cast of it is undefined
#: and numpy's astype warns), so the f64 -> i64 direction takes this neighbour instead
BELOW_2_63 = 2 ** 63 - 1024


def convert_i64_input(n, seed=31):
    """int64 [n]: 0, +-1, 2^53 +- 1 (the first integers fp64 rounds), 2^63 - 1, -2^63, then full-range random."""
    head = np.array([0, 1, -1, 2 ** 53 - 1, 2 ** 53 + 1, -2 ** 53 - 1, 2 ** 53 + 3, I64_MAX, I64_MIN, I64_MAX - 1],
                    dtype=np.int64)
    rng = np.random.default_rng(seed)
    rest = rng.integers(I64_MIN, I64_MAX, size=max(n - len(head), 0), dtype=np.int64)
    return np.concatenate([head, rest])[:max(n, len(head))][-n:]   # n = 1: the last of the list


def convert_f64_input(n, seed=32):
    """float64 [n] of exact integers inside the int64 range: the fp64 images of the list above, then random."""
    head = np.array([0.0, 1.0, -1.0, float(2 ** 53 - 1), float(2 ** 53), float(2 ** 53 + 2), -float(2 ** 53 + 2),
                     float(BELOW_2_63), float(I64_MIN), -0.0])
    rng = np.random.default_rng(seed)
    rest = rng.integers(-2 ** 62, 2 ** 62, size=max(n - len(head), 0), dtype=np.int64).astype(np.float64)
    return np.concatenate([head, rest])[:max(n, len(head))][-n:]


SNAN_BITS = 0x7FF0000000000001                                 # a signalling NaN when read as fp64
QNAN_PAYLOAD_BITS = 0x7FF8000000C0FFEE                         # a quiet NaN with a payload


def bit_pattern_columns(F, m, seed):
    """int64 [F, m] of bit patterns that arithmetic on fp64 would corrupt: small integers (subnormals), -1 and NaNs
    with payloads (x + 0.0 quiets a signalling NaN), -0.0, full-range random bits."""
    rng = np.random.default_rng(seed)
    pool = np.array([0, 1, 2, 3, 255, 4095, -1, -2, SNAN_BITS, SNAN_BITS + 5, QNAN_PAYLOAD_BITS, SNAN_BITS - 2 ** 63,
                     I64_MIN, I64_MAX], dtype=np.int64)
    out = rng.integers(I64_MIN, I64_MAX, size=(F, m), dtype=np.int64)
    pick = rng.random((F, m)) < 0.75
    out[pick] = rng.choice(pool, size=int(pick.sum()))
    return out
