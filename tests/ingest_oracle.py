"""
Plain-numpy reference of csrc/grx_ingest.hip (grx_ingest, grx_orient_count / grx_orient_fill) and the case list of
tests/test_gpu_ingest_kernels.py.  tests/test_ingest_oracle_cpu.py pins the reference to a list-of-lists construction
and to graphrole_amd/graph/csr.py (CSRGraph + InternalGraph) and checks that every case reaches what it is there for.
Imports without a GPU; no reference code; calls neither InternalGraph nor DeviceCSR.oriented().

The reference is written from the definitions in the header comment of grx_ingest.hip and in include/grx.h:
  perm      node labels by (degree descending, label ascending); degree = out-degree of a directed graph, an
            undirected self-loop counts once; inv = its inverse
  row_ptr   exclusive scan of the degrees in that order
  col       every row's neighbours (internal ids) ascending, w aligned with it
  agg_col   the same rows with the neighbours in order of appearance of the incident edge (the loop arc once)
  t_*       directed graphs: the same for the in-adjacency (rows = targets, columns = sources, ascending)
  oriented  d'(v) = degree without the loop; arc u -> v kept iff (d'(u), u) < (d'(v), v), in ascending order of the
            row; per kept arc k = u -> v the word
            begin of N+(v) | min(|N+(v)|, 1023) << 32 | min(|N+(u)|, 1023) << 42 | min(k - begin of N+(u), 1023) << 52
Everything is an integer or a copied weight: the tests compare with equality (weights as int64 bit patterns).
"""
import functools
from typing import Callable, FrozenSet, NamedTuple, Optional

import numpy as np

SCAN_TILE = 2048                   # ING_SCAN_TILE; ing_scan_top_kernel takes more than one tile per thread above
SCAN_TOP_THREADS = 1024            # 1024 tiles (n > 2 097 152)
SORT_TILE = 4096                   # keys per tile of grx_internal_sort_u64
EDGE_GRID_SPAN = 4096 * 256        # the edge kernels stride above this many edges
ORIENT_WAVE_ROWS = 32768           # orient_count / orient_fill stride over rows above this (256 CUs * 32 * 4 waves)
ARC_GRID_SPAN = 256 * 32 * 256     # orient_arc_kernel strides over rows above this
SATURATION = 1023                  # the 10-bit fields of the per-arc word
SMALL_EDGES = 10000                # cases up to this many edges are also built by list_of_lists()


class Reference(NamedTuple):
    n: int
    m: int
    directed: bool
    nnz: int
    perm: np.ndarray               # int64 [n]
    inv: np.ndarray                # int64 [n]
    row_ptr: np.ndarray            # int64 [n + 1]
    col: np.ndarray                # int32 [nnz]
    agg_col: np.ndarray            # int32 [nnz]
    w: Optional[np.ndarray]        # float64 [nnz]
    t_row_ptr: Optional[np.ndarray]
    t_col: Optional[np.ndarray]
    t_w: Optional[np.ndarray]


class Oriented(NamedTuple):
    row_ptr: np.ndarray            # int64 [n + 1]
    col: np.ndarray                # int32 [o_nnz]
    arc: np.ndarray                # int64 [o_nnz]


def bits(x):
    """float64 array -> its int64 bit patterns (what the weight comparisons are made on)."""
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


# ---- reference ------------------------------------------------------------------------------------------------------

def _arcs(src, dst, directed):
    """(rows, cols, edge index) of every arc in slot order: slot 2e = src -> dst, slot 2e + 1 = dst -> src (absent
    for a loop); directed graphs have the one arc per edge."""
    m = len(src)
    if directed:
        return src, dst, np.arange(m, dtype=np.int64)
    rows = np.stack([src, dst], axis=1).reshape(-1)
    cols = np.stack([dst, src], axis=1).reshape(-1)
    present = np.stack([np.ones(m, dtype=bool), src != dst], axis=1).reshape(-1)
    edge = np.repeat(np.arange(m, dtype=np.int64), 2)
    return rows[present], cols[present], edge[present]


def _sorted_rows(n, r, c, w_arc):
    """CSR with ascending columns of the arcs (r, c)."""
    order = np.lexsort((c, r))
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=row_ptr[1:])
    return row_ptr, c[order].astype(np.int32), (None if w_arc is None else w_arc[order])


def reference(n, src, dst, w, directed) -> Reference:
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    rows, cols, edge = _arcs(src, dst, directed)
    deg = np.bincount(rows, minlength=n)
    perm = np.lexsort((np.arange(n), -deg)).astype(np.int64)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n, dtype=np.int64)
    r, c = inv[rows], inv[cols]
    w_arc = None if w is None else np.asarray(w, dtype=np.float64)[edge]
    row_ptr, col, w_col = _sorted_rows(n, r, c, w_arc)
    agg_col = c[np.argsort(r, kind='stable')].astype(np.int32)       # the arcs are in slot order already
    t_row_ptr = t_col = t_w = None
    if directed:
        t_row_ptr, t_col, t_w = _sorted_rows(n, c, r, w_arc)
    return Reference(int(n), int(len(src)), bool(directed), int(len(rows)), perm, inv, row_ptr, col, agg_col, w_col,
                     t_row_ptr, t_col, t_w)


def oriented(row_ptr, col) -> Oriented:
    """The degree-oriented copy of any symmetric CSR with ascending columns (the rows need not be degree-sorted)."""
    n = len(row_ptr) - 1
    deg = np.diff(row_ptr)
    rows = np.repeat(np.arange(n, dtype=np.int64), deg)
    colv = col.astype(np.int64)
    dprime = deg - np.bincount(rows[rows == colv], minlength=n)
    rank = dprime * np.int64(n) + np.arange(n, dtype=np.int64)       # (d', label) as one number
    keep = rank[rows] < rank[colv]
    u, v = rows[keep], colv[keep]
    o_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(u, minlength=n), out=o_ptr[1:])
    olen = np.minimum(np.diff(o_ptr), SATURATION)
    pos = np.minimum(np.arange(len(u), dtype=np.int64) - o_ptr[u], SATURATION)
    arc = o_ptr[v] | (olen[v] << 32) | (olen[u] << 42) | (pos << 52)
    return Oriented(o_ptr, v.astype(np.int32), arc)


def label_csr(n, src, dst):
    """The symmetric CSR of an undirected edge list in LABEL order (ascending columns, a loop once)."""
    rows, cols, _ = _arcs(np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64), False)
    row_ptr, col, _ = _sorted_rows(n, rows, cols, None)
    return row_ptr, col


# ---- second construction: lists of lists, plain Python --------------------------------------------------------------

def list_of_lists(n, src, dst, w, directed):
    """The same structures with Python lists and integers only: add_edge(u, v) appends v to adj[u] and u to adj[v]
    (once for a loop), rows sorted by (-len, label), ids relabelled.  Returns a dict of lists (None where absent);
    'o_row_ptr' / 'o_col' / 'o_arc' for undirected graphs."""
    adj = [[] for _ in range(n)]
    tadj = [[] for _ in range(n)]
    wt = {}
    for e in range(len(src)):
        u, v = int(src[e]), int(dst[e])
        adj[u].append(v)
        if directed:
            tadj[v].append(u)
        elif u != v:
            adj[v].append(u)
        if w is not None:
            wt[(u, v)] = w[e]
            if not directed:
                wt[(v, u)] = w[e]
    perm = sorted(range(n), key=lambda i: (-len(adj[i]), i))
    inv = [0] * n
    for i, lab in enumerate(perm):
        inv[lab] = i

    def rows_of(lists, weight_key):
        ptr, cols, ws = [0], [], []
        for lab in perm:
            nb = sorted(lists[lab], key=lambda x: inv[x])
            cols += [inv[x] for x in nb]
            if w is not None:
                ws += [wt[weight_key(lab, x)] for x in nb]
            ptr.append(len(cols))
        return ptr, cols, (ws if w is not None else None)

    out = {'perm': perm, 'inv': inv}
    out['row_ptr'], out['col'], out['w'] = rows_of(adj, lambda r, c: (r, c))
    out['agg_col'] = [inv[x] for lab in perm for x in adj[lab]]
    out['t_row_ptr'] = out['t_col'] = out['t_w'] = None
    if directed:
        out['t_row_ptr'], out['t_col'], out['t_w'] = rows_of(tadj, lambda r, c: (c, r))
        return out
    # orientation of the relabelled graph
    ptr, col = out['row_ptr'], out['col']
    nbrs = [col[ptr[i]:ptr[i + 1]] for i in range(n)]
    dp = [len(nbrs[i]) - (1 if i in nbrs[i] else 0) for i in range(n)]
    kept = [[v for v in nbrs[u] if (dp[u], u) < (dp[v], v)] for u in range(n)]
    o_ptr = [0]
    for u in range(n):
        o_ptr.append(o_ptr[-1] + len(kept[u]))
    o_arc = []
    for u in range(n):
        for p, v in enumerate(kept[u]):
            o_arc.append(o_ptr[v] | (min(len(kept[v]), 1023) << 32) | (min(len(kept[u]), 1023) << 42) | (min(p, 1023) << 52))
    out['o_row_ptr'], out['o_col'], out['o_arc'] = o_ptr, [v for k in kept for v in k], o_arc
    return out


# ---- weights --------------------------------------------------------------------------------------------------------

#: bit patterns that arithmetic on the value would change or merge: both zeros, the smallest subnormal, the
#: infinities, the largest finite value, quiet and signalling NaNs of both signs with distinct payloads
SPECIAL_WEIGHT_BITS = np.array([
    0x8000000000000000, 0x0000000000000000, 0x0000000000000001, 0x7FF0000000000000, 0xFFF0000000000000,
    0x7FEFFFFFFFFFFFFF, 0x7FF8000000000000, 0x7FF8000000C0FFEE, 0xFFF8000000000001, 0x7FF0000000000001,
    0xFFF0000000000BAD, 0x7FF4000000000000], dtype=np.uint64).view(np.int64)


def special_weights(m, seed):
    """float64 [m]: uniform(0.1, 5) with about a third of the entries replaced by SPECIAL_WEIGHT_BITS; every special
    pattern occurs once m >= 12 (the first entries are the list itself)."""
    rng = np.random.default_rng(seed)
    out = rng.uniform(0.1, 5.0, size=m).view(np.int64)
    pick = rng.random(m) < 1 / 3
    out[pick] = rng.choice(SPECIAL_WEIGHT_BITS, size=int(pick.sum()))
    k = min(m, len(SPECIAL_WEIGHT_BITS))
    out[:k] = SPECIAL_WEIGHT_BITS[:k]
    return out.view(np.float64)


def finite_weights(m, seed):
    """float64 [m]: k / 8 with k in 1 .. 8000.  Any sum of fewer than 2^40 of them is exact in fp64, so a row sum is
    the same number in every order of the additions."""
    return np.random.default_rng(seed).integers(1, 8001, size=m).astype(np.float64) / 8.0


# ---- case builders: (n, src, dst, w, directed), unique edges --------------------------------------------------------

def _shuffled(rng, src, dst, flip=True):
    """Random edge order; with `flip` every edge is given as (high, low) or (low, high) at random."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    order = rng.permutation(len(src))
    src, dst = src[order], dst[order]
    if flip:
        swap = rng.random(len(src)) < 0.5
        src, dst = np.where(swap, dst, src), np.where(swap, src, dst)
    return src, dst


def _n1_loop(weighted=False):
    w = np.array([-0.0]) if weighted else None
    return 1, np.array([0]), np.array([0]), w, False


def _n2_reversed():
    return 2, np.array([1]), np.array([0]), None, False


def _path3():
    return 3, np.array([2, 1]), np.array([1, 0]), np.array([5e-324, np.inf]), False


def _all_loops(n=300):
    nodes = np.random.default_rng(11).permutation(n)
    return n, nodes, nodes.copy(), special_weights(n, 12), False


def _loops_and_edges(n=5000, k=100):
    """k edges and k loops in a sparse graph; the loops sit at even and at odd edge indices."""
    rng = np.random.default_rng(13)
    nodes = rng.choice(n, size=3 * k, replace=False)
    src = np.empty(2 * k, dtype=np.int64)
    dst = np.empty(2 * k, dtype=np.int64)
    is_loop = np.zeros(2 * k, dtype=bool)
    is_loop[0:k:2] = True                                       # even indices in the first half ...
    is_loop[k + 1::2] = True                                    # ... odd ones in the second
    loops, ends = nodes[:k], nodes[k:].reshape(k, 2)
    src[is_loop], dst[is_loop] = loops, loops
    src[~is_loop], dst[~is_loop] = ends[:, 0], ends[:, 1]
    return n, src, dst, None, False


def _ring_edges(k):
    """Ring over nodes 0 .. k - 1 plus the chords i -- i + k // 2 of every second i < k // 2: degrees 2 and 3.  Odd
    ring edges are given as (high, low)."""
    i = np.arange(k, dtype=np.int64)
    a, b = i, (i + 1) % k
    odd = i % 2 == 1
    src, dst = np.where(odd, b, a), np.where(odd, a, b)
    h = k // 2
    c = np.arange(0, h, 2, dtype=np.int64)
    return np.concatenate([src, c + h]), np.concatenate([dst, c])


def _ring(n, isolate_last=False):
    src, dst = _ring_edges(n - 1 if isolate_last else n)
    return n, src, dst, None, False


def _stride_edges(n, m):
    """The first m of the edges i -- (i + k) mod n, k = 1, 2, 3, ... (k < n / 2: no edge twice, none reversed)."""
    src, dst, k = [], [], 1
    while sum(len(s) for s in src) < m:
        assert 2 * k < n
        i = np.arange(n, dtype=np.int64)
        a, b = i, (i + k) % n
        odd = (i + k) % 2 == 1
        src.append(np.where(odd, b, a))
        dst.append(np.where(odd, a, b))
        k += 1
    return np.concatenate(src)[:m], np.concatenate(dst)[:m]


def _slots(n, m, directed):
    src, dst = _stride_edges(n, m)
    return n, src, dst, (special_weights(m, n + m) if directed else None), directed


def _circulant(n=10000, half=4):
    i = np.arange(n, dtype=np.int64)
    src = np.concatenate([i] * half)
    dst = np.concatenate([(i + k) % n for k in range(1, half + 1)])
    return n, src, dst, None, False


def _mass_isolated(n=300000, k=5000, m=20000, loops=40):
    rng = np.random.default_rng(17)
    nodes = np.arange(k, dtype=np.int64) * (n // k) + rng.integers(0, n // k, size=k)
    a, b = rng.integers(0, k, size=2 * m), rng.integers(0, k, size=2 * m)
    key = np.unique(np.minimum(a, b)[a != b] * k + np.maximum(a, b)[a != b])
    key = key[rng.permutation(len(key))[:m]]
    lp = rng.choice(k, size=loops, replace=False)
    src, dst = _shuffled(rng, np.concatenate([key // k, lp]), np.concatenate([key % k, lp]))
    return n, nodes[src], nodes[dst], None, False


HUB_STARS = (63, 64, 65, 127, 128, 129, 1000, 1001)            # neighbour counts of the small star centres
HUB_CLIQUES = (64, 65, 66, 128, 129, 130)                      # K_k: rows of k - 1 arcs with equal d' (kept by label)
HUB_BIG = 70001
HUB_BIG_LABEL = 35000


def _hubs(weighted=False, hub_loop=False, seed=19):
    """One centre with 70 001 neighbours (every other node of the star part), eight smaller centres among its leaves
    with HUB_STARS neighbours in all, and the cliques of HUB_CLIQUES on labels of their own behind the star part
    (not joined to the big centre).  Edges in both orientations, shuffled."""
    rng = np.random.default_rng(seed)
    n_star = HUB_BIG + 1
    big = HUB_BIG_LABEL
    others = np.delete(np.arange(n_star, dtype=np.int64), big)
    src, dst = [np.full(HUB_BIG, big, dtype=np.int64)], [others]
    pool = 40000                                               # leaves above the big centre: one disjoint run per star
    for j, cnt in enumerate(HUB_STARS):
        centre = 10 * (j + 1)
        src.append(np.full(cnt - 1, centre, dtype=np.int64))   # the centre's link to the big one is its cnt-th
        dst.append(np.arange(pool, pool + cnt - 1, dtype=np.int64))
        pool += cnt + 50
    assert pool < n_star
    base = n_star
    for k in HUB_CLIQUES:
        iu = np.triu_indices(k, 1)
        src.append(base + iu[0])
        dst.append(base + iu[1])
        base += k
    n = base
    src, dst = np.concatenate(src), np.concatenate(dst)
    if hub_loop:
        src, dst = np.append(src, big), np.append(dst, big)
    src, dst = _shuffled(rng, src, dst)
    return n, src, dst, (special_weights(len(src), seed + 1) if weighted else None), False


DHUB_ORDINARY = 70001


def _directed_hubs(finite=False, seed=23):
    """Ordinary nodes 0 .. 70 000, a source (label 70 001: an arc to every ordinary node, in-degree 0) and a sink
    (label 70 002, the last: an arc from every ordinary node, out-degree 0).  The ordinary nodes form the ring
    i -> i + 1, every second arc of it with its reciprocal, every 97th node with a loop."""
    rng = np.random.default_rng(seed)
    k = DHUB_ORDINARY
    i = np.arange(k, dtype=np.int64)
    source, sink = k, k + 1
    back = i[::2]
    loops = i[::97]
    src = np.concatenate([np.full(k, source), i, i, (back + 1) % k, loops])
    dst = np.concatenate([i, np.full(k, sink), (i + 1) % k, back, loops])
    src, dst = _shuffled(rng, src, dst, flip=False)
    m = len(src)
    return k + 2, src, dst, (finite_weights(m, seed + 1) if finite else special_weights(m, seed + 1)), True


CLIQUE = 1026
CLIQUE_N = 5000


def clique_labels():
    return 3 * np.arange(CLIQUE, dtype=np.int64) + 1


def _clique(seed=29):
    """K_1026 on the labels 3 j + 1 next to a sparse random part on the other labels; every seventh clique node has
    one pendant neighbour of its own (d' + 1, no triangle).  Every clique node is in C(1025, 2) triangles."""
    rng = np.random.default_rng(seed)
    lab = clique_labels()
    iu = np.triu_indices(CLIQUE, 1)
    rest = np.setdiff1d(np.arange(CLIQUE_N, dtype=np.int64), lab)
    pend_of = lab[::7]
    pendants, sparse = rest[:len(pend_of)], rest[len(pend_of):]
    a, b = rng.integers(0, len(sparse), size=8000), rng.integers(0, len(sparse), size=8000)
    key = np.unique(np.minimum(a, b)[a != b] * len(sparse) + np.maximum(a, b)[a != b])
    src = np.concatenate([lab[iu[0]], pend_of, sparse[key // len(sparse)]])
    dst = np.concatenate([lab[iu[1]], pendants, sparse[key % len(sparse)]])
    src, dst = _shuffled(rng, src, dst)
    return CLIQUE_N, src, dst, None, False


LARGE_N = SCAN_TILE * SCAN_TOP_THREADS + 1                     # 2 097 153: 1025 scan tiles, the last with one element
LARGE_M = 1_200_000


def _large(directed, seed):
    rng = np.random.default_rng(seed)
    n = LARGE_N
    a, b = rng.integers(0, n, size=LARGE_M + 2000), rng.integers(0, n, size=LARGE_M + 2000)
    off = a != b
    a, b = a[off], b[off]
    key = a * n + b if directed else np.minimum(a, b) * n + np.maximum(a, b)
    first = np.sort(np.unique(key, return_index=True)[1])[:LARGE_M]   # unique, in order of appearance
    a, b = a[first], b[first]
    loops = rng.choice(n, size=9, replace=False)
    at = rng.integers(0, len(a), size=9)
    src, dst = np.insert(a, at, loops), np.insert(b, at, loops)
    return n, src, dst, (special_weights(len(src), seed + 1) if directed else None), directed


class Case(NamedTuple):
    name: str
    build: Callable
    props: FrozenSet[str]          # what the case exists for; tests/test_ingest_oracle_cpu.py asserts each of them
    directed: bool
    small: bool                    # at most SMALL_EDGES edges: also built by list_of_lists()


def _case(name, build, *props, directed=False, small=False):
    return Case(name, build, frozenset(props), directed, small)


# Properties (each has a check in test_ingest_oracle_cpu.py::PROPERTY_CHECKS):
#   single_node, reversed_edge, all_loops (half of the slots are sentinels), loops_even_odd
#   block_edge (n within one of a multiple of 256), scan_tile_edge (... of 2048), sort_tile_edge (... of 4096),
#   last_tile_single (the last scan tile holds one element), last_isolated (that element is 0), mass_ties
#   slots_4095 / slots_4096 / slots_4097 (the key count of the arc sorts)
#   identity_perm, mass_isolated, rows_stride (n > 32 768: orient_count / orient_fill stride over rows)
#   ballot_rows (rows of 63, 64, 65, 127, 128, 129, 1000 and 1001 arcs), ballot_kept (oriented lists of 63 .. 65 and
#   127 .. 129 arcs: kept arcs in lane 0 and lane 63 of a full wavefront), hub_row (a row of >= 70 001 arcs),
#   hub_loop, shuffled (0.3 .. 0.7 of the edges given as (high, low)), special_weights, finite_weights
#   in_hub_last (in-degree 70 001, out-degree 0, last internal row), out_hub_first, reciprocal, directed_loops
#   saturation (oriented lengths 1022 .. 1025), scan_top_chunk (> 1024 tiles), edge_stride (m > 1 048 576),
#   arc_stride (n > 2 097 152)
def _make_cases():
    cases = [
        _case('n1_loop', _n1_loop, 'single_node', 'all_loops', small=True),
        _case('n1_loop_w', functools.partial(_n1_loop, True), 'single_node', 'all_loops', small=True),
        _case('n2_reversed', _n2_reversed, 'reversed_edge', small=True),
        _case('path3_w', _path3, 'reversed_edge', small=True),
        _case('all_loops300_w', _all_loops, 'all_loops', 'special_weights', small=True),
        _case('loops100_edges100', _loops_and_edges, 'loops_even_odd', small=True),
    ]
    for n in (255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097):
        edge = ['block_edge'] + (['scan_tile_edge'] if n > 2000 else []) + (['sort_tile_edge'] if n > 4000 else [])
        single = ['last_tile_single'] if n % SCAN_TILE == 1 else []
        cases.append(_case(f'ring{n}', functools.partial(_ring, n), 'mass_ties', *edge, *single, small=True))
        cases.append(_case(f'ring{n}_iso', functools.partial(_ring, n, True), 'mass_ties', 'last_isolated', *edge, *single,
                           small=True))
        cases.append(_case(f'slots4096_n{n}', functools.partial(_slots, n, 2048, False), 'slots_4096', *edge, small=True))
        for m in (4095, 4096, 4097):
            cases.append(_case(f'dslots{m}_n{n}', functools.partial(_slots, n, m, True), f'slots_{m}', 'special_weights',
                               *edge, directed=True, small=True))
    cases += [
        _case('circulant10000', _circulant, 'identity_perm', 'mass_ties'),
        _case('isolated300k', _mass_isolated, 'mass_isolated', 'rows_stride', 'shuffled'),
        _case('hubs', _hubs, 'ballot_rows', 'ballot_kept', 'hub_row', 'shuffled', 'rows_stride'),
        _case('hubs_loop', functools.partial(_hubs, False, True), 'ballot_rows', 'ballot_kept', 'hub_row', 'hub_loop',
              'shuffled'),
        _case('hubs_loop_w', functools.partial(_hubs, True, True), 'ballot_rows', 'hub_row', 'hub_loop', 'shuffled',
              'special_weights'),
        _case('dhubs_w', _directed_hubs, 'in_hub_last', 'out_hub_first', 'reciprocal', 'directed_loops', 'hub_row',
              'special_weights', directed=True),
        _case('dhubs_finite', functools.partial(_directed_hubs, True), 'in_hub_last', 'out_hub_first', 'finite_weights',
              directed=True),
        _case('clique1026', _clique, 'saturation', 'shuffled', 'ballot_kept'),
        _case('large_u', functools.partial(_large, False, 31), 'scan_top_chunk', 'last_tile_single', 'edge_stride',
              'arc_stride', 'rows_stride', 'mass_isolated'),
        _case('large_dw', functools.partial(_large, True, 37), 'scan_top_chunk', 'last_tile_single', 'edge_stride',
              'mass_isolated', 'special_weights', directed=True),
    ]
    return tuple(cases)


CASES = _make_cases()
CASE_NAMES = tuple(c.name for c in CASES)
_BY_NAME = {c.name: c for c in CASES}
assert len(_BY_NAME) == len(CASES)
#: the three cases whose LABEL-order CSR is oriented on its own (the kernel apart from the ingest it normally follows)
LABEL_ORDER_CASES = ('hubs_loop', 'clique1026', 'isolated300k')


def case(name) -> Case:
    return _BY_NAME[name]


@functools.lru_cache(maxsize=None)
def graph(name):
    """(n, src int64, dst int64, w float64 or None, directed) of a case, built once and read-only."""
    n, src, dst, w, directed = _BY_NAME[name].build()
    src = np.ascontiguousarray(src, dtype=np.int64)
    dst = np.ascontiguousarray(dst, dtype=np.int64)
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    for a in (src, dst, w):
        if a is not None:
            a.setflags(write=False)
    return int(n), src, dst, w, bool(directed)


def _freeze(t):
    for a in t:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def expected(name) -> Reference:
    return _freeze(reference(*graph(name)))


@functools.lru_cache(maxsize=None)
def expected_oriented(name) -> Oriented:
    ref = expected(name)
    assert not ref.directed
    return _freeze(oriented(ref.row_ptr, ref.col))


@functools.lru_cache(maxsize=None)
def label_order(name):
    """(row_ptr, col, Oriented) of the label-order CSR of an undirected case."""
    n, src, dst, _, directed = graph(name)
    assert not directed
    row_ptr, col = label_csr(n, src, dst)
    return _freeze((row_ptr, col, _freeze(oriented(row_ptr, col))))
