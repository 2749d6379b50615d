"""
Oracles of the neighbour-role pass of NeighborSense (grx_neighbor_roles, csrc/grx_neighbor_sense.hip).

``neighbor_roles``: a numpy restatement of the kernel's summation order as include/grx.h states it -- every product
w_p * P[col_p, k] rounded on its own, the arcs of a row dealt to S = 8 slots (128 for a row with more than 1024 arcs) by
their position modulo S, every slot summed in ascending order from +0.0, the slots combined by the tree h = S/2, ..., 1:
slot t += slot t + h.  The device result equals it bit for bit.

``dense``: the independent authority, A @ P with A built by networkx; ``bound`` the derived error bound per entry: a
sum of d terms in ANY order errs by at most (d - 1) 2^-53 times the sum of the magnitudes (to first order), 4.4e-13 of
it at d = 4000 -- every test degree stays below that --, and the mean adds the same for its denominator and one rounding
of the quotient, so 1e-12 of the magnitudes (over the denominator) covers both modes.
"""
import networkx as nx
import numpy as np

SLOTS = 8
LONG_SLOTS = 128
LONG_ROW = 1024
MAX_TEST_DEGREE = 4000
REL_BOUND = 1e-12


def _slot_sum(terms: np.ndarray, slots: int) -> np.ndarray:
    """terms [d, ...] -> their sum in the kernel's order (zero padding at the end of a slot adds +0.0: no change)."""
    d = terms.shape[0]
    steps = -(-d // slots)
    padded = np.zeros((steps * slots,) + terms.shape[1:])
    padded[:d] = terms
    padded = padded.reshape((steps, slots) + terms.shape[1:])
    acc = np.zeros((slots,) + terms.shape[1:])
    for i in range(steps):
        acc = acc + padded[i]
    h = slots // 2
    while h:
        acc = acc[:h] + acc[h:2 * h]
        h //= 2
    return acc[0]


def neighbor_roles(row_ptr, col, w, P, mode='mean') -> np.ndarray:
    """The [r, n] feature-major table of grx_neighbor_roles over the CSR (row_ptr, col, w or None) and the n x r
    memberships P, bit for bit."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    P = np.asarray(P, dtype=np.float64)
    n, r = len(row_ptr) - 1, P.shape[1]
    out = np.zeros((r, n))
    for i in range(n):
        b, e = row_ptr[i], row_ptr[i + 1]
        d = e - b
        if d == 0:
            continue
        slots = SLOTS if d <= LONG_ROW else LONG_SLOTS
        rows = P[col[b:e]]
        if w is None:
            total, den = _slot_sum(rows, slots), float(d)
        else:
            wi = np.asarray(w[b:e], dtype=np.float64)
            total, den = _slot_sum(wi[:, None] * rows, slots), _slot_sum(wi, slots)
        if mode == 'mean':
            total = total / den if den != 0.0 else np.zeros(r)
        out[:, i] = total
    return out


def adjacency(G, weighted: bool, direction: str = 'out') -> np.ndarray:
    """op(A) over the sorted labels from networkx: A[u, v] = the weight of u -> v (1 without `weighted`; an undirected
    edge from both ends, a self-loop once); 'in' = A^T and 'all' = A + A^T on a directed graph."""
    nodes = sorted(G)
    A = nx.to_numpy_array(G, nodelist=nodes, weight='weight' if weighted else None, dtype=np.float64)
    if G.is_directed() and direction == 'in':
        A = A.T
    elif G.is_directed() and direction == 'all':
        A = A + A.T
    return np.ascontiguousarray(A)


def csr_of(A: np.ndarray, weighted: bool):
    """(row_ptr int64, col int32 ascending inside a row, w or None) of the non-zeros of a dense matrix; without
    `weighted` the weights are left out when every entry is 1 (A + A^T holds a 2 at a reciprocal pair)."""
    rows, cols = np.nonzero(A)
    row_ptr = np.zeros(A.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=A.shape[0]), out=row_ptr[1:])
    w = np.ascontiguousarray(A[rows, cols])
    return row_ptr, cols.astype(np.int32), (w if weighted or np.any(w != 1.0) else None)


def dense(A: np.ndarray, P: np.ndarray, mode: str = 'mean'):
    """(N [n, r], bound [n, r]) of the dense authority: A @ P, over the row sums of A for the mean (0 where they are 0),
    and REL_BOUND times sum_p |w_p P[col_p, k]| (over the denominator for the mean)."""
    assert np.count_nonzero(A, axis=1).max(initial=0) < MAX_TEST_DEGREE and (A >= 0).all()
    N, mag = A @ P, A @ np.abs(P)
    if mode == 'mean':
        den = A.sum(axis=1)
        safe = np.where(den != 0, den, 1.0)[:, None]
        N, mag = np.where(den[:, None] != 0, N / safe, 0.0), np.where(den[:, None] != 0, mag / safe, 0.0)
    return N, REL_BOUND * mag


def arc_counts(G, role_of: dict, roles: list, direction: str = 'out', weighted: bool = False) -> np.ndarray:
    """The role x role arc mass by a Python loop over the edges: an undirected edge from both ends (a self-loop once),
    a directed arc once ('in': reversed, 'all': both ways)."""
    at = {role: k for k, role in enumerate(roles)}
    C = np.zeros((len(roles), len(roles)))
    for u, v, data in G.edges(data=True):
        w = float(data.get('weight', 1.0)) if weighted else 1.0
        a, b = at[role_of[u]], at[role_of[v]]
        if not G.is_directed():
            C[a, b] += w
            if u != v:
                C[b, a] += w
        else:
            if direction in ('out', 'all'):
                C[a, b] += w
            if direction in ('in', 'all'):
                C[b, a] += w
    return C


#: membership widths of the tests: odd widths (the last lane of a membership row then holds one column instead of two)
#: and both sides of every boundary of the kernel's lane split -- the lanes that share a membership row double at
#: r = 2 | 3, 4 | 5, 8 | 9 and 16 | 17 -- up to GRX_MAX_ROLES
WIDTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 31, 32)


def graph_cases() -> dict:
    """name -> graph: the parity cases.  'star' has one leaf more than the long-row threshold, so its centre takes the
    workgroup path, and isolated nodes appended, so the empty row runs beside it."""
    from tests import graphs
    star = nx.star_graph(LONG_ROW + 1)
    star.add_nodes_from(range(LONG_ROW + 2, LONG_ROW + 7))
    rng = np.random.default_rng(11)
    for u, v in star.edges:
        star[u][v]['weight'] = float(rng.uniform(0.25, 4.0))
    return {'karate': nx.karate_club_graph(), 'ba': graphs.ba(300, 3, 1)[0], 'er': graphs.er(300, 900, 2)[0],
            'loops_dangling': graphs.loops_dangling()[0], 'directed_weighted': graphs.directed_weighted_attrs()[0],
            'directed_unweighted': graphs.directed_unweighted()[0], 'star': star}


def memberships(n: int, r: int, ld: int = None, seed: int = 0) -> np.ndarray:
    """n x ld table of mixed signs with exact zeros sprinkled in; the first r columns are the memberships."""
    rng = np.random.default_rng(seed + 1000 * r)
    P = rng.uniform(-0.5, 1.0, size=(n, ld or r))
    P[rng.random(P.shape) < 0.1] = 0.0
    return P
