"""
Plain numpy restatement of csrc/grx_components.hip on CSR arrays (row_ptr, col) of a graph's distinct arcs (self-loop
entries allowed, weights never read), and the case builders the CPU and the GPU tests of the components share.

* ``components(row_ptr, col, mode=...)``: label[v] = the smallest row of v's component, size[v] = its cardinality, the
  number of components, and for STRONG the rounds and outer iterations of the kernel's own method, round for round:

      TRIM    every alive node without an alive out-neighbour other than itself, or without such an in-neighbour, leaves
              with label = own id (aliveness as at the start of the round); again until a round removes nobody
      COLOUR  colour[v] = min(colour[v], colour[u] over the alive in-neighbours u) from colour[v] = v, every round on the
              colours of the round before, until a round changes nothing
      CLOSE   from the pivots (colour[v] == v) backward over in-arcs inside the colour, one level a round, until a round
              adds nobody
      REMOVE  one round: every node reached gets label = colour and leaves; TRIM again while anybody is alive

  The loop ends in the TRIM or REMOVE round after which nobody is alive; every round counts.  CONNECTED / WEAK are a
  union of the arcs (scipy-free: label propagation to the minimum, whole-array numpy), 0 rounds.
* ``reachable(row_ptr, col, flag)``: the level-synchronous closure of grx_reachable: (flag 0 / 1, count, levels).
* ``bow_tie(row_ptr, col, in_row_ptr, in_col)``: the six categories of graphrole_amd.components.bow_tie from one STRONG
  result and four closures, as category codes.

Every round is a handful of whole-array numpy calls, so 1 M rows take seconds.  Used by tests and tools only.
"""
import functools
import itertools
from collections import namedtuple

import networkx as nx
import numpy as np

from tests.kcore_oracle import directed_csr, symmetric_csr

CONNECTED, WEAK, STRONG = 'connected', 'weak', 'strong'
ROUND_BATCH = 16                                               # CP_ROUND_BATCH of csrc/grx_components.hip
BOW_TIE = ('core', 'in', 'out', 'tube', 'tendril', 'other')

Result = namedtuple('Result', 'label size n_components rounds outer')


def arcs_of(row_ptr, col):
    """(src, dst) int64 of the CSR's entries."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n = len(row_ptr) - 1
    return np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr)), np.asarray(col, dtype=np.int64)[:row_ptr[-1]]


def transpose(row_ptr, col):
    """(row_ptr, col) of the transposed CSR, ascending in each row."""
    src, dst = arcs_of(row_ptr, col)
    return directed_csr(len(row_ptr) - 1, np.stack([dst, src], axis=1))


def _sizes(label):
    n = len(label)
    count = np.bincount(label, minlength=n) if n else np.zeros(0, dtype=np.int64)
    return count[label].astype(np.int64), int(np.count_nonzero(label == np.arange(n)))


def _union(n, src, dst):
    """label[v] = the smallest id joined to v by the arcs, either way: minimum propagation with pointer jumping."""
    label = np.arange(n, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, src, label[dst])
        np.minimum.at(new, dst, label[src])
        new = new[new]
        if np.array_equal(new, label):
            return label
        label = new


def _strong(n, src, dst, _trace=None):
    ids = np.arange(n, dtype=np.int64)
    label = np.full(n, -1, dtype=np.int64)
    alive = np.ones(n, dtype=bool)
    proper = src != dst
    rounds = outer = 0
    trace = _trace if _trace is not None else {}
    gone, trimmed = trace.setdefault('gone', np.zeros(n, dtype=np.int64)), trace.setdefault('trimmed', np.zeros(n, dtype=bool))
    while alive.any():
        while True:                                             # TRIM
            rounds += 1
            a = alive[src] & alive[dst] & proper
            has_out = np.bincount(src[a], minlength=n) > 0
            has_in = np.bincount(dst[a], minlength=n) > 0
            leave = alive & ~(has_out & has_in)
            label[leave] = ids[leave]
            gone[leave], trimmed[leave] = rounds, True
            alive &= ~leave
            if not alive.any():
                return label, rounds, outer
            if not leave.any():
                break
        colour = ids.copy()
        a = alive[src] & alive[dst]
        s, d = src[a], dst[a]
        while True:                                             # COLOUR
            rounds += 1
            new = colour.copy()
            np.minimum.at(new, d, colour[s])
            changed = bool((new != colour)[alive].any())
            colour = new
            if not changed:
                break
        reached = alive & (colour == ids)
        frontier = reached.copy()
        same = colour[s] == colour[d]
        while True:                                             # CLOSE
            rounds += 1
            hit = frontier[d] & same & ~reached[s]
            new = np.zeros(n, dtype=bool)
            new[s[hit]] = True
            reached |= new
            frontier = new
            if not new.any():
                break
        rounds += 1                                             # REMOVE
        label[reached] = colour[reached]
        gone[reached] = rounds
        alive &= ~reached
        outer += 1
    return label, rounds, outer


def components(row_ptr, col, mode=CONNECTED) -> Result:
    src, dst = arcs_of(row_ptr, col)
    n = len(row_ptr) - 1
    if n == 0:
        return Result(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64), 0, 0, 0)
    if mode == STRONG:
        label, rounds, outer = _strong(n, src, dst)
    else:
        label, rounds, outer = _union(n, src, dst), 0, 0
    size, count = _sizes(label)
    return Result(label.astype(np.int32), size, count, rounds, outer)


def strong_trace(row_ptr, col):
    """(gone int64[n] = the round every row leaves in, trimmed bool[n] = it left in a TRIM round) of the STRONG method."""
    src, dst = arcs_of(row_ptr, col)
    trace = {}
    _strong(len(row_ptr) - 1, src, dst, trace)
    return trace['gone'], trace['trimmed']


def reachable(row_ptr, col, flag):
    """(flag int32 0 / 1, count, levels) of the closure of the rows with flag != 0 along the CSR's arcs."""
    src, dst = arcs_of(row_ptr, col)
    level = np.where(np.asarray(flag) != 0, 0, -1)
    depth = 0
    while True:
        new = np.unique(dst[(level[src] == depth) & (level[dst] < 0)])
        if not len(new):
            break
        depth += 1
        level[new] = depth
    out = (level >= 0).astype(np.int32)
    return out, int(out.sum()), depth


def _closure(row_ptr, col, member):
    return reachable(row_ptr, col, member.astype(np.int32))[0].astype(bool)


def bow_tie(row_ptr, col, in_row_ptr, in_col, first_of=None):
    """Category codes (indices into BOW_TIE) of every row.  S = the largest strongly connected component, ties by the
    smallest of first_of[label] (default: the label itself, the smallest row)."""
    r = components(row_ptr, col, STRONG)
    n = len(r.label)
    if n == 0:
        return np.zeros(0, dtype=np.int8)
    roots = np.nonzero(r.label == np.arange(n))[0]
    key = roots if first_of is None else np.asarray(first_of)[roots]
    best = roots[np.lexsort((key, -r.size[roots]))[0]]
    core = r.label == best
    reaches = _closure(in_row_ptr, in_col, core)                # ancestors of S, S included
    reached = _closure(row_ptr, col, core)                      # descendants of S, S included
    inn, out = reaches & ~core, reached & ~core
    from_in = _closure(row_ptr, col, inn)
    to_out = _closure(in_row_ptr, in_col, out)
    rest = ~(core | inn | out)
    code = np.full(n, 5, dtype=np.int8)
    code[rest & (from_in ^ to_out)] = 4
    code[rest & from_in & to_out] = 3
    code[out], code[inn], code[core] = 2, 1, 0
    return code


# ---------------------------------------------------------------------------------------------------- case builders
def graph_csrs(G, nodes=None):
    """(nodes, row_ptr, col, in_row_ptr, in_col) of a networkx graph -- a multigraph's parallel edges once, self-loops
    kept -- rows in `nodes` order (default list(G)); the in CSR is None for an undirected graph."""
    nodes = list(G) if nodes is None else list(nodes)
    row_of = {v: i for i, v in enumerate(nodes)}
    edges = [(row_of[u], row_of[v]) for u, v in G.edges()]
    if not G.is_directed():
        return (nodes,) + symmetric_csr(len(nodes), edges) + (None, None)
    out = directed_csr(len(nodes), edges)
    return (nodes,) + out + transpose(*out)


def interleave(graphs):
    """The disjoint union of equally large CSRs (row_ptr, col) on n0 rows each with INTERLEAVED ids: row j of graph c is
    row j * C + c.  (n, row_ptr, col)."""
    C = len(graphs)
    n0 = len(graphs[0][0]) - 1
    arcs = []
    for c, (row_ptr, col) in enumerate(graphs):
        src, dst = arcs_of(row_ptr, col)
        arcs.append(np.stack([src * C + c, dst * C + c], axis=1))
    arcs = np.concatenate(arcs) if arcs else np.zeros((0, 2), dtype=np.int64)
    return (n0 * C,) + directed_csr(n0 * C, arcs)


@functools.lru_cache(maxsize=None)
def all_digraphs4():
    """The 4 096 digraphs on 4 nodes (every subset of the 12 arcs without loops) as one union of 16 384 rows."""
    pairs = [(u, v) for u in range(4) for v in range(4) if u != v]
    graphs = [directed_csr(4, [p for k, p in enumerate(pairs) if bits >> k & 1]) for bits in range(1 << 12)]
    return interleave(graphs)


@functools.lru_cache(maxsize=None)
def all_graphs5():
    """The 1 024 graphs on 5 nodes as one union of 5 120 rows (symmetric CSR)."""
    pairs = list(itertools.combinations(range(5), 2))
    graphs = [symmetric_csr(5, [p for k, p in enumerate(pairs) if bits >> k & 1]) for bits in range(1 << 10)]
    return interleave(graphs)


def directed_family(seed):
    """Seeded G(n, m) digraphs, n <= 28, at sparse, critical and dense densities, the last two with self-loops."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 29))
    for k, m in enumerate((n // 2, n, int(1.5 * n), min(4 * n, n * (n - 1)))):
        G = nx.gnm_random_graph(n, m, seed=seed * 7 + k, directed=True)
        if k >= 2:
            G.add_edges_from((int(v), int(v)) for v in rng.integers(0, n, size=3))
        yield G


def undirected_family(seed):
    """The undirected families of tests/test_kcore_cpu.py that can be disconnected, some with self-loops."""
    import random
    rng = random.Random(seed)
    n = rng.randint(2, 28)
    yield nx.gnm_random_graph(n, rng.randint(0, 2 * n), seed=seed)
    yield nx.gnm_random_graph(n, rng.randint(n // 2, n + 2), seed=seed + 1)
    yield nx.random_labeled_tree(n, seed=seed)
    G = nx.disjoint_union(nx.gnm_random_graph(n, n // 2 + rng.randint(0, n), seed=seed + 2),
                          nx.disjoint_union(nx.cycle_graph(rng.randint(3, 9)), nx.empty_graph(2)))
    G.add_edge(0, 0)
    yield G
    H = nx.gnm_random_graph(n, rng.randint(n // 3, n), seed=seed + 4)
    yield nx.relabel_nodes(H, dict(zip(H, rng.sample(list(H), len(H)))))


def cycle(k):
    return directed_csr(k, [(i, (i + 1) % k) for i in range(k)])


def path(k):
    return directed_csr(k, [(i, i + 1) for i in range(k - 1)])


def two_cycle_chain(k, ascending=True):
    """k two-cycles {2 i, 2 i + 1} joined by the arcs 2 i + 1 -> 2 i + 2: ids ascend along the chain (one component
    peeled per outer iteration: the known worst case), or -- relabelled v -> 2 k - 1 - v -- descend."""
    arcs = []
    for i in range(k):
        arcs += [(2 * i, 2 * i + 1), (2 * i + 1, 2 * i)]
        if i + 1 < k:
            arcs.append((2 * i + 1, 2 * i + 2))
    a = np.asarray(arcs, dtype=np.int64)
    return directed_csr(2 * k, a if ascending else 2 * k - 1 - a)


HUB_CASES = ('scc_out', 'scc_in', 'source_out', 'sink_in', 'sink_out', 'source_in')


def hub_case(kind, arms=150):
    """A digraph on arms + 4 rows whose row 0 has `arms` arcs (a hub row above 32 * 4 lanes) in the out CSR
    ('..._out') or, with every arc reversed, in the in CSR ('..._in'); rows 1 .. 3 are a 3-cycle.
    'scc_out' / 'scc_in': the hub lies on cycles through its arms (all return through row 1).
    'source_out' / 'sink_in': the hub's other row is empty, so it is trimmed in round 1 by that short row, and its arms
    after it.
    'sink_out' / 'source_in': the hub's long row leads to `arms` sinks (comes from `arms` sources) and the 3-cycle has an
    arc into (out of) the hub: the arms leave in round 1, the hub in round 2 -- because of its LONG row, which is then
    without an alive entry, while the neighbour in its short row is still alive."""
    base, where = kind.split('_')
    n = arms + 4
    leaves = list(range(4, n))
    star = [(0, v) for v in leaves]
    ring = [(1, 2), (2, 3), (3, 1)]
    if base == 'scc':
        arcs, flip = star + [(v, 1) for v in leaves[::2]] + [(1, 0)] + ring, where == 'in'
    elif (base, where) in (('source', 'out'), ('sink', 'in')):
        arcs, flip = star + [(leaves[0], 1), (leaves[1], leaves[2])] + ring, where == 'in'
    else:                                                       # ('sink', 'out'), ('source', 'in')
        arcs, flip = star + [(1, 0)] + ring, where == 'in'
    a = np.asarray(arcs, dtype=np.int64)
    return directed_csr(n, a[:, ::-1] if flip else a)


def motif():
    """The small directed motif of the second-trip test: a hub (row 0, 140 out-arcs) on cycles through a third of its
    arms and rows 1 .. 3 (the other arms are sinks, trimmed at once), a tail that leads from there into a 3-cycle (the
    tail is trimmed and the cycle found in a second outer iteration), and an isolated row.  (row_ptr, col)."""
    arms = 140
    n = arms + 12
    leaves = list(range(4, 4 + arms))
    arcs = [(0, v) for v in leaves] + [(v, 1) for v in leaves[::3]] + [(1, 0), (1, 2), (2, 3), (3, 1)]
    t = 4 + arms
    arcs += [(3, t), (t, t + 1), (t + 1, t + 2), (t + 2, t + 3)]              # the tail
    arcs += [(t + 3, t + 4), (t + 4, t + 5), (t + 5, t + 6), (t + 6, t + 4)]  # into the 3-cycle
    return directed_csr(n, arcs)                                              # row n - 1: isolated


def partition(label):
    """The partition a label array stands for: a frozenset of frozensets of rows."""
    groups = {}
    for v, l in enumerate(np.asarray(label).tolist()):
        groups.setdefault(l, []).append(v)
    return frozenset(frozenset(g) for g in groups.values())
