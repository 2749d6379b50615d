"""
Plain numpy / Python restatement of csrc/grx_biconnected.hip (Tarjan-Vishkin on a BFS spanning forest), step by step
over a CSR (row_ptr, col) of an undirected graph's distinct arcs (symmetric; self-loop entries allowed and skipped):

1. connected components, the representative of each = its smallest row id (the forest's roots);
2. multi-root BFS: level, and parent[v] = the SMALLEST row id among v's neighbours one level up (-1 for a root);
3. subtree sizes; 4. preorder numbers, siblings in row order, the trees one after another in root order;
5. low / high = min / max preorder number reachable from the subtree by one non-tree edge;
6. union-find over the tree edges (each named by its child): both ends of every non-tree edge, and (w, parent[w]) when
   the subtree of w reaches outside the subtree of parent[w]; the label of a set = its smallest member, -1 for roots;
7. count[v] = number of biconnected components that contain v.

Nothing here is fast; it exists to be compared with networkx on small graphs and with the kernels on the same CSR.
"""
from collections import namedtuple

import numpy as np

Result = namedtuple('Result', 'count parent label n_components level size pre low high')


def symmetric_csr(n, edges):
    """(row_ptr, col) of the distinct arcs of an undirected edge list over rows 0 .. n - 1, ascending in each row
    (a self-loop is one entry)."""
    arcs = set()
    for u, v in edges:
        arcs.add((int(u), int(v)))
        arcs.add((int(v), int(u)))
    arcs = sorted(arcs)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    for u, _ in arcs:
        row_ptr[u + 1] += 1
    return np.cumsum(row_ptr), np.array([v for _, v in arcs], dtype=np.int64)


def graph_csr(G):
    """(nodelist, row_ptr, col) of a networkx graph, rows in list(G) order."""
    nodes = list(G)
    row_of = {v: i for i, v in enumerate(nodes)}
    row_ptr, col = symmetric_csr(len(nodes), [(row_of[u], row_of[v]) for u, v in G.edges()])
    return nodes, row_ptr, col


def _find(p, x):
    while p[x] != x:
        p[x] = p[p[x]]
        x = p[x]
    return x


def _union(p, a, b):
    a, b = _find(p, a), _find(p, b)
    if a != b:
        p[max(a, b)] = min(a, b)


def biconnected(row_ptr, col) -> Result:
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n = len(row_ptr) - 1
    rows = [col[row_ptr[v]:row_ptr[v + 1]].tolist() for v in range(n)]
    # 1
    cc = list(range(n))
    for v in range(n):
        for w in rows[v]:
            _union(cc, v, w)
    cc = [_find(cc, v) for v in range(n)]
    roots = [v for v in range(n) if cc[v] == v]
    # 2
    level = np.full(n, -1, dtype=np.int64)
    parent = np.full(n, -1, dtype=np.int64)
    level[roots] = 0
    levels = [list(roots)]
    while levels[-1]:
        l = len(levels) - 1
        nxt = {}
        for v in levels[-1]:
            for w in rows[v]:
                if w != v and (level[w] < 0 or (level[w] == l + 1 and w in nxt)):
                    level[w] = l + 1
                    nxt[w] = min(nxt.get(w, v), v)
        for w, p in nxt.items():
            parent[w] = p
        levels.append(sorted(nxt))
    levels.pop()
    # 3
    size = np.ones(n, dtype=np.int64)
    for lv in reversed(levels[1:]):
        for v in lv:
            size[parent[v]] += size[v]
    # 4
    pre = np.zeros(n, dtype=np.int64)
    first = 0
    for r in roots:
        pre[r] = first
        first += size[r]
    for lv in levels:
        for p in lv:
            at = pre[p] + 1
            for c in rows[p]:
                if parent[c] == p:
                    pre[c] = at
                    at += size[c]
    # 5
    low, high = pre.copy(), pre.copy()
    for v in range(n):
        for w in rows[v]:
            if w != v and parent[v] != w and parent[w] != v:
                low[v] = min(low[v], pre[w])
                high[v] = max(high[v], pre[w])
    for lv in reversed(levels[1:]):
        for v in lv:
            low[parent[v]] = min(low[parent[v]], low[v])
            high[parent[v]] = max(high[parent[v]], high[v])
    # 6
    lab = list(range(n))
    for u in range(n):
        for w in rows[u]:
            if u < w and parent[u] != w and parent[w] != u:
                _union(lab, u, w)                               # BFS forest: a non-tree edge joins unrelated vertices
    for w in range(n):
        v = parent[w]
        if v >= 0 and parent[v] >= 0 and (low[w] < pre[v] or high[w] >= pre[v] + size[v]):
            _union(lab, w, v)
    label = np.array([_find(lab, v) if parent[v] >= 0 else -1 for v in range(n)], dtype=np.int64)
    # 7
    top = {}
    for c in range(n):
        p = parent[c]
        if p >= 0 and (parent[p] < 0 or label[c] != label[p]):
            assert top.setdefault(int(label[c]), int(p)) == p
    count = (parent >= 0).astype(np.int64)
    for p in top.values():
        count[p] += 1
    return Result(count, parent, label, len(top), level, size, pre, low, high)


def components(parent, label):
    """The biconnected components as a set of frozensets of row ids: component label[c] is the union of
    {c, parent[c]} over its tree edges."""
    comps = {}
    for c, (p, r) in enumerate(zip(np.asarray(parent).tolist(), np.asarray(label).tolist())):
        if p >= 0:
            comps.setdefault(r, set()).update((c, p))
    return {frozenset(s) for s in comps.values()}
