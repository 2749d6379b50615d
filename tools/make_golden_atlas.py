#!/usr/bin/env python3
"""
tools/make_golden_atlas.py -- the small-graph atlas fixture (tests/golden/atlas_union.npz) from networkx's bundled
Atlas of Graphs (``nx.graph_atlas_g()``: all 1253 graphs on 0-7 nodes up to isomorphism) on a CPU host:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_atlas.py

The fixture is the disjoint union of atlas graphs 1 .. 1252 (the null graph left out) in atlas order -- node ``offset[a]
+ v`` is node v of atlas graph a -- with a seeded relabelling that interleaves the components in id space, a seeded
orientation and seeded integer weights per edge, and those networkx columns that are too slow to recompute in a test
over the whole union (betweenness 23 s, constraint 2.9 s, effective size 533 s there): they are computed here one atlas
graph at a time (<= 7 nodes each) and placed by label.  All of them are local to a component, so the value on the union
is the value on the atlas graph: unnormalised betweenness (plain, with endpoints, directed, weighted), constraint and
effective size (plain and weighted).  Everything else networkx computes on the union in a fraction of a second and the
tests compute at run time.  tests/atlas.py reads the file; tests/test_atlas_cpu.py checks it against
``nx.graph_atlas_g()`` regenerated and recomputes a sample of the stored columns.  networkx is the only source.
"""
import os

import networkx as nx
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'atlas_union.npz')
SEED = 1253
#: orientation codes of the directed variant
FORWARD, BACKWARD, BOTH = 0, 1, 2


def union_edges():
    """(src, dst, atlas_id) of the disjoint union in atlas order."""
    src, dst, atlas_id = [], [], []
    offset = 0
    for a, g in enumerate(nx.graph_atlas_g()):
        if a == 0:
            continue
        k = g.number_of_nodes()
        assert sorted(g) == list(range(k))
        for u, v in g.edges():
            src.append(offset + u)
            dst.append(offset + v)
        atlas_id += [a] * k
        offset += k
    return np.asarray(src, dtype=np.int32), np.asarray(dst, dtype=np.int32), np.asarray(atlas_id, dtype=np.int16)


def small_graphs(src, dst, atlas_id, orient, weight):
    """Per atlas graph (in atlas order, local node ids): the undirected graph with its weights and the oriented one."""
    first = np.concatenate([[0], np.flatnonzero(np.diff(atlas_id)) + 1])
    sizes = np.diff(np.concatenate([first, [len(atlas_id)]]))
    owner = np.searchsorted(first, src, side='right') - 1
    out = []
    for i, (lo, k) in enumerate(zip(first.tolist(), sizes.tolist())):
        G, D = nx.Graph(), nx.DiGraph()
        G.add_nodes_from(range(k))
        D.add_nodes_from(range(k))
        for e in np.flatnonzero(owner == i).tolist():
            u, v = int(src[e]) - lo, int(dst[e]) - lo
            G.add_edge(u, v, weight=int(weight[e]))
            if orient[e] in (FORWARD, BOTH):
                D.add_edge(u, v)
            if orient[e] in (BACKWARD, BOTH):
                D.add_edge(v, u)
        out.append((lo, k, G, D))
    return out


def slow_columns(G, D):
    """The stored networkx columns of one atlas graph: name -> {node: value}."""
    isolated = {v: float('nan') for v in G if G.degree(v) == 0}          # networkx: NaN (constraint) or an error
    H = G.subgraph([v for v in G if v not in isolated])
    return {
        'betweenness': nx.betweenness_centrality(G, normalized=False),
        'betweenness_endpoints': nx.betweenness_centrality(G, normalized=False, endpoints=True),
        'betweenness_directed': nx.betweenness_centrality(D, normalized=False),
        'betweenness_weighted': nx.betweenness_centrality(G, normalized=False, weight='weight'),
        'constraint': {**nx.constraint(H), **isolated},
        'constraint_weighted': {**nx.constraint(H, weight='weight'), **isolated},
        'effective_size': {**nx.effective_size(H), **isolated},
        'effective_size_weighted': {**nx.effective_size(H, weight='weight'), **isolated},
    }


def structure():
    """The arrays that need no networkx algorithm: the union's edges and the seeded relabelling, orientation and
    weights (a fraction of a second; tests/test_atlas_cpu.py regenerates them)."""
    src, dst, atlas_id = union_edges()
    n, m = len(atlas_id), len(src)
    rng = np.random.default_rng(SEED)
    perm = rng.permutation(n).astype(np.int32)
    orient = rng.integers(0, 3, size=m).astype(np.uint8)
    weight = rng.integers(1, 4, size=m).astype(np.uint8)
    return dict(src=src, dst=dst, atlas_id=atlas_id, perm=perm, orient=orient, weight=weight)


def build():
    base = structure()
    src, dst, atlas_id, orient, weight = (base[k] for k in ('src', 'dst', 'atlas_id', 'orient', 'weight'))
    n = len(atlas_id)
    columns = {}
    for lo, k, G, D in small_graphs(src, dst, atlas_id, orient, weight):
        for name, values in slow_columns(G, D).items():
            col = columns.setdefault(name, np.full(n, np.nan))
            for v in range(k):
                col[lo + v] = values[v]
    return dict(**base, seed=np.int64(SEED), networkx_version=np.str_(nx.__version__), **columns)


def main():
    arrays = build()
    if os.path.exists(OUT):                                     # say whether the committed fixture is reproduced
        with np.load(OUT) as old:
            changed = [k for k in arrays if k not in old.files or not np.array_equal(old[k], arrays[k], equal_nan=(
                np.asarray(arrays[k]).dtype.kind == 'f'))] + [k for k in old.files if k not in arrays]
        print('reproduces the existing fixture array for array' if not changed else f'differs from the existing '
              f'fixture in {changed}')
    np.savez_compressed(OUT, **arrays)
    n, m = len(arrays['atlas_id']), len(arrays['src'])
    print(f'{n} nodes, {m} edges, {len(np.unique(arrays["atlas_id"]))} atlas graphs -> '
          f'{os.path.relpath(OUT, ROOT)} {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    main()
