"""
Edge betweenness against node betweenness on one GPU, one process, one JSON line and the lines of
profiles/edge_betweenness.txt:

BA 1 M nodes, m = 10 (synth.ba_edges(1_000_000, 10, 0)) and the --sources sources random.Random(0) samples (what
edge_betweenness_centrality(G, k=1024, seed=0) runs).  After --warmup warm-ups, --reps runs of each of
  grx_betweenness, grx_edge_betweenness                              (hops)
  grx_weighted_betweenness, grx_weighted_edge_betweenness            (uniform weights, then integer weights 1..5)
each run timed on its own between two device synchronisations, on the same CSR and the same sources.  The yardstick of
an edge call is the node call of the same run: `share` = (edge - node) / edge by the medians is what the kept coeff
array, the edge pass and the final passes over the arcs cost together.  `gather_bytes_per_batch` is what the edge pass
reads from the cell arrays for one batch: always the level / depth word of both ends of every arc for every lane, and
the rest (sigma or D of the row, coeff -- and D -- of the neighbour) only where a lane has a DAG arc, so `..._max`
counts every lane.

    python tools/time_edge_betweenness.py [--n 1000000] [--m 10] [--sources 1024] [--reps 5] [--warmup 1]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return {'min_ms': round(min(times), 1), 'max_ms': round(max(times), 1), 'median_ms': round(float(np.median(times)), 1),
            'runs_ms': [round(t, 1) for t in times]}


def _pair(node, edge, arcs, lanes, always, at_most):
    share = (edge['median_ms'] - node['median_ms']) / edge['median_ms']
    return {'node': node, 'edge': edge, 'edge_over_node': round(edge['median_ms'] / node['median_ms'], 3),
            'share': round(share, 3), 'lanes': lanes, 'gather_bytes_per_batch_always': arcs * lanes * always,
            'gather_bytes_per_batch_max': arcs * lanes * at_most}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--m', type=int, default=10)
    ap.add_argument('--sources', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    args = ap.parse_args()

    from graphrole_amd import kernels as K, measures, synth
    from graphrole_amd.graph.csr import CSRGraph
    src, dst = synth.ba_edges(args.n, args.m, 0)
    picked = random.Random(0).sample(list(range(args.n)), args.sources)
    row = {'n': args.n, 'm': args.m, 'sources': args.sources, 'reps': args.reps}
    lines = []
    for kind in ('hops', 'uniform', 'ints'):
        rng = np.random.default_rng(1)
        w = None if kind == 'hops' else (rng.uniform(0.05, 1.0, size=len(src)) if kind == 'uniform'
                                         else rng.integers(1, 6, size=len(src)).astype(np.float64))
        graph = measures._adapter(CSRGraph(args.n, src, dst, w, validate=False))
        host, out, _ = graph._device_graph()
        sources = np.asarray(host.inv)[picked]
        if kind == 'hops':
            node = _timed(lambda: K.betweenness(out, None, sources, False, 1.0), args.reps, args.warmup)
            edge = _timed(lambda: K.edge_betweenness(out, None, sources, 1.0), args.reps, args.warmup)
            lanes = min(256, ((4 << 30) // (28 * host.n)) // 64 * 64)
            row[kind] = _pair(node, edge, out.nnz, lanes, 8, 24)
        else:
            node = _timed(lambda: K.weighted_betweenness(out, None, sources, False, 1.0), args.reps, args.warmup)
            edge = _timed(lambda: K.weighted_edge_betweenness(out, None, sources, 1.0), args.reps, args.warmup)
            row[kind] = _pair(node, edge, out.nnz, 64, 8, 40)
        r = row[kind]
        lines.append(f"{kind:8s} node {r['node']['min_ms']:8.1f} - {r['node']['max_ms']:8.1f} ms   "
                     f"edge {r['edge']['min_ms']:8.1f} - {r['edge']['max_ms']:8.1f} ms   edge / node "
                     f"{r['edge_over_node']:.3f}   share of the edge pass {r['share']:.3f}   lanes {r['lanes']}   gathers "
                     f"per batch {r['gather_bytes_per_batch_always'] / 1e9:.2f} GB always, at most "
                     f"{r['gather_bytes_per_batch_max'] / 1e9:.2f} GB")
        del graph, host, out
    print(json.dumps(row), flush=True)
    print('\n'.join(lines), flush=True)


if __name__ == '__main__':
    main()
