"""
Closeness / harmonic centrality timings on one GPU (csrc/grx_closeness.hip), one JSON line per case:

- er100k_exact: node_measures(er, ['closeness_centrality', 'harmonic_centrality']) on ER 100 k (m = 1 M): both
  columns from one multi-source BFS pass over every source, end to end (adapter, device graph, kernels, frame), cold
  and warm;
- ba1m_batch: BA 1 M (m = 10), kernels.distance_sums from --batches batches of 64 W sources for W = 1, 2, 4, 8, 16:
  ms per batch, and the 64 W-bit frontier rows gathered per second as an UPPER BOUND (every arc once per level, no
  early exit, levels = the BFS depth from row 0 + 2) against the 62.4 G rows/s random-gather ceiling of
  profiles/r05_aggregation_experiments.txt;
- ba1m_exact: graphrole_amd.closeness_centrality(g) on BA 1 M, every node a source, end to end;
- networkx: nx.single_source_shortest_path_length (what closeness_centrality runs per node) on BA 1 M on this host's
  CPU (--networkx sources; 0 = skip).

    python tools/bench_closeness.py [--cases er100k_exact,ba1m_batch,ba1m_exact,networkx] [--batches 2]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GATHER_ROWS_PER_S = 62.4e9


def _depth(row_ptr, col, s, n):
    """BFS depth from s (for the rows-per-level accounting only)."""
    D = np.full(n, -1, dtype=np.int64)
    D[s] = 0
    frontier, depth = np.array([s]), 0
    while True:
        deg = row_ptr[frontier + 1] - row_ptr[frontier]
        idx = np.repeat(row_ptr[frontier] - np.cumsum(deg) + deg, deg) + np.arange(int(deg.sum()))
        nb = np.unique(col[idx])
        nb = nb[D[nb] < 0]
        if not len(nb):
            return depth
        depth += 1
        D[nb] = depth
        frontier = nb


def _timed(fn, reps):
    import torch
    times = []
    out = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times, out


def batch_case(g, batches, reps):
    from graphrole_amd import kernels as K
    from graphrole_amd.graph.interface.csr import CSRInterface
    graph = CSRInterface(g)
    host, out, _ = graph._device_graph()
    inv = np.asarray(host.inv)
    depth = _depth(np.asarray(g.row_ptr), np.asarray(g.col), 0, g.n)
    rows = []
    for W in (1, 2, 4, 8, 16):
        count = 64 * W * batches
        sources = inv[random.Random(W).sample(range(g.n), count)]
        K.distance_sums(out, sources[:64 * W], words=W)                      # warm-up
        times, _ = _timed(lambda: K.distance_sums(out, sources, words=W), reps)
        ms = float(np.median(times))
        bound = out.nnz * (depth + 2) * batches                              # 64 W-bit rows, no early exit
        rows.append({'W': W, 'sources': count, 'ms': round(ms, 2), 'ms_per_batch': round(ms / batches, 3),
                     'us_per_source': round(ms * 1e3 / count, 2),
                     'rows_per_s_bound_G': round(bound / (ms * 1e-3) / 1e9, 2),
                     'bytes_per_s_bound_TB': round(bound * 8 * W / (ms * 1e-3) / 1e12, 2)})
    return {'case': 'ba1m_batch', 'n': g.n, 'arcs': out.nnz, 'bfs_depth_from_row0': depth, 'runs': rows,
            'gather_ceiling_G_rows_per_s': GATHER_ROWS_PER_S / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='er100k_exact,ba1m_batch,ba1m_exact,networkx')
    ap.add_argument('--batches', type=int, default=2)
    ap.add_argument('--networkx', type=int, default=2)
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    from graphrole_amd import closeness_centrality, node_measures, synth
    cases = args.cases.split(',')
    ba = synth.ba_graph(1_000_000, 10, seed=0) if any(c.startswith('ba1m') or c == 'networkx' for c in cases) else None
    if 'er100k_exact' in cases:
        er = synth.er_graph(100_000, 1_000_000, seed=0)
        times, M = _timed(lambda: node_measures(er, ['closeness_centrality', 'harmonic_centrality']), 2)
        print(json.dumps({'case': 'er100k_exact', 'n': er.n, 'cold_ms': round(times[0], 1),
                          'warm_ms': round(times[1], 1), 'us_per_source': round(times[1] * 1e3 / er.n, 2),
                          'max_closeness': float(M['closeness_centrality'].max()),
                          'max_harmonic': float(M['harmonic_centrality'].max())}), flush=True)
    if 'ba1m_batch' in cases:
        print(json.dumps(batch_case(ba, args.batches, args.reps)), flush=True)
    if 'ba1m_exact' in cases:
        times, c = _timed(lambda: closeness_centrality(ba), 1)
        print(json.dumps({'case': 'ba1m_exact', 'n': ba.n, 'ms': round(times[0], 1),
                          'us_per_source': round(times[0] * 1e3 / ba.n, 2), 'max': float(c.max()),
                          'min': float(c.min())}), flush=True)
    if 'networkx' in cases and args.networkx > 0:
        import networkx as nx
        t0 = time.perf_counter()
        G = nx.Graph()
        G.add_nodes_from(range(ba.n))
        src, dst, _ = ba.edge_arrays()
        G.add_edges_from(zip(src.tolist(), dst.tolist()))
        build_s = time.perf_counter() - t0
        times = []
        for s in random.Random(0).sample(range(ba.n), args.networkx):
            t0 = time.perf_counter()
            sp = nx.single_source_shortest_path_length(G, s)
            sum(sp.values())
            times.append(time.perf_counter() - t0)
        per = float(np.mean(times))
        print(json.dumps({'case': 'networkx', 'graph_build_s': round(build_s, 1), 'sources': args.networkx,
                          's_per_source': round(per, 2), 'exact_closeness_h': round(per * ba.n / 3600, 1)}),
              flush=True)


if __name__ == '__main__':
    main()
