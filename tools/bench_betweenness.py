"""
Betweenness centrality timings on one GPU (csrc/grx_betweenness.hip), one JSON line per case:

- ba1m_batch: BA 1 M (m = 10) from --sources sources, with B = 64 and with the library's default B: ms per batch and
  per source, and the arcs pulled per second against the 62.4 G rows/s random-gather ceiling of
  profiles/r05_aggregation_experiments.txt (one "row" here = one 64-lane chunk of a neighbour's cells);
- ba1m_k1024: graphrole_amd.betweenness_centrality(g, k=1024, seed=0) end to end (adapter, device graph, sources,
  kernels, result Series), cold and warm;
- er100k_exact: exact betweenness (every node a source) on ER 100 k (m = 1 M);
- networkx: nx.betweenness_centrality's per-source loops on BA 1 M on this host's CPU (--networkx sources; 0 = skip).

    python tools/bench_betweenness.py [--cases ba1m_batch,ba1m_k1024,er100k_exact,networkx] [--sources 256]
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
    """BFS depth from s (for the arcs-per-level accounting only)."""
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


def batch_case(g, n_sources, reps):
    import torch
    from graphrole_amd import kernels as K
    from graphrole_amd.graph.interface.csr import CSRInterface
    graph = CSRInterface(g)
    host, out, _ = graph._device_graph()
    sources = np.asarray(host.inv)[random.Random(0).sample(range(g.n), n_sources)]
    lib = K._lib.load()
    rows = []
    for batch in (64, 0):
        K.betweenness(out, None, sources[:64], False, 1.0, batch=batch)          # warm-up
        times = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            K.betweenness(out, None, sources, False, 1.0, batch=batch)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        ms = float(np.median(times))
        # the library's B: its workspace is 20 n B bytes plus a few KiB
        B = batch or lib.grx_betweenness_workspace_bytes(g.n, 0, n_sources) // (20 * g.n)
        batches = -(-n_sources // B)
        rows.append({'B': int(B), 'batches': batches, 'ms': round(ms, 2), 'ms_per_batch': round(ms / batches, 3),
                     'ms_per_source': round(ms / n_sources, 4)})
    return rows, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='ba1m_batch,ba1m_k1024,er100k_exact,networkx')
    ap.add_argument('--sources', type=int, default=256)
    ap.add_argument('--networkx', type=int, default=2)
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    import torch
    from graphrole_amd import betweenness_centrality, synth
    cases = args.cases.split(',')
    ba = synth.ba_graph(1_000_000, 10, seed=0) if any(c.startswith('ba1m') or c == 'networkx' for c in cases) else None
    if 'ba1m_batch' in cases:
        rows, out = batch_case(ba, args.sources, args.reps)
        depth = _depth(ba.row_ptr, ba.col, 0, ba.n)
        for r in rows:
            # per level of one 64-lane chunk: every arc of every row not yet settled (forward) / holding a lane at the
            # level (backward) is one gathered chunk; upper bound = all arcs, twice per level (forward + backward)
            chunks = r['B'] // 64 * r['batches']
            arcs = 2 * out.nnz * (depth + 1) * chunks
            r['gather_rows_per_s_bound'] = round(arcs / (r['ms'] * 1e-3) / 1e9, 1)
        print(json.dumps({'case': 'ba1m_batch', 'n': ba.n, 'arcs': out.nnz, 'sources': args.sources,
                          'bfs_depth_from_row0': depth, 'runs': rows,
                          'gather_ceiling_G_rows_per_s': GATHER_ROWS_PER_S / 1e9}), flush=True)
    if 'ba1m_k1024' in cases:
        times = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bc = betweenness_centrality(ba, k=1024, seed=0)
            times.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({'case': 'ba1m_k1024', 'cold_ms': round(times[0], 1), 'warm_ms': round(times[1], 1),
                          'max': float(bc.max())}), flush=True)
    if 'er100k_exact' in cases:
        er = synth.er_graph(100_000, 1_000_000, seed=0)
        times = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bc = betweenness_centrality(er)
            times.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({'case': 'er100k_exact', 'n': er.n, 'cold_ms': round(times[0], 1),
                          'warm_ms': round(times[1], 1), 'ms_per_source': round(times[1] / er.n, 4),
                          'max': float(bc.max())}), flush=True)
    if 'networkx' in cases and args.networkx > 0:
        import networkx as nx
        from networkx.algorithms.centrality.betweenness import _accumulate_basic, _single_source_shortest_path_basic
        t0 = time.perf_counter()
        G = nx.Graph()
        G.add_nodes_from(range(ba.n))
        src, dst, _ = ba.edge_arrays()
        G.add_edges_from(zip(src.tolist(), dst.tolist()))
        build_s = time.perf_counter() - t0
        bc = dict.fromkeys(G, 0.0)
        times = []
        for s in random.Random(0).sample(range(ba.n), args.networkx):
            t0 = time.perf_counter()
            S, P, sigma, _ = _single_source_shortest_path_basic(G, s)
            _accumulate_basic(bc, S, P, sigma, s)
            times.append(time.perf_counter() - t0)
        print(json.dumps({'case': 'networkx', 'graph_build_s': round(build_s, 1), 'sources': args.networkx,
                          's_per_source': round(float(np.mean(times)), 2)}), flush=True)


if __name__ == '__main__':
    main()
