"""
Weighted shortest-path distances on one GPU (grx_weighted_distances in csrc/grx_sssp.hip), one JSON line:

--case ba: BA 1 M nodes, m = 10 (the edges of the BASELINE graph, synth.ba_edges(1_000_000, 10, 0)); --case grid: the
4-neighbour grid of isqrt(n) x isqrt(n) nodes, a graph whose lightest paths have thousands of arcs.  Both with seeded
uniform weights in [0.05, 1) and --sources random sources (1 024 by default).  For every --batch value: each run timed
on its own between two device synchronisations after --warmup warm-ups, all --reps runs listed with their median and
spread, the rounds run and the time per round, and the distance bytes a round gathers (every arc reads its tail's 8 S
bytes) over the time.  For scale: the same sources through kernels.distance_sums (the bitset BFS of the unweighted
closeness: one bit of state per source where this keeps 64) on the same CSR.  --check rows are compared with scipy's
Dijkstra.

    python tools/bench_weighted_distances.py [--case ba] [--n 1000000] [--m 10] [--sources 1024] [--batch 0]
                                             [--reps 5] [--warmup 1] [--check 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, reps):
    import torch
    times, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times, out


def _summary(times):
    return {'median_ms': round(float(np.median(times)), 2), 'min_ms': round(min(times), 2),
            'max_ms': round(max(times), 2), 'runs_ms': [round(t, 2) for t in times]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='ba', choices=('ba', 'grid'))
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--m', type=int, default=10)
    ap.add_argument('--sources', type=int, default=1024)
    ap.add_argument('--batch', default='0', help='comma-separated sources per batch (16, 32, 64; 0 = the library\'s choice)')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--check', type=int, default=4, help='rows compared with scipy.sparse.csgraph.dijkstra')
    ap.add_argument('--label', default='', help='copied into the result line')
    args = ap.parse_args()

    from graphrole_amd import kernels as K, measures, synth
    from graphrole_amd.graph.csr import CSRGraph
    if args.case == 'ba':
        n = args.n
        src, dst = synth.ba_edges(n, args.m, 0)
    else:
        side = int(np.sqrt(args.n))
        n = side * side
        ids = np.arange(n, dtype=np.int64).reshape(side, side)
        src = np.concatenate([ids[:, :-1].ravel(), ids[:-1, :].ravel()])
        dst = np.concatenate([ids[:, 1:].ravel(), ids[1:, :].ravel()])
    weights = np.random.default_rng(1).uniform(0.05, 1.0, size=len(src))
    graph = measures._adapter(CSRGraph(n, src, dst, weights, validate=False))
    host, out, _ = graph._device_graph()
    sources = np.asarray(host.inv)[np.random.default_rng(0).choice(host.n, size=args.sources, replace=False)]
    row = {'label': args.label, 'case': args.case, 'n': host.n, 'arcs': out.nnz, 'hub_rows': out.n_hubs, 'sources': args.sources,
           'weighted': {}}
    first = None
    for batch in [int(b) for b in args.batch.split(',') if b != '']:
        fn = lambda: K.weighted_distances(out, sources, batch)                     # noqa: E731
        for _ in range(args.warmup):
            fn()
        times, (reach, dsum, harmonic, far, ecc, _, rounds) = _timed(fn, args.reps)
        S = batch or (16 if args.sources <= 16 else 32 if args.sources <= 32 else 64)
        median_s = float(np.median(times)) * 1e-3
        gathered = rounds * out.nnz * 8 * S
        bits = [K.to_host(t)[:host.n].tobytes() for t in (reach, dsum, harmonic, far)]
        first = first or bits
        row['weighted'][f'batch={batch}'] = dict(
            _summary(times), lanes=S, batches=-(-args.sources // S), rounds=rounds,
            ms_per_round=round(median_s * 1e3 / rounds, 3), state_bytes=host.n * (16 * S + 4),
            gather_bytes_per_round_every_arc=out.nnz * 8 * S,
            every_arc_gather_TB_per_s=round(gathered / median_s / 1e12, 3),
            largest_source_ecc=float(K.to_host(ecc).max()), same_bits_as_first=bits == first)
    if args.check:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import dijkstra
        some = sources[:args.check]
        dist = K.to_host(K.weighted_distances(out, some, want_matrix=True)[5])
        A = csr_matrix((K.to_host(out.w)[:out.nnz], K.to_host(out.col)[:out.nnz], K.to_host(out.row_ptr)),
                       shape=(host.n, host.n))
        want = dijkstra(A, directed=False, indices=some)
        row['scipy_rows'] = {'rows': int(args.check), 'equal_bits': bool(dist.tobytes() == want.tobytes()),
                             'max_abs_diff': float(np.max(np.abs(dist - want)))}
    K.distance_sums(out, sources)
    bfs_times, _ = _timed(lambda: K.distance_sums(out, sources), args.reps)
    row['unweighted_distance_sums'] = _summary(bfs_times)
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
