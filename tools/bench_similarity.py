"""
Structural-similarity timings on one GPU (csrc/grx_similarity.hip): JSON lines, every case timed with device events over
--reps runs after --warmup warm-ups (minimum - maximum and every run), all in one process.

- 1,024 queries against a table of --n rows (1 M: the size of the BA 1 M baseline graph) at c = 6 and c = 32, k = 10,
  both metrics, with `segments` = 1 and the library's choice; the table holds uniform random memberships (the arrival
  order of the candidates is random, the common case; the slow order -- every candidate nearer than all before it -- is
  what tests/similarity_oracle.arc builds and is not timed here);
- all pairs at --pairs-n rows (100 k), c = 6, and at --n rows with --all-pairs (otherwise the time at --n is extrapolated
  from the pair rate measured at --pairs-n and labelled as such);
- for each, the pair rate and its fraction of the bound of the file's header: 39.3 T fp64 vector operations per second
  over 2 c (cosine) resp. 3 c (Euclidean) operations per pair;
- selection and merge are not timed apart (they are not kernels of their own but the rare branch of the scan, and the
  merge launch is the difference a profiler would show): `segments` = 1 runs the same arithmetic without a merge;
- grx_neighbor_roles on the BA graph of --n nodes, m = 10, r = 6 in the same process: the familiar yardstick;
- sklearn's NearestNeighbors(algorithm='brute', n_jobs=16).kneighbors for the 1,024-query case on the host (--sklearn).

    python tools/bench_similarity.py [--n 1000000] [--pairs-n 100000] [--reps 5] [--warmup 2] [--all-pairs] [--sklearn]
                                     [--out profiles/similarity.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VECTOR_OPS_PER_S = 256 * 4 * 16 * 2.4e9          # fp64 vector operations per second, the header's peak
OPS_PER_PAIR = {'cosine': 2, 'euclidean': 3}     # per column


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--pairs-n', type=int, default=100_000)
    ap.add_argument('--queries', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--all-pairs', action='store_true', help='also time all pairs at --n rows')
    ap.add_argument('--sklearn', action='store_true', help='also time sklearn on the host')
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args()

    import torch
    from graphrole_amd import kernels as K, synth
    from graphrole_amd.graph.csr import CSRGraph
    from graphrole_amd.measures import _adapter

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        runs = []
        for _ in range(args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            runs.append(start.elapsed_time(stop))
        return runs

    def report(what, n, nq, c, metric, segments, runs, **more):
        pairs = float(n) * nq
        rate = pairs / (min(runs) * 1e-3)
        bound = VECTOR_OPS_PER_S / (OPS_PER_PAIR[metric] * c)
        emit(dict(case=what, n=n, nq=nq, c=c, k=10, metric=metric, segments=segments,
                  ms=[round(min(runs), 3), round(max(runs), 3)], runs_ms=[round(x, 3) for x in runs],
                  pairs_per_s=float(f'{rate:.4g}'), bound_pairs_per_s=float(f'{bound:.4g}'),
                  fraction_of_bound=round(rate / bound, 3), **more))
        return rate

    rng = np.random.default_rng(0)
    n, nq = args.n, args.queries
    for c in (6, 32):
        table = rng.random((n, c))
        X = K.to_device(table)
        Q = K.to_device(np.ascontiguousarray(table[rng.choice(n, nq, replace=False)]))
        out = K.empty((nq, 10), torch.int32), K.empty((nq, 10))
        for metric in ('cosine', 'euclidean'):
            results = {}
            for segments in (1, 0):
                runs = timed(lambda: K.similar_rows(X, Q, None, k=10, metric=metric, segments=segments, out=out))
                report('queries', n, nq, c, metric, segments, runs)
                results[segments] = K.to_host(out[0]).copy(), K.to_host(out[1]).copy()
            assert results[0][0].tobytes() == results[1][0].tobytes() and results[0][1].tobytes() == results[1][1].tobytes()
            if args.sklearn:
                from sklearn.neighbors import NearestNeighbors
                nn = NearestNeighbors(n_neighbors=10, algorithm='brute', metric=metric, n_jobs=16).fit(table)
                queries = K.to_host(Q)
                host_runs = []
                for _ in range(2):
                    t0 = time.perf_counter()
                    ind = nn.kneighbors(queries, return_distance=False)
                    host_runs.append((time.perf_counter() - t0) * 1e3)
                agree = float(np.mean([len(set(a) & set(b)) / 10 for a, b in zip(ind, results[0][0])]))
                emit(dict(case='sklearn_brute_16_threads', n=n, nq=nq, c=c, k=10, metric=metric,
                          ms=[round(min(host_runs), 1), round(max(host_runs), 1)], neighbours_shared=round(agree, 4)))
        del X, Q

    # all pairs
    c = 6
    small = K.to_device(rng.random((args.pairs_n, c)))
    out = K.empty((args.pairs_n, 10), torch.int32), K.empty((args.pairs_n, 10))
    rates = {}
    for metric in ('cosine', 'euclidean'):
        runs = timed(lambda: K.similar_rows(small, None, None, k=10, metric=metric, out=out))
        rates[metric] = report('all_pairs', args.pairs_n, args.pairs_n, c, metric, 0, runs)
    del small, out
    if args.all_pairs:
        big = K.to_device(rng.random((n, c)))
        out = K.empty((n, 10), torch.int32), K.empty((n, 10))
        runs = timed(lambda: K.similar_rows(big, None, None, k=10, metric='cosine', out=out))
        report('all_pairs', n, n, c, 'cosine', 0, runs)
        del big, out
    else:
        emit(dict(case='all_pairs_EXTRAPOLATED_from_the_pair_rate_above', n=n, nq=n, c=c, k=10, metric='cosine',
                  seconds=round(float(n) * n / rates['cosine'], 2)))

    # the yardstick: grx_neighbor_roles on the BA graph of the same size
    src, dst = synth.ba_edges(n, 10, seed=0)
    csr = _adapter(CSRGraph(n, src, dst, validate=False))._device_graph()[1]
    P = K.to_device(rng.random((n, 6)))
    N = K.empty((6, n))
    runs = timed(lambda: K.neighbor_roles(csr, P, 'mean', out=N))
    emit(dict(case='grx_neighbor_roles', graph='ba_m10', n=n, arcs=csr.nnz, r=6, ms=[round(min(runs), 3), round(max(runs), 3)],
              runs_ms=[round(x, 3) for x in runs]))


if __name__ == '__main__':
    main()
