"""
Eccentricity timings on one GPU (grx_eccentricity in csrc/grx_closeness.hip), one JSON line per case:

- ba1m_m10: BA 1 M nodes, m = 10 (the BASELINE graph, synth.ba_graph(1_000_000, 10, seed=0));
- ba1m_m2:  BA 1 M nodes, m = 2 (sparser, deeper);
- cycle20k: the cycle on 20 000 nodes -- vertex-transitive, the worst case of the bounds method: nothing is ever
  pruned, every node becomes a source and every batch pays both passes.

Each line holds the time of graphrole_amd.measures' eccentricity column by method='bounds' (for every --words value: the
64-bit source words of one round) and by method='all' on the graph's structure CSR -- every run timed on its own between
two device synchronisations after --warmup warm-ups, all --reps runs listed with their median and spread -- the rounds
and sources the bounds method used, whether the two methods agree, the diameter and radius, and for scale the time of
one kernels.distance_sums call with 64 sources (W = 1: one bitset BFS pass) on the same CSR.

    python tools/bench_eccentricity.py [--cases ba1m_m10] [--words 0,4,1] [--reps 5] [--warmup 1] [--all-reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _cycle(n):
    from graphrole_amd.graph.csr import CSRGraph
    src = np.arange(n, dtype=np.int64)
    return CSRGraph(n, src, (src + 1) % n)


CASES = {
    'ba1m_m10': lambda synth: synth.ba_graph(1_000_000, 10, seed=0),
    'ba1m_m2': lambda synth: synth.ba_graph(1_000_000, 2, seed=0),
    'cycle20k': lambda synth: _cycle(20_000),
}


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


def run_case(case, words_list, reps, all_reps, warmup):
    from graphrole_amd import kernels as K, measures, synth
    graph = measures._adapter(CASES[case](synth))
    host = graph._device_graph()[0]
    s_out = graph._structure_csrs()[0]
    row = {'case': case, 'n': host.n, 'arcs': s_out.nnz, 'hub_rows': s_out.n_hubs, 'bounds': {}}
    reference = None
    for words in words_list:
        fn = lambda: measures._eccentricity_column(graph, K, 'bounds', words)      # noqa: E731
        for _ in range(warmup):
            fn()
        times, (col, info) = _timed(fn, reps)
        ecc = K.to_host(col)[:host.n].astype(np.int64)
        reference = ecc if reference is None else reference
        row['bounds'][f'words={words}'] = dict(_summary(times), rounds=info['rounds'], sources=info['sources'],
                                               sources_per_round=64 * (words or measures._ECC_BOUNDS_WORDS),
                                               same_as_first=bool(np.array_equal(ecc, reference)))
    fn = lambda: measures._eccentricity_column(graph, K, 'all', 0)                  # noqa: E731
    for _ in range(min(warmup, 1)):
        fn()
    times, (col, _) = _timed(fn, all_reps)
    ecc = K.to_host(col)[:host.n].astype(np.int64)
    row['all'] = dict(_summary(times), same_as_bounds=bool(reference is None or np.array_equal(ecc, reference)))
    best = min(v['median_ms'] for v in row['bounds'].values()) if row['bounds'] else None
    row['all_over_best_bounds'] = None if not best else round(row['all']['median_ms'] / best, 2)
    row['diameter'], row['radius'] = int(ecc.max()), int(ecc.min())
    values, counts = np.unique(ecc, return_counts=True)
    row['distribution'] = {int(v): int(c) for v, c in zip(values, counts)} if len(values) <= 16 else len(values)
    sources = np.asarray(host.inv)[np.random.default_rng(0).choice(host.n, size=64, replace=False)]
    K.distance_sums(s_out, sources, words=1)
    bfs_times, _ = _timed(lambda: K.distance_sums(s_out, sources, words=1), reps)
    row['bfs_pass_64_sources_ms'] = round(float(np.median(bfs_times)), 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='ba1m_m10')
    ap.add_argument('--words', default='0', help='comma-separated source words per round of the bounds method '
                                                 '(0 = the default of graphrole_amd.eccentricity)')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--all-reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    args = ap.parse_args()
    words = [int(w) for w in args.words.split(',') if w != '']
    for case in args.cases.split(','):
        print(json.dumps(run_case(case, words, args.reps, args.all_reps, args.warmup)), flush=True)


if __name__ == '__main__':
    main()
