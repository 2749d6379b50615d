"""
Betweenness centrality over shortest paths by weight on one GPU (grx_weighted_betweenness in
csrc/grx_weighted_betweenness.hip), one JSON line:

BA 1 M nodes, m = 10 (the edges of the BASELINE graph, synth.ba_edges(1_000_000, 10, 0)) with --weights uniform
(seeded floats in [0.05, 1): lightest paths hardly ever tie) or ints (seeded integers 1..5: many ties) and --sources
random sources.  For every --batch value: each run timed on its own between two device synchronisations after --warmup
warm-ups, all --reps runs listed with their median and spread, the relaxation rounds and the deepest DAG level, and
whether the bc bytes equal those of the first width.  With --split one more run per width under the library's event
profiler gives the relaxation / forward / backward shares (events around every round: that run is slower and is not
one of the timed ones).  For scale, the same sources through kernels.betweenness (unweighted Brandes on the same CSR,
the weights not read) and through kernels.weighted_distances (the relaxation alone, with its per-target sums).
--check sources are compared with networkx on a 2 000-node BA graph with the same kind of weights (networkx needs
minutes per source at 1 M nodes).

    python tools/bench_weighted_betweenness.py [--n 1000000] [--m 10] [--weights uniform] [--sources 1024]
                                               [--batch 0,32,16] [--reps 3] [--warmup 1] [--split] [--check 8]

Run one process per (weights, sources) pair, each under a time limit of its own.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPLIT = {'relaxation': 'wbc relaxation: sp_round_kernel (+hub)', 'forward': 'wb_forward_kernel (+hub)',
         'backward': 'wb_backward_kernel (+hub)'}


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


def _weights(kind, count, seed=1):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.05, 1.0, size=count) if kind == 'uniform' else rng.integers(1, 6, size=count).astype(np.float64)


def _split(fn):
    """{'relaxation' | 'forward' | 'backward': (ms, launches)} of one run under the event profiler."""
    import torch
    from graphrole_amd import _lib
    lib = _lib.load()
    ids = {lib.grx_profile_kernel_name(i).decode(): i for i in range(lib.grx_profile_kernel_count())}
    lib.grx_profile_reset()
    lib.grx_profile_select(sum(1 << ids[name] for name in SPLIT.values()))
    lib.grx_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    out = {}
    for key, name in SPLIT.items():
        ms, launches = ctypes.c_double(0), ctypes.c_longlong(0)
        lib.grx_profile_read(ids[name], ctypes.byref(ms), ctypes.byref(launches))
        out[key] = {'ms': round(ms.value, 2), 'scopes': launches.value}
    lib.grx_profile_enable(0)
    lib.grx_profile_select(0)
    total = sum(v['ms'] for v in out.values()) or 1.0
    for v in out.values():
        v['share'] = round(v['ms'] / total, 3)
    return out


def _check(kind, count):
    """`count` sampled sources on a 2 000-node BA graph against networkx, relative error of the worst node."""
    import networkx as nx
    from graphrole_amd import weighted_betweenness_centrality
    G = nx.barabasi_albert_graph(2000, 5, seed=4)
    for (u, v), w in zip(G.edges(), _weights(kind, G.number_of_edges(), seed=2)):
        G[u][v]['weight'] = float(w)
    got = weighted_betweenness_centrality(G, k=count, seed=5)
    want = nx.betweenness_centrality(G, k=count, seed=5, weight='weight')
    want = np.array([want[v] for v in got.index])
    err = np.abs(got.to_numpy() - want) / np.where(want > 0, want, 1.0)
    return {'sources': count, 'max_rel_err': float(err.max()),
            'exact_zeros_kept': bool(np.array_equal(got.to_numpy() == 0, want == 0)), 'levels': got.attrs['levels']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--m', type=int, default=10)
    ap.add_argument('--weights', default='uniform', choices=('uniform', 'ints'))
    ap.add_argument('--sources', type=int, default=1024)
    ap.add_argument('--batch', default='0', help='comma-separated sources per batch (16, 32, 64; 0 = the library\'s choice)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--split', action='store_true', help='one more run per width under the event profiler')
    ap.add_argument('--check', type=int, default=8, help='sampled sources compared with networkx on a small graph')
    ap.add_argument('--label', default='', help='copied into the result line')
    args = ap.parse_args()

    from graphrole_amd import kernels as K, measures, synth
    from graphrole_amd.graph.csr import CSRGraph
    src, dst = synth.ba_edges(args.n, args.m, 0)
    graph = measures._adapter(CSRGraph(args.n, src, dst, _weights(args.weights, len(src)), validate=False))
    host, out, _ = graph._device_graph()
    sources = np.asarray(host.inv)[np.random.default_rng(0).choice(host.n, size=args.sources, replace=False)]
    row = {'label': args.label, 'n': host.n, 'arcs': out.nnz, 'hub_rows': out.n_hubs, 'weights': args.weights,
           'sources': args.sources, 'weighted_betweenness': {}}
    first = None
    for batch in [int(b) for b in args.batch.split(',') if b != '']:
        fn = lambda: K.weighted_betweenness(out, None, sources, False, 1.0, batch)         # noqa: E731
        for _ in range(args.warmup):
            fn()
        times, (bc, rounds, levels) = _timed(fn, args.reps)
        S = batch or (16 if args.sources <= 16 else 32 if args.sources <= 32 else 64)
        bits = K.to_host(bc)[:host.n].tobytes()
        first = first or bits
        entry = dict(_summary(times), lanes=S, batches=-(-args.sources // S), relaxation_rounds=rounds,
                     deepest_level=levels, state_bytes=host.n * (28 * S + 4),
                     ms_per_source=round(float(np.median(times)) / args.sources, 3), same_bits_as_first=bits == first,
                     largest_bc=float(K.to_host(bc)[:host.n].max()))
        if args.split:
            entry['split'] = _split(fn)
        row['weighted_betweenness'][f'batch={batch}'] = entry
    K.betweenness(out, None, sources, False, 1.0)
    times, _ = _timed(lambda: K.betweenness(out, None, sources, False, 1.0), args.reps)
    row['unweighted_betweenness'] = _summary(times)
    K.weighted_distances(out, sources)
    times, result = _timed(lambda: K.weighted_distances(out, sources), args.reps)
    row['weighted_distances'] = dict(_summary(times), rounds=result[6])
    if args.check:
        row['networkx_check'] = _check(args.weights, args.check)
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
