"""
Sense-making timings on one GPU: per-measure milliseconds of graphrole_amd.node_measures on synthetic graphs
(graphrole_amd/synth.py), power-iteration counts, milliseconds and bytes per iteration against the random-gather
ceiling measured for the aggregation kernel (profiles/r05_aggregation_experiments.txt: 62.4 G gathered rows/s from a
64 MB power-law table), and RoleExtractor.sense_making on an 8-role factor.  One JSON line per graph.

    python tools/bench_sense.py [--graphs ba1m,ba10m,dw5m] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GATHER_ROWS_PER_S = 62.4e9
GRAPHS = {
    'ba1m': lambda synth: synth.ba_graph(1_000_000, 10, seed=0),
    'ba10m': lambda synth: synth.ba_graph(10_000_000, 10, seed=0),
    'dw5m': lambda synth: synth.directed_weighted_graph(5_000_000, 100_000_000, seed=0),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', default='ba1m,ba10m,dw5m')
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    import torch
    from graphrole_amd import RoleExtractor, synth
    from graphrole_amd.graph.interface.csr import CSRInterface
    from graphrole_amd.measures import ConvergenceError, available_measures, measures_of

    for key in args.graphs.split(','):
        g = GRAPHS[key](synth)
        graph = CSRInterface(g)
        t0 = time.perf_counter()
        graph._device_graph()
        torch.cuda.synchronize()
        ingest_ms = (time.perf_counter() - t0) * 1e3
        host, out, tr = graph._device_graph()
        csr_in = tr if g.directed else out
        n, nnz = host.n, csr_in.nnz
        result = {'graph': key, 'n': n, 'arcs_pulled': nnz, 'weighted': bool(g.weighted), 'ingest_ms': round(ingest_ms, 2),
                  'measures': {}}
        names = available_measures(g.directed, False)
        measures_of(graph, [nm for nm in names if nm != 'eigenvector'])   # warm-up: kernels loaded, orientation cached
        runs = [(name, {}) for name in names]
        # networkx's stopping rule (L1 change < N tol) stops PageRank on a 1 M-node graph after an iteration or two:
        # a second run with a tight tolerance gives the per-iteration figures over many iterations
        runs += [(name, {'tol': 1e-15, 'max_iter': 200}) for name in ('pagerank', 'eigenvector')]
        for name, kw in runs:
            times = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                try:
                    it = measures_of(graph, [name], **kw).attrs['iterations'].get(name)
                    converged = True
                except ConvergenceError as exc:
                    it, converged = exc.iterations, False
                times.append((time.perf_counter() - t0) * 1e3)
            entry = {'ms': round(float(np.median(times)), 3)}
            if it:
                entry['converged'] = converged
                # per iteration: col (4 B) + gathered vector (8 B) [+ weight 8 B] per arc; row_ptr, x_in, x_out and the
                # per-node scaled vector / inverse out-weight (PageRank) or z (eigenvector) per node
                per_arc = 12 + (8 if csr_in.w is not None else 0)
                per_node = 8 * (5 if name == 'pagerank' else 6)
                bytes_it = nnz * per_arc + n * per_node
                ms_it = entry['ms'] / it
                entry.update({'iterations': it, 'ms_per_iteration': round(ms_it, 4), 'bytes_per_iteration': bytes_it,
                              'GB_per_s': round(bytes_it / ms_it / 1e6, 1),
                              'gather_ceiling_ms_per_iteration': round(nnz / GATHER_ROWS_PER_S * 1e3, 4)})
            result['measures'][name + ('' if not kw else '_tol1e-15')] = entry
        M = measures_of(graph, [nm for nm in names if nm != 'eigenvector'])
        rng = np.random.default_rng(0)
        roles = RoleExtractor(n_roles=8)
        roles.node_role_factor = pd.DataFrame(rng.random((n, 8)), index=M.index,
                                              columns=[f'role_{i}' for i in range(8)])
        M = M.fillna(0)
        roles.sense_making(M)
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            roles.sense_making(M)
            times.append((time.perf_counter() - t0) * 1e3)
        result['sense_making_ms'] = round(float(np.median(times)), 2)
        result['sense_making_shape'] = [n, 8, M.shape[1]]
        print(json.dumps(result), flush=True)
        del graph, g, M, roles
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
