"""
NeighborSense timings on one GPU (csrc/grx_neighbor_sense.hip), one JSON line per membership width, on the BA graph with
--n nodes and m = 10 (the BASELINE graph at 1 M, synth.ba_edges(n, 10, seed=0)).

Each line holds, for one width r (default 6 and 32), over --reps runs after --warmup warm-ups, every run timed on its own
between two device synchronisations (minimum - maximum and every run), all in the same process, the kernels run in turn
(so each follows another kernel, not an idle device) and the whole call after them:

- grx_neighbor_roles alone (mode 'mean', P and the output allocated once): without weights, with uniform weights (an
  fp64 array of ones: the same result, one more 8-byte stream per arc), and without weights at every lanes_per_row the
  entry point accepts;
- grx_aggregate on the same CSR at f = r (sums and means together, rows packed to its cache-line stride): the yardstick,
  an unweighted gather of the same rows;
- the whole RoleExtractor.neighbor_sense call (label matching, upload of P, transpose, the kernel, grx_gram, the NNLS).

Beside the times: the algorithmic bytes of the kernel -- per arc 4 (column index) + 8 r (the gathered membership row)
(+ 8 with weights), per node 16 (row pointers) + 8 r (output) -- and the bandwidth the best run reached with them.

    python tools/bench_neighbor_sense.py [--n 1000000] [--reps 5] [--warmup 2] [--widths 6,32]
                                         [--out profiles/neighbor_sense.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--widths', default='6,32')
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args()

    import pandas as pd
    import torch
    from graphrole_amd import RoleExtractor, kernels as K, synth
    from graphrole_amd.graph.csr import CSRGraph
    from graphrole_amd.measures import _adapter

    src, dst = synth.ba_edges(args.n, 10, seed=0)
    G = CSRGraph(args.n, src, dst, validate=False)
    csr = _adapter(G)._device_graph()[1]
    n, nnz = csr.n, csr.nnz
    ones = K.to_device(np.ones(nnz))
    rng = np.random.default_rng(0)

    for r in (int(x) for x in args.widths.split(',')):
        values = rng.random((n, r))
        frame = pd.DataFrame(values, columns=[f'role_{k}' for k in range(r)])
        P = K.to_device(values)
        out = K.empty((r, n))
        extractor = RoleExtractor(n_roles=max(r, 2))
        cases = {
            'grx_neighbor_roles': lambda: K.neighbor_roles(csr, P, 'mean', out=out),
            'grx_neighbor_roles_weighted': lambda: K.neighbor_roles(csr, P, 'mean', ones, out=out),
        }
        for lanes in K.neighbor_lanes(r):
            cases[f'grx_neighbor_roles_lanes{lanes}'] = (lambda L=lanes: K.neighbor_roles(csr, P, 'mean', lanes=L, out=out))
        cols = [K.to_device(np.ascontiguousarray(values[:, k])) for k in range(r)]
        rows, ldr = K.pack_rows(cols, n)
        agg_out = K.empty((2 * r, n))
        cases['grx_aggregate'] = lambda: K.aggregate(csr, rows, r, ldr, out=agg_out)
        whole = lambda: extractor.neighbor_sense(G, frame)     # mostly host work: timed apart from the kernels

        for fn in cases.values():
            for _ in range(args.warmup):
                fn()
        times = {case: [] for case in cases}
        for _ in range(args.reps):
            for case, fn in cases.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[case].append((time.perf_counter() - t0) * 1e3)
        whole()
        times['neighbor_sense'] = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            whole()
            torch.cuda.synchronize()
            times['neighbor_sense'].append((time.perf_counter() - t0) * 1e3)
        # the mean of the neighbours equals the aggregate's mean up to the summation order
        K.neighbor_roles(csr, P, 'mean', out=out)
        K.aggregate(csr, rows, r, ldr, out=agg_out)
        gap = float(np.max(np.abs(K.to_host(out) - K.to_host(agg_out)[r:])))
        assert gap < 1e-12, gap

        median = {case: float(np.median(t)) for case, t in times.items()}
        plain = nnz * (4 + 8 * r) + n * (16 + 8 * r)
        row = {'graph': 'ba_m10', 'n': n, 'arcs': nnz, 'r': r, 'max_degree': int(np.diff(csr._host[0]).max()),
               'long_rows': int(np.count_nonzero(np.diff(csr._host[0]) > K.NS_LONG_ROW)), 'aggregate_ldr': int(ldr),
               'ms': {case: [round(min(t), 3), round(max(t), 3)] for case, t in times.items()},
               'runs_ms': {case: [round(x, 3) for x in t] for case, t in times.items()},
               'algorithmic_bytes': {'unweighted': plain, 'weighted': plain + 8 * nnz},
               'tb_per_s': {'unweighted': round(plain / min(times['grx_neighbor_roles']) / 1e9, 3),
                            'weighted': round((plain + 8 * nnz) / min(times['grx_neighbor_roles_weighted']) / 1e9, 3)},
               'ratio_to_grx_aggregate': round(median['grx_neighbor_roles'] / median['grx_aggregate'], 3),
               'max_abs_gap_to_aggregate_mean': gap}
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
