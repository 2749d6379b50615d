"""
Truss-number timings on one GPU (csrc/grx_truss.hip), one JSON line per graph, all graphs with --n nodes:

- ba_m10:     the BA graph with 1 M nodes and m = 10 (the BASELINE graph, synth.ba_edges(1_000_000, 10, seed=0));
- ba_m2:      the BA graph with m = 2;
- bipartite:  the random bipartite graph of tools/bench_square_clustering.py, n / 2 nodes on either side and about 5 n
              distinct edges: no triangle, so the call is the support pass, one sweep and one round.

Each line holds the time of kernels.truss_numbers on the graph's structure CSR (--reps runs after --warmup warm-ups,
every run timed on its own between two device synchronisations; minimum - maximum and every run), the same with
want_node=False, the rounds, the levels and the edges by truss number, and in the same process, run in turn with it,
kernels.clustering without weights (the same row intersections as the support pass) and kernels.core_numbers on the
same CSR as yardsticks.  Unless --no-profile, the per-kernel split of ONE call -- support pass, peeling by kernel, node
pass -- comes from a `rocprofv3 --kernel-trace --stats` run of its own in a fresh child process (the timed runs are
never profiled).  --lanes adds the time of the call at each lane-group width (4, 8, 16, 32).  --oracle adds the
frontier and decrement counts of tests/truss_oracle.py on the same CSR (host only, more than a minute at 10 M edges;
the counts do not depend on the labelling, so they can be taken from the same edge list on any machine).

    python tools/bench_truss.py [--n 1000000] [--reps 5] [--warmup 2] [--graphs ba_m10,ba_m2,bipartite] [--no-profile]
                                [--lanes] [--oracle]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRAPHS = ('ba_m10', 'ba_m2', 'bipartite')
#: kernel-name fragment -> stage of the split
STAGES = (('tr_support', 'support'), ('tr_rows', 'support_rows'), ('tr_node', 'node'), ('tr_peel', 'peel'),
          ('pl_min', 'sweep_min'), ('pl_collect', 'sweep_collect'), ('pl_finalize', 'finalize'), ('tr_init', 'init'))


def _csr(name, n):
    """The structure CSR (internal row order) of graph `name`."""
    from graphrole_amd import synth
    from graphrole_amd.graph.csr import CSRGraph
    from graphrole_amd.measures import _adapter
    if name == 'bipartite':
        rng = np.random.default_rng(2)
        key = np.unique(rng.integers(0, n // 2, size=5 * n) * (n // 2) + rng.integers(0, n // 2, size=5 * n))
        src, dst = key // (n // 2), n // 2 + key % (n // 2)
    else:
        src, dst = synth.ba_edges(n, {'ba_m10': 10, 'ba_m2': 2}[name], seed=0)
    return _adapter(CSRGraph(n, src, dst, validate=False))._structure_csrs()[0]


def child(name, n):
    """One warm-up and one call: the process rocprofv3 traces."""
    import torch
    from graphrole_amd import kernels as K
    csr = _csr(name, n)
    K.truss_numbers(csr)
    K.truss_numbers(csr)
    torch.cuda.synchronize()


def kernel_split(name, n):
    """{stage: launches and ms per call} from a rocprofv3 run of `--child name` (two calls: halved)."""
    if shutil.which('rocprofv3') is None:
        return {'error': 'rocprofv3 not found'}
    out_dir = tempfile.mkdtemp(prefix='tr_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '--',
               sys.executable, os.path.abspath(__file__), '--child', name, '--n', str(n)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if done.returncode != 0:                                # nothing more on this GPU after a failed run
            raise RuntimeError(f'rocprofv3 exit {done.returncode}: {done.stdout[-400:]}')
        split = {}
        for path in glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True):
            for row in csv.DictReader(open(path)):
                stage = next((s for frag, s in STAGES if frag in row.get('Name', '')), None)
                if stage:
                    got = split.setdefault(stage, {'calls': 0, 'ms': 0.0})
                    got['calls'] += int(row['Calls']) // 2
                    got['ms'] = round(got['ms'] + float(row['TotalDurationNs']) / 2e6, 4)
        return split or {'error': 'no kernel_stats.csv rows'}
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--graphs', default=','.join(GRAPHS))
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--oracle', action='store_true')
    ap.add_argument('--lanes', action='store_true', help='also time the call at every lane-group width')
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.n)
        return

    import torch
    from graphrole_amd import kernels as K
    for name in args.graphs.split(','):
        csr = _csr(name, args.n)
        cases = {
            'truss_numbers': lambda: K.truss_numbers(csr),
            'truss_numbers_arcs_only': lambda: K.truss_numbers(csr, want_node=False),
            'grx_clustering': lambda: K.clustering(csr)[0],
            'grx_core_numbers': lambda: K.core_numbers(csr),
        }
        for fn in cases.values():
            for _ in range(args.warmup):
                fn()
        times = {case: [] for case in cases}
        out = {}
        for _ in range(args.reps):
            for case, fn in cases.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out[case] = fn()
                torch.cuda.synchronize()
                times[case].append((time.perf_counter() - t0) * 1e3)
        arc, node, n_rounds, n_levels = out['truss_numbers']
        values, counts = np.unique(K.to_host(arc)[:csr.nnz], return_counts=True)
        median = {case: float(np.median(t)) for case, t in times.items()}
        row = {'graph': name, 'n': csr.n, 'arcs': csr.nnz, 'lanes': csr.lanes_per_row, 'hub_rows': csr.n_hubs,
               'max_degree': int(np.diff(csr._host[0]).max()),
               'ms': {case: [round(min(t), 3), round(max(t), 3)] for case, t in times.items()},
               'runs_ms': {case: [round(x, 3) for x in t] for case, t in times.items()},
               'rounds': n_rounds, 'levels': n_levels, 'max_truss': int(values[-1]),
               'us_per_round': round(1e3 * median['truss_numbers'] / max(n_rounds, 1), 1),
               'edges_by_truss': {int(v): int(c) // 2 for v, c in zip(values, counts)},
               'max_node_truss': int(K.to_host(node)[:csr.n].max()),
               'ratio_to_grx_clustering': round(median['truss_numbers'] / median['grx_clustering'], 2),
               'ratio_to_grx_core_numbers': round(median['truss_numbers'] / median['grx_core_numbers'], 2)}
        if args.lanes:
            # the same call at every lane-group width: a peel that waits for a few long intersections scales with it
            row['ms_by_lanes'] = {}
            for lanes in (4, 8, 16, 32):
                K.truss_numbers(csr, lanes=lanes)
                t = []
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    K.truss_numbers(csr, lanes=lanes)
                    torch.cuda.synchronize()
                    t.append((time.perf_counter() - t0) * 1e3)
                row['ms_by_lanes'][lanes] = [round(min(t), 3), round(max(t), 3)]
        if args.oracle:
            from tests import truss_oracle
            want = truss_oracle.truss_numbers(K.to_host(csr.row_ptr), K.to_host(csr.col)[:csr.nnz])
            assert np.array_equal(want.arc_truss, K.to_host(arc)[:csr.nnz]) and want.n_rounds == n_rounds
            row['frontier_edges'] = csr.nnz // 2
            row['largest_frontier'] = int(want.frontier_max)
            row['decrements'] = int(want.decrements)
        if not args.no_profile:
            row['kernel_split_ms'] = kernel_split(name, args.n)
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
