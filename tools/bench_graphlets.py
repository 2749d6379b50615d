"""
Graphlet-orbit timings on one GPU (csrc/grx_graphlets.hip), one JSON line per graph, all graphs with --n nodes:

- ba_m10:     the BA graph with 1 M nodes and m = 10 (the BASELINE graph, synth.ba_edges(1_000_000, 10, seed=0));
- ba_m2:      the BA graph with m = 2;
- bipartite:  the random bipartite graph of tools/bench_square_clustering.py, n / 2 nodes on either side and about 5 n
              distinct edges: no triangle, so orbits 3 and 9-14 are zero and the 4-clique kernel skips every arc.

Each line holds the time of grx_graphlet_orbits ALONE -- its Q input (d_squares) and the orientation are computed once,
outside the timed window -- over --reps runs after --warmup warm-ups, every run timed on its own between two device
synchronisations (minimum - maximum and every run), and in the same process, run in turn with it, kernels.square_clustering
(the Q input: what kernels.graphlet_orbits adds on top of the entry point), kernels.truss_numbers and the whole
kernels.graphlet_orbits call on the same CSR.  Unless --no-profile, the per-stage split of ONE grx_graphlet_orbits call
comes from a `rocprofv3 --kernel-trace --stats` run of its own in a fresh child process (the timed runs are never
profiled).  The nine graphlet totals of the graph are recorded beside the times.

    python tools/bench_graphlets.py [--n 1000000] [--reps 5] [--warmup 2] [--graphs ba_m10,ba_m2,bipartite] [--no-profile]
                                    [--out profiles/graphlets.txt]
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
#: kernel-name fragment -> stage of the split (the first match counts)
STAGES = (('gl_stats', 'row_statistics'), ('gl_support', 'arc_support'), ('gl_mirror', 'arc_support_mirror'),
          ('gl_pass_a', 'row_pass_a'), ('gl_pass_b', 'row_pass_b'), ('gl_diamond', 'arc_diamond'),
          ('gl_k4', 'four_cliques'), ('gl_finish', 'finish'), ('sq_count', 'q_input_count'), ('sq_rows', 'q_input_rows'))
NAMES = ('edge', 'path3', 'triangle', 'path4', 'star4', 'cycle4', 'paw', 'diamond', 'clique4')


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


class EntryPoint:
    """grx_graphlet_orbits with everything else prepared once: Q, the orientation, the workspace, the outputs."""

    def __init__(self, csr):
        import torch
        from graphrole_amd import kernels as K
        self.K, self.csr = K, csr
        self.squares = K.square_clustering(csr, want_counts=True)[1]
        self.o = csr.oriented()
        self.ws, self.ws_bytes = K._workspace('grx_graphlet_orbits_workspace_bytes', csr.n, csr.nnz)
        self.orbits = torch.empty((15, csr.n), dtype=torch.int64, device=K.device())
        self.hubs = K._hubs_for(csr, None)

    def __call__(self):
        from graphrole_amd import _lib
        K, csr = self.K, self.csr
        hub_ptr, n_hubs, lanes, _keep = self.hubs
        _lib.call('grx_graphlet_orbits', csr.n, K._ptr(csr.row_ptr), K._ptr(csr.col), K._ptr(self.o.row_ptr),
                  K._ptr(self.o.col), hub_ptr, n_hubs, lanes, K._ptr(self.squares), K._ptr(self.orbits), None, None,
                  K._ptr(self.ws), self.ws_bytes, K._stream())
        return self.orbits


def child(name, n):
    """One warm-up and one call of the entry point, and one of its Q input: the process rocprofv3 traces."""
    import torch
    from graphrole_amd import kernels as K
    csr = _csr(name, n)
    call = EntryPoint(csr)                                      # the first square_clustering call
    call()
    call()
    K.square_clustering(csr, want_counts=True)                  # the second
    torch.cuda.synchronize()


def kernel_split(name, n):
    """{stage: launches and ms per call} from a rocprofv3 run of `--child name` (two calls of each: halved)."""
    if shutil.which('rocprofv3') is None:
        return {'error': 'rocprofv3 not found'}
    out_dir = tempfile.mkdtemp(prefix='gl_prof_')
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
        entry = EntryPoint(csr)
        cases = {
            'grx_graphlet_orbits': entry,
            'grx_square_clustering': lambda: K.square_clustering(csr, want_counts=True)[1],
            'grx_truss_numbers': lambda: K.truss_numbers(csr),
            'graphlet_orbits_with_q': lambda: K.graphlet_orbits(csr)[0],
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
        orbits = K.to_host(out['grx_graphlet_orbits'])
        assert orbits.tobytes() == K.to_host(out['graphlet_orbits_with_q']).tobytes()
        s = orbits.sum(axis=1)
        totals = dict(zip(NAMES, (int(x) for x in (s[0] // 2, s[2], s[3] // 3, s[4] // 2, s[7], s[8] // 4, s[9],
                                                   s[13] // 2, s[14] // 4))))
        median = {case: float(np.median(t)) for case, t in times.items()}
        row = {'graph': name, 'n': csr.n, 'arcs': csr.nnz, 'lanes': csr.lanes_per_row, 'hub_rows': csr.n_hubs,
               'max_degree': int(np.diff(csr._host[0]).max()),
               'max_out_degree': int(np.diff(entry.o._host[0]).max()),
               'ms': {case: [round(min(t), 3), round(max(t), 3)] for case, t in times.items()},
               'runs_ms': {case: [round(x, 3) for x in t] for case, t in times.items()},
               'graphlets': totals,
               'ratio_to_grx_square_clustering': round(median['grx_graphlet_orbits'] / median['grx_square_clustering'], 3),
               'ratio_to_grx_truss_numbers': round(median['grx_graphlet_orbits'] / median['grx_truss_numbers'], 3)}
        if not args.no_profile:
            row['kernel_split_ms'] = kernel_split(name, args.n)
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
