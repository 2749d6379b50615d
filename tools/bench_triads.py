"""
Triad-census timings on one GPU (csrc/grx_triads.hip), one JSON line per graph, all graphs with --n nodes:

- ba_m10:  the BA graph with 1 M nodes and m = 10 (synth.ba_edges(1_000_000, 10, seed=0)) on a seeded random
           orientation, a fifth of its edges made mutual;
- ba_m2:   the same with m = 2;
- gnm:     a directed G(n, m) with m = 2 n distinct arcs drawn at random (few mutual pairs, few triangles).

Each line holds the time of grx_triad_census ALONE -- the CSR, the codes, the workspace and the outputs are prepared
once, outside the timed window -- with the totals and without, over --reps runs after --warmup warm-ups, every run timed
on its own between two device synchronisations (minimum - maximum and every run), and in the same process, run in turn
with it, grx_clustering on the same directed CSR (Fagiolo's coefficient: one intersection per arc slot where the census
runs one per pair): the yardstick.  Unless --no-profile, the per-kernel split of ONE grx_triad_census call comes from a
`rocprofv3 --kernel-trace --stats` run of its own in a fresh child process (the timed runs are never profiled).  The
census of the graph is recorded beside the times.

    python tools/bench_triads.py [--n 1000000] [--reps 5] [--warmup 2] [--graphs ba_m10,ba_m2,gnm] [--no-profile]
                                 [--out profiles/triads.txt]
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

GRAPHS = ('ba_m10', 'ba_m2', 'gnm')
#: kernel-name fragments (all must occur) -> stage of the split (the first match counts)
STAGES = ((('hub_rows', 'td_stats'), 'row_classes_hubs'), (('td_stats',), 'row_classes'),
          (('td_arc',), 'arc_intersections'),
          (('hub_rows', 'td_sums'), 'row_sums_and_finish_hubs'), (('td_sums',), 'row_sums_and_finish'),
          (('td_pairs',), 'pair_count'), (('td_totals',), 'totals'), (('td_third',), 'totals'),
          (('grx_fill',), 'zero_fill'))


def _arcs(name, n):
    """(src, dst) of the distinct arcs of graph `name`, no self-loops."""
    from graphrole_amd import synth
    rng = np.random.default_rng(5)
    if name == 'gnm':
        a, b = rng.integers(0, n, size=2 * n), rng.integers(0, n, size=2 * n)
        key = np.unique(a[a != b] * np.int64(n) + b[a != b])
        return key // n, key % n
    u, v = synth.ba_edges(n, {'ba_m10': 10, 'ba_m2': 2}[name], seed=0)
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    kind = rng.random(len(u))                                   # < 0.2: both arcs; else one, in a random direction
    fwd, bwd = kind < 0.6, (kind < 0.2) | (kind >= 0.6)
    return np.concatenate([u[fwd], v[bwd]]), np.concatenate([v[fwd], u[bwd]])


def _inputs(name, n):
    """(device CSR, codes, fwd, bwd): the all-neighbours CSR in internal row order, the direction code of every slot
    and the same directions as grx_clustering reads them (1 for a present direction, -1 for an absent one)."""
    from graphrole_amd import kernels as K
    from graphrole_amd.graph.csr import CSRGraph
    from graphrole_amd.measures import _adapter, _triad_csr
    src, dst = _arcs(name, n)
    csr, codes, (_, _, host_codes) = _triad_csr(_adapter(CSRGraph(n, src, dst, directed=True, validate=False)), K)
    fwd = K.to_device(np.where(host_codes & 1, 1.0, -1.0))
    bwd = K.to_device(np.where(host_codes & 2, 1.0, -1.0))
    return csr, codes, fwd, bwd


class EntryPoint:
    """grx_triad_census with everything else prepared once: the workspace and the outputs."""

    def __init__(self, csr, codes, want_totals):
        import torch
        from graphrole_amd import kernels as K
        self.K, self.csr, self.codes = K, csr, codes
        self.ws, self.ws_bytes = K._workspace('grx_triad_census_workspace_bytes', csr.n, csr.nnz)
        self.census = torch.empty((16, csr.n), dtype=torch.int64, device=K.device())
        self.totals = torch.empty(16, dtype=torch.int64, device=K.device()) if want_totals else None
        self.hubs = K._hubs_for(csr, None)

    def __call__(self):
        from graphrole_amd import _lib
        K, csr = self.K, self.csr
        hub_ptr, n_hubs, lanes, _keep = self.hubs
        _lib.call('grx_triad_census', csr.n, K._ptr(csr.row_ptr), K._ptr(csr.col), K._ptr(self.codes), hub_ptr, n_hubs,
                  lanes, K._ptr(self.census), K._ptr(self.totals), None, K._ptr(self.ws), self.ws_bytes, K._stream())
        return self.census


def child(name, n):
    """One warm-up and one call of the entry point: the process rocprofv3 traces."""
    import torch
    csr, codes, _, _ = _inputs(name, n)
    call = EntryPoint(csr, codes, True)
    call()
    call()
    torch.cuda.synchronize()


def kernel_split(name, n):
    """{stage: launches and ms per call} from a rocprofv3 run of `--child name` (two calls: halved)."""
    if shutil.which('rocprofv3') is None:
        return {'error': 'rocprofv3 not found'}
    out_dir = tempfile.mkdtemp(prefix='td_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '--',
               sys.executable, os.path.abspath(__file__), '--child', name, '--n', str(n)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if done.returncode != 0:                                # nothing more on this GPU after a failed run
            raise RuntimeError(f'rocprofv3 exit {done.returncode}: {done.stdout[-400:]}')
        split = {}
        for path in glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True):
            for row in csv.DictReader(open(path)):
                kernel = row.get('Name', '')
                stage = next((s for frags, s in STAGES if all(f in kernel for f in frags)), None)
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
    from graphrole_amd.measures import TRIAD_NAMES
    for name in args.graphs.split(','):
        csr, codes, fwd, bwd = _inputs(name, args.n)
        entry = EntryPoint(csr, codes, True)
        cases = {
            'grx_triad_census': entry,
            'grx_triad_census_no_totals': EntryPoint(csr, codes, False),
            'grx_clustering': lambda: K.clustering(csr, fwd, bwd, 1.0)[0],
        }
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
        totals = [int(x) for x in K.to_host(entry.totals)]
        assert sum(totals) == csr.n * (csr.n - 1) * (csr.n - 2) // 6
        median = {case: float(np.median(t)) for case, t in times.items()}
        row = {'graph': name, 'n': csr.n, 'arc_slots': csr.nnz, 'lanes': csr.lanes_per_row, 'hub_rows': csr.n_hubs,
               'max_degree': int(np.diff(csr._host[0]).max()),
               'ms': {case: [round(min(t), 3), round(max(t), 3)] for case, t in times.items()},
               'runs_ms': {case: [round(x, 3) for x in t] for case, t in times.items()},
               'census': dict(zip(TRIAD_NAMES, totals)),
               'ratio_to_grx_clustering': round(median['grx_triad_census'] / median['grx_clustering'], 3)}
        if not args.no_profile:
            row['kernel_split_ms'] = kernel_split(name, args.n)
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
