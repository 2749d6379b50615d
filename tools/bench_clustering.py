"""
Weighted / directed clustering timings on one GPU (csrc/grx_clustering.hip), one JSON line per case, all in one process
on the BA graph with 1 M nodes and m = 10 (the BASELINE graph, synth.ba_edges(1_000_000, 10, seed=0)):

- unweighted:                kernels.clustering with no value array (every s = 1);
- uniform_weights:           the same edges with uniform (0, 1] weights;
- directed:                  the same edges as arcs from the newer node to the older one (no reciprocal pair): the
                             same all-neighbours CSR with both value arrays, weight=None;
- structural_holes:          kernels.structural_holes (the constraint column, no weights) on the same CSR -- the kernel
                             whose per-arc stage does the same row intersections with two gathers per hit: the yardstick;
- structural_holes_weights:  the yardstick with the uniform weights, for the two cases that read value arrays;
- triangle_counts:           kernels.triangle_counts + kernels.local_structure on the same CSR -- the path the
                             undirected graph without weights keeps.

After --warmup warm-ups of every case, --reps rounds run every case once each, in turn (so that a drift of the clocks
meets all of them alike), every run timed on its own between two device synchronisations; reported as a min - max range
with the single runs and the ratio of the medians to the yardstick's.  Unless --no-profile, the per-kernel split of ONE
call of the cases that read value arrays comes from a `rocprofv3 --kernel-trace --stats` run of its own in a fresh child
process each (the timed runs are never profiled).

    python tools/bench_clustering.py [--n 1000000] [--m 10] [--reps 5] [--warmup 2] [--no-profile] [--out FILE]
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROFILED = ('uniform_weights', 'directed', 'structural_holes_weights')


def _cases(n, m):
    """({case: callable returning the device column}, the undirected CSR, host seconds of the directed CSR)."""
    from graphrole_amd import kernels as K
    from graphrole_amd import synth
    from graphrole_amd.graph.csr import CSRGraph
    from graphrole_amd.measures import _adapter, _directional_csr, _max_weight

    src, dst = synth.ba_edges(n, m, seed=0)
    w = 1.0 - np.random.default_rng(1).random(len(src))         # (0, 1]
    weighted = _adapter(CSRGraph(n, src, dst, weights=w, validate=False))
    csr = weighted._device_graph()[1]
    max_weight = _max_weight(weighted, True)
    directed = _adapter(CSRGraph(n, src, dst, directed=True, validate=False))
    t0 = time.perf_counter()
    dcsr, fwd, bwd = _directional_csr(directed, K, False)
    build_s = time.perf_counter() - t0
    assert dcsr.nnz == csr.nnz
    cases = {
        'unweighted': lambda: K.clustering(csr)[0],
        'uniform_weights': lambda: K.clustering(csr, csr.w, None, max_weight)[0],
        'directed': lambda: K.clustering(dcsr, fwd, bwd, 1.0)[0],
        'structural_holes': lambda: K.structural_holes(csr)[0],
        'structural_holes_weights': lambda: K.structural_holes(csr, csr.w)[0],
        'triangle_counts': lambda: K.local_structure(csr, K.triangle_counts(csr), False)[0],
    }
    return cases, csr, build_s


def child(case, n, m):
    """One warm-up and one call: the process rocprofv3 traces."""
    import torch
    fn = _cases(n, m)[0][case]
    fn()
    fn()
    torch.cuda.synchronize()


def kernel_split(case, n, m):
    """{body<lanes> or body_hub: launches and ms per call} of the grx_rowjoin.h kernels, by their cl_* / sh_* bodies, from
    a rocprofv3 run of `--child case` (two calls: halved)."""
    if shutil.which('rocprofv3') is None:
        return {'error': 'rocprofv3 not found'}
    out_dir = tempfile.mkdtemp(prefix='cl_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '--',
               sys.executable, os.path.abspath(__file__), '--child', case, '--n', str(n), '--m', str(m)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if done.returncode != 0:                                # nothing more on this GPU after a failed run
            raise RuntimeError(f'rocprofv3 exit {done.returncode}: {done.stdout[-400:]}')
        split = {}
        for path in glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True):
            for row in csv.DictReader(open(path)):
                found = re.search(r'(rj_\w+)<(?:(\d+), )?.*?((?:cl|sh)_\w+)>', row.get('Name', ''))
                if found is None:
                    continue
                key = '%s<%s>' % (found.group(3), found.group(2)) if found.group(2) else found.group(3) + '_hub'
                split[key] = {'calls': int(row['Calls']) // 2, 'ms': round(float(row['TotalDurationNs']) / 2e6, 4)}
        return dict(sorted(split.items(), key=lambda kv: -kv[1]['ms'])) or {'error': 'no kernel_stats.csv rows'}
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--m', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.n, args.m)
        return

    import torch
    from graphrole_amd import kernels as K
    cases, csr, build_s = _cases(args.n, args.m)
    for fn in cases.values():
        for _ in range(args.warmup):
            fn()
    times = {name: [] for name in cases}
    out = {}
    for _ in range(args.reps):
        for name, fn in cases.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[name] = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    median = {name: float(np.median(t)) for name, t in times.items()}
    for name, t in times.items():
        yardstick = 'structural_holes_weights' if name in PROFILED else 'structural_holes'
        row = {'case': name, 'n': csr.n, 'arcs': csr.nnz, 'lanes': csr.lanes_per_row, 'hub_rows': csr.n_hubs,
               'ms': [round(min(t), 3), round(max(t), 3)], 'runs_ms': [round(x, 3) for x in t],
               'median_ms': round(median[name], 3), 'mean_of_column': float(np.mean(K.to_host(out[name])[:csr.n])),
               'ratio_to_structural_holes': round(median[name] / median['structural_holes'], 3),
               'ratio_to_its_yardstick': [yardstick, round(median[name] / median[yardstick], 3)]}
        if name == 'directed':
            row['directional_csr_build_s'] = round(build_s, 3)
        if name in PROFILED and not args.no_profile:
            row['kernel_split_ms'] = kernel_split(name, args.n, args.m)
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
