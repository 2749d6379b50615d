"""
Core-number / onion-layer timings on one GPU (csrc/grx_kcore.hip), one JSON line per case:

- ba1m_m10: BA 1 M nodes, m = 10 (the BASELINE graph, synth.ba_graph(1_000_000, 10, seed=0));
- ba1m_m1:  BA 1 M nodes, m = 1 (a tree: one shell, many layers);
- gnm1m:    G(n, m) with 1 M nodes and 1.2 M edges (isolated nodes, small shells).

Each line holds the time of kernels.core_numbers on the graph's structure CSR (median of --reps runs after --warmup
warm-ups, every run timed on its own between two device synchronisations), the round count and the distinct core
values, for scale the time of one kernels.distance_sums call with 64 sources (W = 1: one bitset BFS pass) on the same
CSR, and -- unless --no-profile -- the per-kernel split of ONE call from a `rocprofv3 --kernel-trace --stats` run of its
own in a fresh child process (the timed runs are never profiled).

    python tools/bench_kcore.py [--cases ba1m_m10,ba1m_m1,gnm1m] [--reps 5] [--warmup 2] [--no-profile]
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

CASES = {
    'ba1m_m10': lambda synth: synth.ba_graph(1_000_000, 10, seed=0),
    'ba1m_m1': lambda synth: synth.ba_graph(1_000_000, 1, seed=0),
    'gnm1m': lambda synth: synth.er_graph(1_000_000, 1_200_000, seed=0),
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


def _structure(case):
    from graphrole_amd import synth
    from graphrole_amd.measures import _adapter
    graph = _adapter(CASES[case](synth))
    host = graph._device_graph()[0]
    return graph, host, graph._structure_csrs()[0]


def child(case):
    """One warm-up and one call: the process rocprofv3 traces."""
    import torch
    from graphrole_amd import kernels as K
    _, _, s_out = _structure(case)
    K.core_numbers(s_out)
    K.core_numbers(s_out)
    torch.cuda.synchronize()


def kernel_split(case):
    """{kernel: launches and ms per call} of the kc_* kernels and the pl_* ones of grx_peel.h from a rocprofv3 run of
    `--child case` (two calls: halved)."""
    if shutil.which('rocprofv3') is None:
        return {'error': 'rocprofv3 not found'}
    out_dir = tempfile.mkdtemp(prefix='kc_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '--',
               sys.executable, os.path.abspath(__file__), '--child', case]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if done.returncode != 0:
            return {'error': f'rocprofv3 exit {done.returncode}', 'tail': done.stdout[-400:]}
        split = {}
        for path in glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get('Name', '')
                prefix = next((p for p in ('kc_', 'pl_') if p in name), None)
                if prefix is None:
                    continue
                key = name[name.index(prefix):].split('(')[0].split('<')[0]
                split[key] = {'calls': int(row['Calls']) // 2,
                              'ms': round(float(row['TotalDurationNs']) / 2e6, 4)}
        return dict(sorted(split.items(), key=lambda kv: -kv[1]['ms'])) or {'error': 'no kernel_stats.csv rows'}
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def run_case(case, reps, warmup, profile):
    from graphrole_amd import kernels as K
    _, host, s_out = _structure(case)
    for _ in range(warmup):
        K.core_numbers(s_out)
    times, (core, onion, n_rounds) = _timed(lambda: K.core_numbers(s_out), reps)
    core_only, _ = _timed(lambda: K.core_numbers(s_out, want_onion=False), reps)
    core = K.to_host(core)[:host.n]
    sources = np.asarray(host.inv)[np.random.default_rng(0).choice(host.n, size=64, replace=False)]
    K.distance_sums(s_out, sources, words=1)
    bfs_times, _ = _timed(lambda: K.distance_sums(s_out, sources, words=1), reps)
    ms, bfs_ms = float(np.median(times)), float(np.median(bfs_times))
    values, counts = np.unique(core, return_counts=True)
    row = {'case': case, 'n': host.n, 'arcs': s_out.nnz, 'hub_rows': s_out.n_hubs,
           'core_numbers_ms': round(ms, 3), 'runs_ms': [round(t, 3) for t in times],
           'core_only_ms': round(float(np.median(core_only)), 3),
           'rounds': n_rounds, 'us_per_round': round(1e3 * ms / max(n_rounds, 1), 1),
           'bfs_pass_64_sources_ms': round(bfs_ms, 3), 'bfs_passes': round(ms / bfs_ms, 1),
           'distinct_cores': len(values), 'max_core': int(values[-1]),
           'shells': {int(v): int(c) for v, c in zip(values[-4:], counts[-4:])}}
    if profile:
        row['kernel_split_ms'] = kernel_split(case)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='ba1m_m10,ba1m_m1,gnm1m')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child)
        return
    for case in args.cases.split(','):
        print(json.dumps(run_case(case, args.reps, args.warmup, not args.no_profile)), flush=True)


if __name__ == '__main__':
    main()
