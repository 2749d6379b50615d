"""
Square-clustering timings on one GPU (csrc/grx_square_clustering.hip), one JSON line per graph, all in one process:

- ba_m10:     the BA graph with 1 M nodes and m = 10 (the BASELINE graph, synth.ba_edges(1_000_000, 10, seed=0));
- ba_m2:      the BA graph with 1 M nodes and m = 2;
- bipartite:  a random bipartite graph, n / 2 nodes on either side and 5 n distinct edges between uniformly drawn
              pairs (triangle clustering is 0 there by construction).

On every graph three cases are timed in the same run: kernels.square_clustering, and as yardsticks kernels.clustering
(grx_clustering, no weights) and kernels.triangle_counts + kernels.local_structure (the 'clustering' column of
node_measures) on the same CSR.  After --warmup warm-ups of every case, --reps rounds run every case once each, in
turn, every run timed on its own between two device synchronisations; reported as a min - max range with the single
runs and the ratio of the medians.  Wedges are sum_u k_u^2 (one gathered 4-byte column id and one atomic each; the
rows of the dense tier gather theirs twice, which gathered_GBps counts).  Unless --no-profile, the split of ONE call
over the three tier launches comes from a `rocprofv3 --kernel-trace --stats` run of its own in a fresh child process
(the timed runs are never profiled).

    python tools/bench_square_clustering.py [--n 1000000] [--reps 5] [--warmup 2] [--graphs ba_m10,ba_m2,bipartite]
                                            [--no-profile] [--out FILE]
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

GRAPHS = ('ba_m10', 'ba_m2', 'bipartite')
TIERS = {'64': 'wave_table', '256': 'lds_table', '1024': 'dense'}


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


def _cases(csr):
    from graphrole_amd import kernels as K
    return {
        'square_clustering': lambda: K.square_clustering(csr)[0],
        'grx_clustering': lambda: K.clustering(csr)[0],
        'triangle_counts': lambda: K.local_structure(csr, K.triangle_counts(csr), False)[0],
    }


def child(name, n):
    """One warm-up and one call: the process rocprofv3 traces."""
    import torch
    fn = _cases(_csr(name, n))['square_clustering']
    fn()
    fn()
    torch.cuda.synchronize()


def tier_split(name, n):
    """{tier: ms per call} of the three sq_count_kernel launches and the row-statistics launches, from a rocprofv3 run
    of `--child name` (two calls: halved)."""
    if shutil.which('rocprofv3') is None:
        return {'error': 'rocprofv3 not found'}
    out_dir = tempfile.mkdtemp(prefix='sq_prof_')
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
                found = re.search(r'sq_count_kernel<(\d+)', kernel)
                key = TIERS[found.group(1)] if found else 'row_statistics' if 'sq_rows' in kernel else None
                if key:
                    split[key] = round(split.get(key, 0.0) + float(row['TotalDurationNs']) / 2e6, 4)
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
        row_ptr = K.to_host(csr.row_ptr).astype(np.int64)
        k = np.diff(row_ptr)
        prefix = np.concatenate([[0], np.cumsum(k[K.to_host(csr.col)[:csr.nnz]])])
        per_row = prefix[row_ptr[1:]] - prefix[row_ptr[:-1]]     # the wedges of every row: what the tiers are cut by
        tiers = {'wave_table': per_row <= K.SQ_WAVE_MAX_WEDGES, 'dense': per_row > K.SQ_LDS_MAX_WEDGES}
        tiers['lds_table'] = ~tiers['wave_table'] & ~tiers['dense']
        wedges = int(per_row.sum())
        gathered = wedges + int(per_row[tiers['dense']].sum())
        cases = _cases(csr)
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
        median = {case: float(np.median(t)) for case, t in times.items()}
        sq = median['square_clustering']
        row = {'graph': name, 'n': csr.n, 'arcs': csr.nnz, 'lanes': csr.lanes_per_row, 'hub_rows': csr.n_hubs,
               'max_degree': int(k.max()), 'wedges': wedges, 'max_row_wedges': int(per_row.max()),
               'rows': {tier: int(mask.sum()) for tier, mask in tiers.items()},
               'wedges_by_tier': {tier: int(per_row[mask].sum()) for tier, mask in tiers.items()},
               'ms': {case: [round(min(t), 3), round(max(t), 3)] for case, t in times.items()},
               'runs_ms': {case: [round(x, 3) for x in t] for case, t in times.items()},
               'median_ms': {case: round(m, 3) for case, m in median.items()},
               'wedges_per_s': round(wedges / (sq * 1e-3), 0), 'gathered_GBps': round(4 * gathered / (sq * 1e-3) / 1e9, 2),
               'ratio_to_grx_clustering': round(sq / median['grx_clustering'], 2),
               'ratio_to_triangle_counts': round(sq / median['triangle_counts'], 2),
               'mean_of_column': {case: float(np.mean(K.to_host(out[case])[:csr.n])) for case in cases}}
        if not args.no_profile:
            split = tier_split(name, args.n)
            row['tier_split_ms'] = split
            total = sum(v for v in split.values() if isinstance(v, float))
            if total:
                row['tier_share'] = {tier: round(v / total, 3) for tier, v in split.items()}
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')
        del csr, cases, out


if __name__ == '__main__':
    main()
