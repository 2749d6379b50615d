"""
Structural-hole timings on one GPU (csrc/grx_structural_holes.hip), one JSON line per case:

- ba1m_m10:   BA 1 M nodes, m = 10 (the BASELINE graph, synth.ba_graph(1_000_000, 10, seed=0)), weight=None;
- ba1m_m10_w: the same edges with uniform (0, 1] weights, weight='weight';
- gnm1m:      G(n, m) with 1 M nodes and 1.2 M edges, weight=None;
- dgnm1m:     a directed G(n, m) with 1 M nodes and 10 M arcs, weight=None (mutual weights 1 and 2).

Each line holds the warm time of the constraint column -- kernels.structural_holes on the cached mutual-weight CSR, every
one of --reps runs after --warmup warm-ups timed on its own between two device synchronisations, as a min - max range --
and of the call with all three outputs; in the same process the time of the existing clustering + effective_size path
(kernels.triangle_counts + kernels.local_structure) on the same CSR, as the yardstick; the probe count of the per-arc
stage's bound, sum over arcs of min(d_u, d_v) * ceil(log2 max(d_u, d_v)), from the degrees; the host time of the
directed symmetrisation; and -- unless --no-profile -- the per-kernel split of ONE call from a `rocprofv3 --kernel-trace
--stats` run of its own in a fresh child process (the timed runs are never profiled).

    python tools/bench_structural_holes.py [--cases ba1m_m10,ba1m_m10_w,gnm1m,dgnm1m] [--reps 5] [--warmup 2]
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


def _ba(weighted):
    from graphrole_amd import synth
    from graphrole_amd.graph.csr import CSRGraph
    src, dst = synth.ba_edges(1_000_000, 10, seed=0)
    w = 1.0 - np.random.default_rng(1).random(len(src)) if weighted else None     # (0, 1]
    return CSRGraph(1_000_000, src, dst, weights=w, validate=False)


def _gnm(directed):
    from graphrole_amd import synth
    from graphrole_amd.graph.csr import CSRGraph
    if not directed:
        return synth.er_graph(1_000_000, 1_200_000, seed=0)
    src, dst = synth.er_edges(1_000_000, 9_100_000, seed=0)    # distinct unordered pairs, each in a random direction;
    flip = np.random.default_rng(2).random(len(src)) < 0.5      # the first 900 000 get their reverse as well: 10 M arcs
    src, dst = np.where(flip, dst, src), np.where(flip, src, dst)
    return CSRGraph(1_000_000, np.concatenate([src, dst[:900_000]]), np.concatenate([dst, src[:900_000]]),
                    directed=True, validate=False)


CASES = {
    'ba1m_m10': (lambda: _ba(False), None),
    'ba1m_m10_w': (lambda: _ba(True), 'weight'),
    'gnm1m': (lambda: _gnm(False), None),
    'dgnm1m': (lambda: _gnm(True), None),
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


def _setup(case):
    """(adapter, (csr, z, out_row_ptr), host seconds of building the mutual-weight CSR)."""
    import torch
    from graphrole_amd.measures import _adapter, _mutual_weight_csr
    build, weight = CASES[case]
    graph = _adapter(build())
    graph._device_graph()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mutual = _mutual_weight_csr(graph, graph._K(), weight is not None)
    torch.cuda.synchronize()
    return graph, mutual, time.perf_counter() - t0


def child(case):
    """One warm-up and one call: the process rocprofv3 traces."""
    import torch
    from graphrole_amd import kernels as K
    _, (csr, z, orp), _ = _setup(case)
    K.structural_holes(csr, z, orp)
    K.structural_holes(csr, z, orp)
    torch.cuda.synchronize()


def kernel_split(case):
    """{body<lanes> or body_hub: launches and ms per call} of the grx_rowjoin.h kernels, by their sh_* bodies, from a
    rocprofv3 run of `--child case` (two calls: halved)."""
    if shutil.which('rocprofv3') is None:
        return {'error': 'rocprofv3 not found'}
    out_dir = tempfile.mkdtemp(prefix='sh_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '--',
               sys.executable, os.path.abspath(__file__), '--child', case]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if done.returncode != 0:                                # nothing more on this GPU after a failed run
            raise RuntimeError(f'rocprofv3 exit {done.returncode}: {done.stdout[-400:]}')
        split = {}
        for path in glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True):
            for row in csv.DictReader(open(path)):
                found = re.search(r'(rj_\w+)<(?:(\d+), )?.*?(sh_\w+)>', row.get('Name', ''))
                if found is None:
                    continue
                key = '%s<%s>' % (found.group(3), found.group(2)) if found.group(2) else found.group(3) + '_hub'
                split[key] = {'calls': int(row['Calls']) // 2,
                              'ms': round(float(row['TotalDurationNs']) / 2e6, 4)}
        return dict(sorted(split.items(), key=lambda kv: -kv[1]['ms'])) or {'error': 'no kernel_stats.csv rows'}
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def _probes(graph, csr):
    """The bound of the per-arc stage and what shapes it: (probes, arcs with a hub end's share of them)."""
    g = graph.to_csr()
    if graph.directed:
        row_ptr, col = csr._host
        deg = np.diff(row_ptr)
        du, dv = np.repeat(deg, deg), deg[col]
        both = 1
    else:
        src, dst, _ = g.edge_arrays()
        deg = np.bincount(src, minlength=g.n) + np.bincount(dst, minlength=g.n)
        du, dv = deg[src], deg[dst]
        both = 2                                                # every edge is an arc from both ends
    lo, hi = np.minimum(du, dv), np.maximum(du, dv)
    per_arc = lo * np.ceil(np.log2(np.maximum(hi, 1))).astype(np.int64)
    hub = hi > 32 * csr.lanes_per_row
    return int(both * per_arc.sum()), float(per_arc[hub].sum() / max(per_arc.sum(), 1)), int(both * lo.sum())


def run_case(case, reps, warmup, profile):
    from graphrole_amd import kernels as K
    graph, (csr, z, orp), build_s = _setup(case)
    for _ in range(warmup):
        K.structural_holes(csr, z, orp)
    times, (con, _, _) = _timed(lambda: K.structural_holes(csr, z, orp), reps)
    all_times, _ = _timed(lambda: K.structural_holes(csr, z, orp, want_effective_size=True, want_local=True), reps)
    loops = bool(graph._has_loops) or bool(graph.directed)
    K.local_structure(csr, K.triangle_counts(csr), loops)
    tri_times, _ = _timed(lambda: K.local_structure(csr, K.triangle_counts(csr), loops), reps)
    probes, hub_share, walked = _probes(graph, csr)
    con = K.to_host(con)[:csr.n]
    row = {'case': case, 'n': csr.n, 'arcs': csr.nnz, 'lanes': csr.lanes_per_row, 'hub_rows': csr.n_hubs,
           'weighted': z is not None,
           'constraint_ms': [round(min(times), 3), round(max(times), 3)], 'runs_ms': [round(t, 3) for t in times],
           'all_outputs_ms': [round(min(all_times), 3), round(max(all_times), 3)],
           'clustering_effective_size_ms': [round(min(tri_times), 3), round(max(tri_times), 3)],
           'ratio': round(float(np.median(times) / np.median(tri_times)), 1),
           'probes': probes, 'walked_entries': walked, 'probe_share_of_hub_arcs': round(hub_share, 3),
           'ns_per_probe': round(1e6 * float(np.median(times)) / max(probes, 1), 4),
           'mutual_csr_build_s': round(build_s, 3),
           'constraint_nan': int(np.isnan(con).sum()), 'constraint_mean': float(np.nanmean(con))}
    if profile:
        row['kernel_split_ms'] = kernel_split(case)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='ba1m_m10,ba1m_m10_w,gnm1m,dgnm1m')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child)
        return
    for case in args.cases.split(','):
        line = json.dumps(run_case(case, args.reps, args.warmup, not args.no_profile))
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
