"""
Component timings on one GPU (csrc/grx_components.hip), written to profiles/components.txt:

- ba1m_fragments: BA 1 M nodes, m = 10 (synth.ba_edges(1_000_000, 10, seed=0)) with 100 000 isolated nodes and 10 000
  small trees (3 to 12 nodes) added: connected components;
- ba1m_oriented:  a random orientation of that BA graph (every edge keeps one arc): weak, strong, bow tie;
- gnm1m_directed: a directed G(n, m) with n = 1 M and m = 2 n: weak, strong, bow tie.

Every kernel call is timed on its own between two device synchronisations, --reps runs after one warm-up, reported as
min - max.  For scale the same process times grx_biconnected (on the symmetric CSR) and grx_core_numbers on the same
graph.  The strong components are also run through tests/components_oracle.py on the host: its labels must equal the
kernel's, its round count must equal the kernel's, and its outer-iteration count is the one printed (the C entry point
reports rounds only).  The bow tie is one STRONG call and four grx_reachable calls, as graphrole_amd.components.bow_tie
makes them.

    python tools/bench_components.py [--cases ba1m_fragments,ba1m_oriented,gnm1m_directed] [--reps 5] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ('ba1m_fragments', 'ba1m_oriented', 'gnm1m_directed')


def _csr(n, src, dst):
    """(row_ptr, col) of the distinct arcs src -> dst, ascending in each row."""
    key = np.unique(np.asarray(src, dtype=np.int64) * n + np.asarray(dst, dtype=np.int64))
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // n, minlength=n), out=row_ptr[1:])
    return row_ptr, key % n


def _fragments(rng, first):
    """10 000 random trees of 3 to 12 nodes on fresh ids from `first`: (src, dst, the id after the last)."""
    src, dst, at = [], [], first
    for size in rng.integers(3, 13, size=10_000).tolist():
        for k in range(1, size):
            src.append(at + int(rng.integers(0, k)))
            dst.append(at + k)
        at += size
    return np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64), at


def build(case):
    """(n, out CSR, in CSR or None, symmetric CSR) as host arrays."""
    from graphrole_amd import synth
    if case == 'gnm1m_directed':
        n = 1_000_000
        src, dst = synth.er_edges(n, 2 * n, seed=0)
        flip = np.random.default_rng(1).random(len(src)) < 0.5           # er_edges lists src < dst: orient at random
        src, dst = np.where(flip, dst, src), np.where(flip, src, dst)
    else:
        src, dst = synth.ba_edges(1_000_000, 10, seed=0)
        n = 1_000_000
        if case == 'ba1m_fragments':
            rng = np.random.default_rng(2)
            t_src, t_dst, n = _fragments(rng, n + 100_000)
            src, dst = np.concatenate([src, t_src]), np.concatenate([dst, t_dst])
        else:
            flip = np.random.default_rng(3).random(len(src)) < 0.5
            src, dst = np.where(flip, dst, src), np.where(flip, src, dst)
    sym = _csr(n, np.concatenate([src, dst]), np.concatenate([dst, src]))
    if case == 'ba1m_fragments':
        return n, sym, None, sym
    return n, _csr(n, src, dst), _csr(n, dst, src), sym


def _timed(fn, reps):
    import torch
    fn()
    times, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return f'{min(times):.3f} - {max(times):.3f} ms', out


def _histogram(size, label):
    roots = size[label == np.arange(len(label))]
    edges = [1, 2, 3, 4, 8, 16, 64, 1024, 1 << 20, 1 << 40]
    names = ['1', '2', '3', '4-7', '8-15', '16-63', '64-1023', '1024-2^20', '> 2^20']
    counts = np.histogram(roots, bins=edges)[0]
    return ', '.join(f'{nm}: {int(c)}' for nm, c in zip(names, counts) if c) + f'; largest {int(roots.max())}'


def run_case(case, reps, emit):
    from graphrole_amd import kernels as K
    from tests import components_oracle as co
    n, out, inn, sym = build(case)
    d_out, d_sym = K.DeviceCSR(*out), K.DeviceCSR(*sym)
    d_in = K.DeviceCSR(*inn) if inn is not None else None
    emit(f'[{case}] n = {n}, arcs = {int(out[0][-1])}, hub rows = {d_out.n_hubs}'
         + (f' (in: {d_in.n_hubs})' if d_in is not None else ''))
    if inn is None:
        t, (label, size, count, _) = _timed(lambda: K.components(d_sym, mode='connected'), reps)
        emit(f'  connected            {t}   components {count}')
        emit(f'  connected, no sizes  {_timed(lambda: K.components(d_sym, mode="connected", want_size=False), reps)[0]}')
        label, size = K.to_host(label)[:n], K.to_host(size)[:n]
        want = co.components(*sym, co.CONNECTED)
        assert np.array_equal(label, want.label) and np.array_equal(size, want.size) and count == want.n_components
        emit(f'  component sizes      {_histogram(size, label)}')
    else:
        t, (label, size, count, _) = _timed(lambda: K.components(d_out, mode='weak'), reps)
        emit(f'  weak                 {t}   components {count}')
        t, (label, size, count, rounds) = _timed(lambda: K.components(d_out, d_in, mode='strong'), reps)
        label, size = K.to_host(label)[:n], K.to_host(size)[:n]
        want = co.components(*out, co.STRONG)
        assert np.array_equal(label, want.label) and np.array_equal(size, want.size)
        assert (count, rounds) == (want.n_components, want.rounds)
        emit(f'  strong               {t}   components {count}, outer iterations {want.outer}, rounds {rounds}')
        emit(f'  SCC sizes            {_histogram(size, label)}')

        def bow_tie():
            label, size, _, _ = K.components(d_out, d_in, mode='strong')
            label, size = K.to_host(label)[:n], K.to_host(size)[:n]
            roots = np.nonzero(label == np.arange(n))[0]
            core = label == roots[np.lexsort((roots, -size[roots]))[0]]
            reach = lambda csr, member: K.to_host(K.reachable(csr, member.astype(np.int32))[0])[:n] != 0
            inn_ = reach(d_in, core) & ~core
            out_ = reach(d_out, core) & ~core
            from_in, to_out = reach(d_out, inn_), reach(d_in, out_)
            rest = ~(core | inn_ | out_)
            return [int(x.sum()) for x in (core, inn_, out_, rest & from_in & to_out, rest & (from_in ^ to_out),
                                           rest & ~from_in & ~to_out)]
        t, sizes = _timed(bow_tie, reps)
        emit(f'  bow tie              {t}   ' + ', '.join(f'{c} {k}' for c, k in zip(co.BOW_TIE, sizes)))
        assert sizes == np.bincount(co.bow_tie(*out, *inn), minlength=6).tolist()
    emit(f'  grx_biconnected      {_timed(lambda: K.biconnected(d_sym, want_forest=False), reps)[0]}   (symmetric CSR)')
    loops = np.repeat(np.arange(n), np.diff(out[0])) == out[1]
    if loops.any():
        emit('  grx_core_numbers     not run: the graph has self-loops')
    elif inn is None:
        emit(f'  grx_core_numbers     {_timed(lambda: K.core_numbers(d_sym), reps)[0]}')
    else:
        emit(f'  grx_core_numbers     {_timed(lambda: K.core_numbers(d_out, d_in), reps)[0]}   (in + out degree)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'components.txt'))
    args = ap.parse_args()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
    emit(f'tools/bench_components.py --reps {args.reps}: min - max of {args.reps} runs after one warm-up, each timed '
         f'between two device synchronisations')
    for case in args.cases.split(','):
        run_case(case, args.reps, emit)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
