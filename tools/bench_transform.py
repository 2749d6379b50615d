"""
Role-transfer timings on one GPU (not a test): RoleExtractor.transform and its parts on the feature table of the
1 M-node Barabasi-Albert graph with the roles of the BASELINE step (bench.py: max_generations = 4, n_roles = 6), and
RecursiveFeatureExtractor.replay_features of the final columns against extract_features() of the same graph.

    python tools/bench_transform.py [--n 1000000] [--m 10] [--reps 5] [--sklearn-rows 0]

Every figure is min - max over --reps runs after a warm-up, host clock between two device synchronisations, profiler
off; the per-kernel split is one extra run with the library's event profiler on.  The comparator is measured in the
same process on the same table: the same number of iterations through grx_nmf_w_pass with H held fixed (what a user
could assemble before grx_nmf_transform existed; it streams X once per iteration).  sklearn's NMF(solver='mu')
.transform runs once on the host CPU on the whole table (--sklearn-rows N: on the first N rows only, extrapolated
linearly and reported as extrapolated -- for tables on which the full run takes over a minute).  One JSON line.
"""
import argparse
import ctypes
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def span(times):
    return {'min_ms': round(min(times) * 1e3, 3), 'max_ms': round(max(times) * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--m', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sklearn-rows', type=int, default=0, help='0 = the whole table')
    args = ap.parse_args()
    import torch
    from graphrole_amd import RecursiveFeatureExtractor, RoleExtractor, _lib, synth
    from graphrole_amd import kernels as K
    from graphrole_amd.roles import factor

    def timed(fn, reps=args.reps):
        fn()                                                  # warm-up
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return out

    G = synth.ba_graph(args.n, args.m, seed=0)
    fe = RecursiveFeatureExtractor(G, max_generations=4)
    features = fe.extract_features()
    np.random.seed(0)
    rx = RoleExtractor(n_roles=6)
    rx.extract_role_factors(features)
    H = np.ascontiguousarray(rx.role_feature_factor.to_numpy(dtype=np.float64))
    n, F = features.shape
    r = H.shape[0]
    result = {'n': n, 'F': F, 'r': r, 'reps': args.reps}

    # ---- transform: the public call, the device call, its kernels
    Xd, _ = factor.device_matrix(features)
    W, info = K.nmf_transform(Xd, n, H)
    n_iter = int(info.n_iter)
    result['n_iter'] = n_iter
    result['direct_residuals'] = int(info.direct_residuals)
    result['transform_api'] = span(timed(lambda: rx.transform(features)))
    result['transform_roles_api'] = span(timed(lambda: rx.transform_roles(features), reps=2))
    result['grx_nmf_transform'] = span(timed(lambda: K.nmf_transform(Xd, n, H)))
    lib = _lib.load()
    names = [lib.grx_profile_kernel_name(i).decode() for i in range(lib.grx_profile_kernel_count())]
    lib.grx_profile_enable(1)
    lib.grx_profile_reset()
    K.nmf_transform(Xd, n, H)
    split = {}
    for name in ('transform_norms_kernel', 'project_kernel', 'nmf_transform_block_kernel', 'nmf_residual_kernel'):
        ms, launches = ctypes.c_double(0.0), ctypes.c_longlong(0)
        lib.grx_profile_read(names.index(name), ctypes.byref(ms), ctypes.byref(launches))
        split[name] = {'launches': int(launches.value), 'ms': round(ms.value, 4)}
    lib.grx_profile_enable(0)
    result['kernel_split'] = split
    # (the first of these launches writes W0 and its error terms without an update)
    result['block_ms_per_launch'] = round(split['nmf_transform_block_kernel']['ms'] /
                                          max(split['nmf_transform_block_kernel']['launches'], 1), 4)
    result['bytes'] = {'X_pass': n * F * 8, 'block': 3 * n * r * 8}

    # ---- comparator: n_iter W passes of the fit's kernel with H fixed, same table, same process
    W0 = np.full((r, Xd.shape[1]), np.sqrt(float(features.to_numpy(dtype=np.float64).mean()) / r))

    def w_passes():
        state.W.copy_(W0d)
        for _ in range(n_iter):
            state.w_pass()

    W0d = K.to_device(W0)
    state = K.NmfState(Xd, n, K.to_device(W0), H)
    result['w_pass_loop'] = span(timed(w_passes))
    diff = K.to_host(state.W)[:, :n] - K.to_host(W)[:, :n]
    result['w_pass_loop_vs_transform_relmax'] = float(np.abs(diff).max() / np.abs(K.to_host(W)[:, :n]).max())

    # ---- sklearn on the host CPU (a row subset, extrapolated)
    try:
        from sklearn.decomposition import NMF
        warnings.simplefilter('ignore')
        rows = min(args.sklearn_rows, n) if args.sklearn_rows > 0 else n
        Xs = np.ascontiguousarray(features.to_numpy(dtype=np.float64)[:rows])
        model = NMF(n_components=r, solver='mu', init='nndsvda')
        model.components_, model.n_components_, model.n_features_in_ = H.copy(), r, F
        t0 = time.perf_counter()
        _, _, it = model._fit_transform(Xs, H=model.components_, update_H=False)
        dt = time.perf_counter() - t0
        result['sklearn_cpu'] = {'rows': rows, 'n_iter': int(it), 'ms': round(dt * 1e3, 1),
                                 **({'extrapolated_full_table_ms': round(dt * 1e3 * n / rows, 1)} if rows < n else {}),
                                 'threads': os.cpu_count() if 'OMP_NUM_THREADS' not in os.environ else int(os.environ['OMP_NUM_THREADS'])}
    except ImportError:
        result['sklearn_cpu'] = 'not measured (scikit-learn is not installed)'

    # ---- replay of the final columns against extract_features() of the same graph
    columns = list(features.columns)
    replayed = fe.replay_features(columns)
    result['replay_equals_extract'] = bool(replayed.equals(features))
    result['replay_features'] = span(timed(lambda: fe.replay_features(columns)))

    def extract():
        fe.reset()
        fe.extract_features()

    result['extract_features'] = span(timed(extract))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
