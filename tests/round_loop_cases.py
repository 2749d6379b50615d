"""
The graphs of the round-loop boundary tests (tests/test_gpu_round_loops.py, tests/test_round_loops_cpu.py): every path
of 1 .. 40 nodes, rows in node order, undirected and directed (0 -> 1 -> ... -> n - 1), with the oracles' results on
them computed once per process.

Why paths: the device-steered loops (csrc/grx_common.h) enqueue a fixed batch of rounds between two read-backs -- 8 BFS
levels (betweenness, closeness, biconnected), 16 peeling rounds (k-core).  A path of n nodes has BFS depth n - 1 from
an end, so its level loop needs n launches (the last one finds the empty frontier): 1 .. 40, on both sides of every
multiple of 8.  Its peeling takes ceil(n / 2) rounds: 15, 16, 17 at n = 29 .. 34, on both sides of 16.
"""
from functools import lru_cache

import numpy as np

from tests import betweenness_oracle as bo
from tests import biconnected_oracle as bico
from tests import closeness_oracle as co
from tests import kcore_oracle as ko

SIZES = tuple(range(1, 41))
LEVEL_BATCH = 8
ROUND_BATCH = 16


@lru_cache(maxsize=None)
def path_csrs(n, directed):
    """(row_ptr, col, in_row_ptr, in_col) of the path 0 - 1 - ... - (n - 1); undirected: the in CSR is the out CSR."""
    edges = [(v, v + 1) for v in range(n - 1)]
    if not directed:
        out = ko.symmetric_csr(n, edges)
        return out + out
    return ko.directed_csr(n, edges) + ko.directed_csr(n, [(v, u) for u, v in edges])


@lru_cache(maxsize=None)
def distance_sums(n, directed):
    """(reach, dsum, harmonic fp64) with every node a source, walking the out-arcs."""
    row_ptr, col, in_row_ptr, in_col = path_csrs(n, directed)
    reach, dsum, harm = co.distance_sums(row_ptr, col, range(n), in_adjacency=(in_row_ptr, in_col))
    return reach, dsum, np.array([co.harm_to_float(h) for h in harm], dtype=np.float64)


def betweenness_scale(n, directed):
    scale = bo.rescale_factor(n, True, directed, None, False)
    return 1.0 if scale is None else scale


@lru_cache(maxsize=None)
def betweenness(n, directed):
    row_ptr, col, _, _ = path_csrs(n, directed)
    return bo.betweenness_arrays(row_ptr, col, range(n), directed)


@lru_cache(maxsize=None)
def biconnected(n):
    row_ptr, col, _, _ = path_csrs(n, False)
    return bico.biconnected(row_ptr, col)


@lru_cache(maxsize=None)
def core_numbers(n, directed):
    row_ptr, col, in_row_ptr, in_col = path_csrs(n, directed)
    return ko.core_numbers(row_ptr, col, in_row_ptr, in_col) if directed else ko.core_numbers(row_ptr, col)
