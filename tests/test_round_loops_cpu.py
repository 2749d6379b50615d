"""
The paths of tests/round_loop_cases.py reach the batch boundaries they exist for -- from the oracles alone, no kernel:
the BFS depth from an end is n - 1 (so the level loops need n launches), the peeling takes ceil(n / 2) rounds, and the
counts lie on both sides of the batch sizes of the device loops.
"""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import closeness_oracle as co
from tests import round_loop_cases as rl

CSRC = Path(__file__).resolve().parent.parent / 'graphrole_amd' / 'csrc'


@pytest.mark.parametrize('directed', [False, True], ids=['undirected', 'directed'])
def test_bfs_depth_from_an_end_is_n_minus_1(directed):
    for n in rl.SIZES:
        row_ptr, col, _, _ = rl.path_csrs(n, directed)
        levels = co.bfs_levels(row_ptr, col, 0)
        assert levels.max() == n - 1 and np.array_equal(levels, np.arange(n)), n
        assert rl.biconnected(n).level.max() == n - 1, n          # the forest's root is node 0, an end
        assert rl.distance_sums(n, directed)[1].max() == n * (n - 1) // 2, n   # the far end sums 1 + ... + (n - 1)


@pytest.mark.parametrize('directed', [False, True], ids=['undirected', 'directed'])
def test_peeling_takes_half_n_rounds(directed):
    for n in rl.SIZES:
        want = rl.core_numbers(n, directed)
        assert want.onion.max() == want.n_rounds == (n + 1) // 2, n


def test_the_counts_straddle_the_batches():
    launches = {int(co.bfs_levels(*rl.path_csrs(n, False)[:2], 0).max()) + 1 for n in rl.SIZES}
    rounds = {int(rl.core_numbers(n, False).onion.max()) for n in rl.SIZES}
    for multiple in (rl.LEVEL_BATCH, 2 * rl.LEVEL_BATCH, 3 * rl.LEVEL_BATCH):
        assert {multiple - 1, multiple, multiple + 1} <= launches
    assert {7, 8, 9, 15, 16, 17} <= launches
    assert {rl.ROUND_BATCH - 1, rl.ROUND_BATCH, rl.ROUND_BATCH + 1} == {15, 16, 17} <= rounds


def test_the_batches_are_the_ones_of_the_sources():
    def constant(file, name):
        return int(re.search(rf'constexpr int {name} = (\d+);', (CSRC / file).read_text()).group(1))

    assert constant('grx_brandes.h', 'BR_LEVEL_BATCH') == rl.LEVEL_BATCH     # all four betweenness entry points
    assert constant('grx_closeness.hip', 'CL_LEVEL_BATCH') == rl.LEVEL_BATCH
    assert constant('grx_biconnected.hip', 'BC_LEVEL_BATCH') == rl.LEVEL_BATCH
    assert constant('grx_kcore.hip', 'KC_ROUND_BATCH') == rl.ROUND_BATCH
