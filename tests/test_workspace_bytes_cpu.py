"""
Every grx_*_workspace_bytes of include/grx.h returns exactly what tests/golden/workspace_bytes.json recorded for it
(tools/record_workspace_bytes.py, run on the build before the workspace layouts moved onto the common carver GrxCarve):
a change of the host code that lays a workspace out must not change a size for any shape.  No device: the functions are
host arithmetic.  The GPU side of the same contract is the guard-band suites, which hand every entry point exactly the
published size between poisoned guards.
"""
import json
import os

import pytest

from tools import record_workspace_bytes as recorder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'workspace_bytes.json')

# the least the grid must hold per argument: the alignment straddles, the thresholds and the budget-bound sizes
REQUIRED = {
    'n': [0, 1, 63, 64, 65, 1000, 4097, 70_001, 1 << 22],
    'm': [1, 64, 65, 1000, 1024, 1025, 4096, 4097, 8192, 8193, 70_001, 1 << 22],
    'nnz': [0, 1, 65, 1000, 70_001, 1 << 24],
    'nq': [1, 65, 1000],
    'batch': [0, 16, 32, 64, 128, 192, 256],
    'words': [0, 1, 2, 4, 8, 16],
    'n_sources': [1, 17, 65, 200, 1 << 20],
    'directed': [0, 1],
    'F': [1, 20, 480],
    'r': [1, 6, 16],
    'k': [1, 10, 64],
    'c': [1, 8, 33],
    'segments': [0, 1, 256],
    'ncols': [1, 12, 128],
}


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def declared():
    return recorder.declared(open(recorder.HEADER).read())


def test_every_declared_function_has_rows(golden, declared):
    assert len(declared) >= 34, sorted(declared)
    assert set(golden['functions']) == set(declared)
    for name, args in declared.items():
        entry = golden['functions'][name]
        assert entry['args'] == args, name                     # recorded under the header's argument names
        assert len(entry['bytes']) == len(list(recorder.rows(args, golden['grid']))) >= 1, name


def test_grid_holds_the_threshold_values(golden):
    for arg, values in REQUIRED.items():
        assert set(values) <= set(golden['grid'][arg]), arg


def test_sizes_are_the_recorded_ones(golden, declared):
    from graphrole_amd import _lib
    lib = _lib.load()
    wrong = []
    for name, entry in golden['functions'].items():
        fn = getattr(lib, name)
        for row, want in zip(recorder.rows(entry['args'], golden['grid']), entry['bytes']):
            got = int(fn(*row))
            if got != want:
                wrong.append((name, dict(zip(entry['args'], row)), got, want))
    assert not wrong, f'{len(wrong)} sizes differ from the recording, the first: {wrong[:5]}'
