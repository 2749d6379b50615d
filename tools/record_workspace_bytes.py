#!/usr/bin/env python3
"""
tools/record_workspace_bytes.py -- record what every ``size_t grx_*_workspace_bytes(...)`` of include/grx.h returns
over a grid of shapes, into tests/golden/workspace_bytes.json (tests/test_workspace_bytes_cpu.py reads it):

    PYTHONDONTWRITEBYTECODE=1 python tools/record_workspace_bytes.py [out.json]

The functions are host arithmetic and need no device.  The header is parsed for the functions and their argument
names; every argument takes the values GRID lists under its name and a function is called on the cross product, first
argument slowest (itertools.product), through graphrole_amd._lib.load() -- GRX_LIB_PATH selects the build.  Record with
the build whose layouts are the reference (the commit before a change of the host-side layout code), never with the
build under test.

The file: {"grid": {argument: [values]}, "functions": {name: {"args": [argument names], "bytes": [one value per
row of the product]}}}.
"""
import itertools
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

HEADER = os.path.join(ROOT, 'include', 'grx.h')
OUT = os.path.join(ROOT, 'tests', 'golden', 'workspace_bytes.json')

# 63 / 64 / 65 straddle a 256-byte boundary of an int32 array; at 2^22 nodes the 4 GiB state budgets narrow the batch
# width; the m values are the thresholds KM_SMALL_M, Q_CELLS and QC_BIG and their neighbours
GRID = {
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


def declared(header_text):
    """{function: [argument names]} of every size_t grx_*_workspace_bytes declaration, in header order."""
    out = {}
    for name, args in re.findall(r'^size_t\s+(grx_\w+_workspace_bytes)\s*\(([^)]*)\)\s*;', header_text, re.M):
        args = args.strip()
        out[name] = [] if args in ('', 'void') else [a.split()[-1].lstrip('*') for a in args.split(',')]
    return out


def rows(args, grid):
    """The argument tuples of one function, in the order the recorded values are stored."""
    return itertools.product(*(grid[a] for a in args))


def record():
    from graphrole_amd import _lib
    lib = _lib.load()
    functions = {}
    for name, args in declared(open(HEADER).read()).items():
        fn = getattr(lib, name)
        functions[name] = {'args': args, 'bytes': [int(fn(*row)) for row in rows(args, GRID)]}
    return {'grid': GRID, 'functions': functions}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    data = record()
    with open(out, 'w') as f:
        f.write('{"grid": ' + json.dumps(data['grid']) + ',\n "functions": {\n')
        f.write(',\n'.join(f'  {json.dumps(name)}: {json.dumps(entry)}' for name, entry in data['functions'].items()))
        f.write('\n }}\n')
    total = sum(len(entry['bytes']) for entry in data['functions'].values())
    print(f'{out}: {len(data["functions"])} functions, {total} rows')


if __name__ == '__main__':
    main()
