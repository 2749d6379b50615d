"""
The workspace sizes of the four betweenness entry points, stated from the layout alone and compared with the library
(no device: the *_workspace_bytes functions are host arithmetic).

Layout, every array on a 256-byte boundary, `cells` = n * width:
  grx_betweenness            level int32[cells], sigma fp64[cells], delta fp64[cells], reach int32[width], 256 bytes of
                             control words; grx_edge_betweenness: one more fp64[cells] (coeff)
  grx_weighted_betweenness   D, delta, sigma fp64[cells] each, depth int32[cells], stamp int32[n], reach (256 bytes),
                             256 bytes of control words; grx_weighted_edge_betweenness: one more fp64[cells] (coeff)
Width 0 is the library's choice under a 4 GiB state budget:
  hops     the widest multiple of 64 up to 256 with n * width * (20, edges 28) bytes within the budget, at least 64, and
           no wider than the source list rounded up to a multiple of 64
  weight   the widest of 16, 32, 64 with n * (width * (28, edges 36) + 4) bytes within the budget, and no wider than the
           source list rounded up to one of them
"""
import pytest

BUDGET = 4 << 30
SIZES = (1, 10, 70_001)
BIG = (700_000, 1_000_000, 2_000_000, 1 << 22)                 # where the budget narrows the library's choice
SOURCES = (0, 1, 16, 17, 64, 65, 70, 200, 1 << 20)


def _up(nbytes: int) -> int:
    return (nbytes + 255) // 256 * 256


def hops_bytes(n: int, width: int, edges: bool) -> int:
    cells = n * width
    return _up(4 * cells) + (3 if edges else 2) * _up(8 * cells) + _up(4 * width) + 256


def weight_bytes(n: int, width: int, edges: bool) -> int:
    cells = n * width
    return (4 if edges else 3) * _up(8 * cells) + _up(4 * cells) + _up(4 * n) + 256 + 256


def hops_width(n: int, n_sources: int, edges: bool) -> int:
    fits = BUDGET // (n * (28 if edges else 20)) // 64 * 64
    return min(max(64, min(fits, 256)), max(64, -(-n_sources // 64) * 64))


def weight_width(n: int, n_sources: int, edges: bool) -> int:
    widest = 16
    while widest < 64 and n * (2 * widest * (36 if edges else 28) + 4) <= BUDGET:
        widest *= 2
    width = 16
    while width < widest and width < n_sources:
        width *= 2
    return width


@pytest.fixture(scope='module')
def lib():
    from graphrole_amd import _lib
    return _lib.load()


@pytest.mark.parametrize('edges', [False, True], ids=['nodes', 'edges'])
def test_hops_workspace_is_the_layout(lib, edges):
    size = lib.grx_edge_betweenness_workspace_bytes if edges else lib.grx_betweenness_workspace_bytes
    for n in SIZES + BIG:
        for width in (64, 128, 192, 256):
            for n_sources in (1, 70):
                assert size(n, width, n_sources) == hops_bytes(n, width, edges), (n, width, n_sources)
        for n_sources in SOURCES:
            want = hops_bytes(n, hops_width(n, n_sources, edges), edges)
            assert size(n, 0, n_sources) == want, (n, n_sources)
    assert len({hops_width(n, 1 << 20, edges) for n in BIG}) >= 3    # the budget is what chooses at these sizes


@pytest.mark.parametrize('edges', [False, True], ids=['nodes', 'edges'])
def test_weight_workspace_is_the_layout(lib, edges):
    size = lib.grx_weighted_edge_betweenness_workspace_bytes if edges else lib.grx_weighted_betweenness_workspace_bytes
    for n in SIZES + BIG:
        for width in (16, 32, 64):
            for n_sources in (1, 70):
                assert size(n, width, n_sources) == weight_bytes(n, width, edges), (n, width, n_sources)
        for n_sources in SOURCES:
            want = weight_bytes(n, weight_width(n, n_sources, edges), edges)
            assert size(n, 0, n_sources) == want, (n, n_sources)
        # a width the entry point would refuse sizes like the library's choice
        assert size(n, 48, 70) == size(n, 0, 70), n
    assert len({weight_width(n, 1 << 20, edges) for n in BIG}) >= 2  # the budget is what chooses at these sizes
