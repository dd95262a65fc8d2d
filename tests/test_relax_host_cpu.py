"""CPU: what the four batch entry points of the tile-relaxation stages (csrc/tile_relax.hpp: cgc_geodesic_rounds,
cgc_reconstruct_rounds, cgc_watershed_rounds, cgc_watershed_jumps) refuse before their fill of the counter and their first launch.
In every call exactly one argument is bad; the workspace and the counter are host memory that a call which got further would hand
to the runtime, so a refusal that is missing shows as another return code, not as CGC_EINVAL."""
import ctypes

import pytest

import cgc_net_amd  # noqa: F401
from cgc_net_amd import _abi, kernels

EINVAL = -1
GOOD = dict(H=4, W=4, connectivity=1, first=0, count=8)


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    lib = ctypes.CDLL(kernels.lib_path())
    _abi.declare(lib)
    return lib


def call(lib, entry, counter, H, W, connectivity, first, count):
    ws = ctypes.create_string_buffer(256)
    ws, counter = ctypes.addressof(ws), (ctypes.addressof(counter) if counter is not None else None)
    if entry == 'geodesic_rounds':
        return lib.cgc_geodesic_rounds(H, W, 5, 7, connectivity, -1, ws, first, count, counter, None)
    if entry == 'reconstruct_rounds':
        return lib.cgc_reconstruct_rounds(H, W, connectivity, ws, first, count, counter, None)
    if entry == 'watershed_rounds':
        return lib.cgc_watershed_rounds(H, W, 5, 7, connectivity, ws, first, count, counter, None)
    assert entry == 'watershed_jumps' and connectivity == 1 and first == 0      # it takes neither
    return lib.cgc_watershed_jumps(H, W, ws, count, counter, None)


ROUNDS = ['geodesic_rounds', 'reconstruct_rounds', 'watershed_rounds']


@pytest.mark.parametrize('entry', ROUNDS + ['watershed_jumps'])
def test_refusals_before_the_fill(lib, entry):
    counter = ctypes.c_int(7)
    for H, W in ((65536, 32768), (2 ** 31 - 1, 2), (-1, 4), (4, -1)):
        assert call(lib, entry, counter, **dict(GOOD, H=H, W=W)) == EINVAL
    if entry in ROUNDS:
        for connectivity in (0, 3, -1):
            assert call(lib, entry, counter, **dict(GOOD, connectivity=connectivity)) == EINVAL
        assert call(lib, entry, counter, **dict(GOOD, first=-1)) == EINVAL
        assert call(lib, entry, counter, **dict(GOOD, first=2 ** 31 - 8, count=8)) == EINVAL      # a round stamps first + count
    for count in (0, -1):
        assert call(lib, entry, counter, **dict(GOOD, count=count)) == EINVAL
    assert call(lib, entry, None, **GOOD) == EINVAL                                                # no counter
    assert counter.value == 7                                                                      # nobody filled it
