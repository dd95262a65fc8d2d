"""CPU: the host side of the image stage (label.hip, edt.hip, geodesic.hip, nuclei.hip; cgc_net_amd.nuclei).  The five workspace
sizing entry points against closed forms written out here -- the launchers carve the same layouts, so a piece that moves or changes
size shows up as a different total -- and the pure argument helpers of nuclei.py, which need no GPU tensor."""
import ctypes
import math

import pytest

import cgc_net_amd  # noqa: F401
from cgc_net_amd import _abi, kernels, nuclei

SHAPES = [(1, 1), (1, 37), (41, 1), (7, 5), (64, 64), (65, 63), (64, 65), (129, 257), (300, 300), (3, 2100), (0, 5), (4, 0)]


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    lib = ctypes.CDLL(kernels.lib_path())
    _abi.declare(lib)
    return lib


def a(x):
    return (x + 255) // 256 * 256


def cdiv(x, y):
    return -(-x // y)


@pytest.mark.parametrize('H,W', SHAPES)
def test_image_workspace_sizes(lib, H, W):
    n = H * W
    for c in (0, 1):
        assert lib.cgc_label_ws_bytes(H, W, c) == a(4 * n) * (2 if c else 1) + a(4 * cdiv(n, 2048))
    assert lib.cgc_edt_ws_bytes(H, W) == a(8 * cdiv(H, 64) * W) + a(2 * n)
    assert lib.cgc_geodesic_ws_bytes(H, W) == a(8 * n) + a(n) + a(4 * cdiv(H, 64) * cdiv(W, 64))


def test_nuclei_workspace_sizes(lib):
    for m in (0, 1, 63, 64, 1000):
        assert lib.cgc_nuclei_ws_bytes(m) == 5 * a(4 * (m + 1)) + 2 * a(8 * (m + 1)) + a(4 * (m + 1))
    for k, px in ((1, 5000), (3, 70000), (100, 5000)):
        slot = a(4 * px) + 2 * a(px) + a(4 * 65536) + a(4 * (4 * px + 8))
        assert lib.cgc_nuclei_big_ws_bytes(k, ctypes.c_int64(px)) == min(k, 32) * slot


def test_sizing_refusals(lib):
    for H, W in ((65536, 32768), (32768, 65536), (2 ** 31 - 1, 2)):          # H * W >= 2^31
        assert lib.cgc_label_ws_bytes(H, W, 0) == 0 and lib.cgc_label_ws_bytes(H, W, 1) == 0
        assert lib.cgc_geodesic_ws_bytes(H, W) == 0 and lib.cgc_edt_ws_bytes(H, W) == 0
    assert lib.cgc_label_ws_bytes(46340, 46340, 0) > 0 and lib.cgc_geodesic_ws_bytes(46340, 46340) > 0      # just below 2^31
    assert lib.cgc_edt_ws_bytes(32767, 32767) > 0
    assert lib.cgc_edt_ws_bytes(32768, 1) == 0 and lib.cgc_edt_ws_bytes(1, 32768) == 0                       # a side > 32767
    for H, W in ((-1, 4), (4, -1), (-3, -3)):
        assert lib.cgc_label_ws_bytes(H, W, 1) == 0 and lib.cgc_edt_ws_bytes(H, W) == 0 and lib.cgc_geodesic_ws_bytes(H, W) == 0
    assert lib.cgc_nuclei_ws_bytes(-1) == 0


# ------------------------------------------------------------------ argument helpers of nuclei.py
@pytest.mark.parametrize('distance,d2max', [(0, 0), (1, 1), (1.5, 2), (2 ** 0.5, 2), (3, 9), (10, 100)])
def test_d2max(distance, d2max):
    assert nuclei._d2max(distance, 'max_distance') == d2max
    assert nuclei._d2max(float(distance), 'max_distance') == d2max


@pytest.mark.parametrize('distance,dmax', [(0, 0), (1, 5), (1.5, 7), (3, 15), (10, 50)])
def test_geodesic_bound(distance, dmax):
    assert nuclei._geodesic_bound(distance, 5, 'max_distance') == dmax


def test_bounds_cap_and_refuse():
    for huge in (1e6, 1e300, float('inf')):
        assert nuclei._d2max(huge, 'distance') == nuclei.EDT_INF - 1
    for huge in (1e10, 1e300, float('inf')):
        assert nuclei._geodesic_bound(huge, 5, 'distance') == nuclei.GEO_INF - 1
    assert nuclei._d2max(math.sqrt(nuclei.EDT_INF - 1), 'distance') == nuclei.EDT_INF - 1
    assert nuclei._geodesic_bound(nuclei.GEO_INF - 1, 1, 'distance') == nuclei.GEO_INF - 1
    for bad in (-1, -0.5, float('nan')):
        with pytest.raises(ValueError):
            nuclei._d2max(bad, 'distance')
        with pytest.raises(ValueError):
            nuclei._geodesic_bound(bad, 5, 'distance')


def test_geodesic_steps():
    assert nuclei._geodesic_steps('cityblock') == (1, 0)
    assert nuclei._geodesic_steps('chessboard') == (1, 1)
    assert nuclei._geodesic_steps('chamfer') == (5, 7)
    assert nuclei._geodesic_steps((3, 4)) == (3, 4)
    for bad in ('euclid', (0, 0), (2, 1), (2, 5), (1, -1), (1.5, 2), (5,), 5, None):
        with pytest.raises(ValueError):
            nuclei._geodesic_steps(bad)
