"""CPU: the host side of the seeded-watershed stage (csrc/watershed.hip; cgc_net_amd.nuclei.watershed, split_touching(growth='flood')):
what the public functions refuse before their first launch, the workspace size against its closed form and what the library refuses
without launching.

As in tests/test_reconstruct_host_cpu.py the tests lift the "on the GPU" refusal (``on_gpu=False``) and replace the kernel table by
one that fails the test when it is asked for: every refusal checked here is raised before any launch."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import _abi, kernels, nuclei


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    lib = ctypes.CDLL(kernels.lib_path())
    _abi.declare(lib)
    return lib


@pytest.fixture
def no_launch(monkeypatch):
    """Host tensors pass the image check; asking for the kernel table fails the test."""
    check = nuclei._check_image

    def lifted(fn, name, image, dtypes=None, on_gpu=True):
        return check(fn, name, image, on_gpu=False) if dtypes is None else check(fn, name, image, dtypes, on_gpu=False)

    def refuse():
        pytest.fail('a launch was reached')

    monkeypatch.setattr(nuclei, '_check_image', lifted)
    monkeypatch.setattr(kernels, 'get', refuse)


def test_only_tensors_on_the_gpu():
    good = torch.zeros(4, 5, dtype=torch.uint8)
    for bad in (good, np.zeros((4, 5), np.uint8), [[0, 1], [1, 0]], None):
        with pytest.raises(TypeError):
            nuclei.watershed(bad, bad)
    with pytest.raises(TypeError):
        nuclei.split_touching(good, 2, growth='flood')
    with pytest.raises(TypeError):
        nuclei.split_touching(good, None, growth='flood', markers='h_maxima', h=1)


def test_watershed_dtypes_and_dimensions(no_launch):
    m = torch.zeros(4, 5, dtype=torch.int32)
    for dtype in (torch.int64, torch.float32, torch.float64, torch.float16):
        with pytest.raises(TypeError):
            nuclei.watershed(torch.zeros(4, 5, dtype=dtype), m)                  # heights must fit int32
    for dtype in (torch.float32, torch.float16):
        with pytest.raises(TypeError):
            nuclei.watershed(m, torch.zeros(4, 5, dtype=dtype))
        with pytest.raises(TypeError):
            nuclei.watershed(m, m, within=torch.zeros(4, 5, dtype=dtype))
    for shape in ((5,), (2, 4, 5), ()):
        with pytest.raises(ValueError):
            nuclei.watershed(torch.zeros(shape, dtype=torch.int32), torch.zeros(shape, dtype=torch.int32))
    for other in (torch.zeros(5, 4, dtype=torch.int32), torch.zeros(4, 6, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            nuclei.watershed(m, other)
        with pytest.raises(ValueError):
            nuclei.watershed(m, m, within=other)
    for good in (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32):
        for markers in (torch.bool, torch.uint8, torch.int16, torch.int64):
            with pytest.raises(ValueError):                                      # the dtypes pass, the connectivity does not
                nuclei.watershed(m.to(good), m.to(markers), within=m.to(torch.int64), connectivity=3)


def test_watershed_steps_and_connectivity(no_launch):
    m = torch.zeros(4, 5, dtype=torch.int16)
    for bad in (0, 3, 4, '1', None, 1.5):
        with pytest.raises(ValueError):
            nuclei.watershed(m, m, connectivity=bad)
    for bad in ('euclidean', 'l2', None, (0, 0), (1, 3), (2, 1), (1.5, 2), (1,), (1, 2, 3), (-1, 0)):
        with pytest.raises(ValueError):
            nuclei.watershed(m, m, metric=bad)


def test_the_kernel_table_refuses_before_any_copy():
    """HipKernels.watershed_flood checks steps, connectivity and overflow before it touches a tensor: shapes alone are enough."""
    class Shape(object):
        dtype = torch.int32

        def __init__(self, *shape):
            self.shape = shape

    flood = kernels.HipKernels.watershed_flood
    img = Shape(4, 5)
    for a, b in ((0, 0), (1, 3), (2, 1), (-1, 0)):
        with pytest.raises(ValueError):
            flood(None, img, img, None, a, b, 1)
    for connectivity in (0, 3, None):
        with pytest.raises(ValueError):
            flood(None, img, img, None, 5, 7, connectivity)
    big = Shape(20000, 20000)                                                    # 7 * 4e8 >= 2^31
    with pytest.raises(ValueError):
        flood(None, big, big, None, 5, 7, 1)
    with pytest.raises(ValueError):
        flood(None, big, big, None, 6, 0, 1)                                     # b == 0: a counts


def test_split_touching_refusals(no_launch):
    m = torch.zeros(6, 7, dtype=torch.uint8)
    split = nuclei.split_touching
    for bad in ('watershed', 'Flood', 'floods', None, 1):
        with pytest.raises(ValueError):
            split(m, 2, growth=bad)                                              # 'watershed' is still no growth
    with pytest.raises(ValueError):
        split(m, 2, growth='flood', markers='watershed')
    # 'flood' itself is accepted: each refusal below is about another argument and says so
    with pytest.raises(ValueError, match='h is only used'):
        split(m, 2, growth='flood', h=1)                                         # h without markers='h_maxima'
    with pytest.raises(ValueError, match='needs h'):
        split(m, 2, growth='flood', markers='h_maxima')                          # h is required
    for bad in (0, 0.1, -1, float('nan')):
        with pytest.raises(ValueError, match='h must be'):
            split(m, 2, growth='flood', markers='h_maxima', h=bad)
    with pytest.raises(ValueError, match='core_radius'):
        split(m, -1, growth='flood')                                             # 'core' still checks its radius
    with pytest.raises(ValueError, match='connectivity'):
        split(m, 2, growth='flood', connectivity=3)
    with pytest.raises(ValueError, match='min_size'):
        split(m, 2, growth='flood', min_size=-1)
    with pytest.raises(ValueError, match='connectivity'):
        split(m, None, growth='flood', markers='h_maxima', h=1, connectivity=0)
    with pytest.raises(ValueError, match="'geodesic' or 'flood'"):
        split(m, 2, growth='euclidean', markers='h_maxima', h=1)                 # still needs a growth along paths


def test_signatures():
    p = inspect.signature(nuclei.watershed).parameters
    assert list(p) == ['height', 'markers', 'within', 'metric', 'connectivity', 'return_level']
    assert [p[k].default for k in list(p)[2:]] == [None, 'chamfer', 1, False]
    q = inspect.signature(nuclei.split_touching).parameters
    assert (q['growth'].default, q['markers'].default, q['h'].default) == ('euclidean', 'core', None)
    assert 'Host syncs' in nuclei.watershed.__doc__ and "growth='flood'" in nuclei.split_touching.__doc__
    assert 'watershed' in nuclei.__doc__


def test_the_cpu_twin_has_no_flood():
    with pytest.raises(NotImplementedError):
        kernels.KernelSpec().watershed_flood(None, None, None, 5, 7, 1)
    assert kernels.WS_JUMP_BATCH >= 1


# ------------------------------------------------------------------ the library, without a launch
def a(x):
    return (x + 255) // 256 * 256


def cdiv(x, y):
    return -(-x // y)


@pytest.mark.parametrize('H,W', [(1, 1), (1, 37), (41, 1), (7, 5), (64, 64), (65, 63), (64, 65), (129, 257), (300, 300), (3, 2100),
                                 (0, 5), (4, 0)])
def test_workspace_size(lib, H, W):
    # keys (8 bytes), domain (1), heights (4), pointers (4) per pixel, one stamp per 64 x 64 tile
    want = a(8 * H * W) + a(H * W) + 2 * a(4 * H * W) + a(4 * cdiv(H, 64) * cdiv(W, 64))
    assert lib.cgc_watershed_ws_bytes(H, W) == want


def test_library_refusals(lib):
    einval = -1
    for H, W in ((65536, 32768), (32768, 65536), (2 ** 31 - 1, 2), (-1, 4), (4, -1)):
        assert lib.cgc_watershed_ws_bytes(H, W) == 0
        assert lib.cgc_watershed_begin(None, None, 1, None, 0, H, W, 1, 0, None, None) == einval
        assert lib.cgc_watershed_rounds(H, W, 1, 0, 1, None, 0, 8, None, None) == einval
        assert lib.cgc_watershed_parents(H, W, 1, 0, 1, None, None) == einval
        assert lib.cgc_watershed_jumps(H, W, None, 8, None, None) == einval
        assert lib.cgc_watershed_finish(H, W, None, None, None, None) == einval
    assert lib.cgc_watershed_ws_bytes(46340, 46340) > 0                                       # just below 2^31
    for a_, b_ in ((0, 0), (-1, 0), (1, 3), (2, 1), (5, 11)):                                  # step costs
        assert lib.cgc_watershed_begin(None, None, 1, None, 0, 4, 4, a_, b_, None, None) == einval
        assert lib.cgc_watershed_rounds(4, 4, a_, b_, 1, None, 0, 8, None, None) == einval
        assert lib.cgc_watershed_parents(4, 4, a_, b_, 1, None, None) == einval
    assert lib.cgc_watershed_begin(None, None, 1, None, 0, 20000, 20000, 5, 7, None, None) == einval      # 7 H W reaches 2^31
    assert lib.cgc_watershed_begin(None, None, 1, None, 0, 20000, 20000, 6, 0, None, None) == einval
    for bytes_ in (0, 3, 5, 16, -1):
        assert lib.cgc_watershed_begin(None, None, bytes_, None, 0, 4, 4, 5, 7, None, None) == einval
    assert lib.cgc_watershed_begin(None, None, 1, None, 0, 4, 4, 5, 7, None, None) == einval  # NULL pointers
    assert lib.cgc_watershed_parents(4, 4, 5, 7, 1, None, None) == einval
    assert lib.cgc_watershed_finish(4, 4, None, None, None, None) == einval
    for connectivity in (0, 3, -1):
        assert lib.cgc_watershed_rounds(4, 4, 5, 7, connectivity, None, 0, 8, None, None) == einval
        assert lib.cgc_watershed_parents(4, 4, 5, 7, connectivity, None, None) == einval
    assert lib.cgc_watershed_rounds(4, 4, 5, 7, 1, None, -1, 8, None, None) == einval
    assert lib.cgc_watershed_rounds(4, 4, 5, 7, 1, None, 0, 0, None, None) == einval
    assert lib.cgc_watershed_rounds(4, 4, 5, 7, 1, None, 2 ** 31 - 8, 8, None, None) == einval
    assert lib.cgc_watershed_rounds(4, 4, 5, 7, 1, None, 0, 8, None, None) == einval          # no counter
    assert lib.cgc_watershed_jumps(4, 4, None, 8, None, None) == einval                       # no counter
    one = ctypes.c_int(0)                                                                     # a counter, but no jump to make
    assert lib.cgc_watershed_jumps(4, 4, None, 0, ctypes.addressof(one), None) == einval
    assert lib.cgc_watershed_begin(None, None, 1, None, 0, 0, 7, 5, 7, None, None) == 0       # an empty image: nothing to do
    assert lib.cgc_watershed_parents(0, 7, 5, 7, 2, None, None) == 0
    assert lib.cgc_watershed_finish(7, 0, None, None, None, None) == 0
    assert lib.cgc_abi_version() == _abi.ABI_VERSION >= 14
