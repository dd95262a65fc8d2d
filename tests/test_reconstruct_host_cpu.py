"""CPU: the host side of the morphological-reconstruction stage (csrc/reconstruct.hip; cgc_net_amd.nuclei.reconstruct, h_maxima,
regional_maxima, fill_holes, split_touching(markers='h_maxima')): what the public functions refuse before their first launch, the
integer helpers, the workspace size against its closed form, what the library refuses without launching, and split_touching's
untouched defaults.

The public functions only take tensors on the GPU, and say so first.  To reach the refusals behind that one without a GPU the tests
lift it (``on_gpu=False``) and replace the kernel table by one that fails the test when it is asked for: every refusal checked here
is raised before any launch."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import _abi, kernels, nuclei

FUNCTIONS = {
    'reconstruct': lambda t, **kw: nuclei.reconstruct(t, t, **kw),
    'h_maxima': lambda t, **kw: nuclei.h_maxima(t, kw.pop('h', 2), **kw),
    'regional_maxima': lambda t, **kw: nuclei.regional_maxima(t, **kw),
    'fill_holes': lambda t, **kw: nuclei.fill_holes(t, **kw),
}


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


@pytest.mark.parametrize('name', sorted(FUNCTIONS))
def test_only_tensors_on_the_gpu(name):
    fn = FUNCTIONS[name]
    for bad in (torch.zeros(4, 5, dtype=torch.uint8), np.zeros((4, 5), np.uint8), [[0, 1], [1, 0]], None):
        with pytest.raises(TypeError):
            fn(bad)
    with pytest.raises(TypeError):
        nuclei.split_touching(torch.zeros(4, 5, dtype=torch.uint8), None, growth='geodesic', markers='h_maxima', h=1)


@pytest.mark.parametrize('name', sorted(FUNCTIONS))
def test_dtypes_and_dimensions(name, no_launch):
    fn = FUNCTIONS[name]
    for dtype in (torch.int64, torch.float32, torch.float64, torch.float16):
        with pytest.raises(TypeError):
            fn(torch.zeros(4, 5, dtype=dtype))
    for shape in ((5,), (2, 4, 5), ()):
        with pytest.raises(ValueError):
            fn(torch.zeros(shape, dtype=torch.int32))
    for bad in (0, 3, 4, '1', None, 1.5):
        with pytest.raises(ValueError):
            fn(torch.zeros(4, 5, dtype=torch.int16), connectivity=bad)


def test_reconstruct_refusals(no_launch):
    a, b = torch.zeros(4, 5, dtype=torch.int32), torch.zeros(5, 4, dtype=torch.int32)
    with pytest.raises(ValueError):
        nuclei.reconstruct(a, b)
    with pytest.raises(ValueError):
        nuclei.reconstruct(a, torch.zeros(4, 6, dtype=torch.uint8))
    with pytest.raises(TypeError):
        nuclei.reconstruct(a, a.to(torch.int64))                       # each argument is checked
    with pytest.raises(TypeError):
        nuclei.reconstruct(a.to(torch.int64), a)
    for bad in ('dilate', 'opening', None, 1):
        with pytest.raises(ValueError):
            nuclei.reconstruct(a, a, method=bad)
    for good in (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32):
        with pytest.raises(ValueError):                                 # the dtype passes, the method does not
            nuclei.reconstruct(a.to(good), a, method='bad')


def test_h_refusals(no_launch):
    t = torch.zeros(4, 5, dtype=torch.int32)
    for bad in (0, -1, 2 ** 31, 2 ** 40):
        with pytest.raises(ValueError):
            nuclei.h_maxima(t, bad)
    for bad in (1.0, 2.5, '3', None):
        with pytest.raises(TypeError):
            nuclei.h_maxima(t, bad)
    assert nuclei._check_h(1) == 1 and nuclei._check_h(2 ** 31 - 1) == 2 ** 31 - 1 and nuclei._check_h(np.int32(7)) == 7


def test_split_touching_refusals(no_launch):
    m = torch.zeros(6, 7, dtype=torch.uint8)
    split = nuclei.split_touching
    with pytest.raises(ValueError):
        split(m, 2, markers='watershed')
    with pytest.raises(ValueError):
        split(m, 2, markers='h_maxima', h=1)                            # growth defaults to 'euclidean'
    with pytest.raises(ValueError):
        split(m, 2, growth='euclidean', markers='h_maxima', h=1)
    with pytest.raises(ValueError):
        split(m, 2, growth='geodesic', markers='h_maxima')              # h is required
    for bad in (0, 0.1, -1, float('nan')):
        with pytest.raises(ValueError):
            split(m, 2, growth='geodesic', markers='h_maxima', h=bad)   # h8 must be at least 1
    with pytest.raises(ValueError):
        split(m, 2, growth='geodesic', markers='h_maxima', h=1, connectivity=3)
    with pytest.raises(ValueError):
        split(m, 2, growth='geodesic', markers='h_maxima', h=1, min_size=-1)
    for growth in ('euclidean', 'geodesic'):
        with pytest.raises(ValueError):
            split(m, 2, growth=growth, h=1)                             # h without markers='h_maxima'
        with pytest.raises(ValueError):
            split(m, -1, growth=growth)                                 # 'core' still checks its radius


def test_split_touching_defaults_are_untouched():
    p = inspect.signature(nuclei.split_touching).parameters
    assert list(p) == ['mask', 'core_radius', 'connectivity', 'min_size', 'growth', 'markers', 'h']
    assert p['mask'].default is inspect.Parameter.empty and p['core_radius'].default is inspect.Parameter.empty
    assert (p['connectivity'].default, p['min_size'].default, p['growth'].default) == (1, 0, 'euclidean')
    assert (p['markers'].default, p['h'].default) == ('core', None)
    for name, want in (('reconstruct', {'method': 'dilation', 'connectivity': 1}), ('h_maxima', {'connectivity': 1}),
                       ('regional_maxima', {'connectivity': 1}), ('fill_holes', {'connectivity': 1})):
        q = inspect.signature(getattr(nuclei, name)).parameters
        assert {k: v.default for k, v in q.items() if v.default is not inspect.Parameter.empty} == want


def test_eighths_on_host_tensors():
    vals = [0, 1, 2, 3, 4, 24, 25, 26, 99, 100, 10 ** 6 - 1, 10 ** 6, 2 ** 31 - 2, 2 ** 31 - 1] + list(range(5000, 5400))
    t = nuclei._eighths(torch.tensor(vals, dtype=torch.int32))
    assert t.dtype == torch.int32 and t.tolist() == [math.isqrt(64 * v) for v in vals]


def test_the_cpu_twin_has_no_reconstruction():
    with pytest.raises(NotImplementedError):
        kernels.KernelSpec().morph_reconstruct(None, None, 1)


# ------------------------------------------------------------------ the library, without a launch
def a(x):
    return (x + 255) // 256 * 256


def cdiv(x, y):
    return -(-x // y)


@pytest.mark.parametrize('H,W', [(1, 1), (1, 37), (41, 1), (7, 5), (64, 64), (65, 63), (64, 65), (129, 257), (300, 300), (3, 2100),
                                 (0, 5), (4, 0)])
def test_workspace_size(lib, H, W):
    assert lib.cgc_reconstruct_ws_bytes(H, W) == 2 * a(4 * H * W) + a(4 * cdiv(H, 64) * cdiv(W, 64))


def test_library_refusals(lib):
    einval = -1
    for H, W in ((65536, 32768), (32768, 65536), (2 ** 31 - 1, 2), (-1, 4), (4, -1)):
        assert lib.cgc_reconstruct_ws_bytes(H, W) == 0
        assert lib.cgc_reconstruct_begin(None, None, H, W, 0, None, None) == einval
        assert lib.cgc_reconstruct_rounds(H, W, 1, None, 0, 8, None, None) == einval
        assert lib.cgc_reconstruct_finish(H, W, 0, None, None, None) == einval
    assert lib.cgc_reconstruct_ws_bytes(46340, 46340) > 0                                    # just below 2^31
    assert lib.cgc_reconstruct_begin(None, None, 4, 4, 0, None, None) == einval             # NULL pointers
    assert lib.cgc_reconstruct_finish(4, 4, 0, None, None, None) == einval
    for connectivity in (0, 3, -1):
        assert lib.cgc_reconstruct_rounds(4, 4, connectivity, None, 0, 8, None, None) == einval
    assert lib.cgc_reconstruct_rounds(4, 4, 1, None, -1, 8, None, None) == einval
    assert lib.cgc_reconstruct_rounds(4, 4, 1, None, 0, 0, None, None) == einval
    assert lib.cgc_reconstruct_rounds(4, 4, 1, None, 2 ** 31 - 8, 8, None, None) == einval
    assert lib.cgc_reconstruct_rounds(4, 4, 1, None, 0, 8, None, None) == einval             # no counter
    assert lib.cgc_reconstruct_begin(None, None, 0, 7, 0, None, None) == 0                   # an empty image: nothing to do
    assert lib.cgc_reconstruct_finish(0, 7, 1, None, None, None) == 0
    assert lib.cgc_abi_version() == _abi.ABI_VERSION >= 13
