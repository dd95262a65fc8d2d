"""CPU: the host side of the stain front end (csrc/stain.hip, csrc/smooth.hip; cgc_net_amd.nuclei.separate_stains, histogram,
otsu_threshold, smooth, stain_foreground): what the public functions refuse before their first launch and what the library refuses
without launching.

As in tests/test_watershed_host_cpu.py the tests lift the "on the GPU" refusal (``on_gpu=False``) and replace the kernel table by one
that fails the test when it is asked for: every refusal checked here is raised before any launch."""
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


def tile(*shape, dtype=torch.uint8):
    return torch.zeros(shape or (4, 5, 3), dtype=dtype)


def plane(*shape, dtype=torch.uint8):
    return torch.zeros(shape or (4, 5), dtype=dtype)


def test_only_tensors_on_the_gpu():
    for bad in (tile(), np.zeros((4, 5, 3), np.uint8), None):
        with pytest.raises(TypeError):
            nuclei.separate_stains(bad)
        with pytest.raises(TypeError):
            nuclei.stain_foreground(bad)
    for bad in (plane(), np.zeros((4, 5), np.uint8), [[0, 1], [1, 0]], None):
        with pytest.raises(TypeError):
            nuclei.histogram(bad)
        with pytest.raises(TypeError):
            nuclei.otsu_threshold(bad)
        with pytest.raises(TypeError):
            nuclei.smooth(bad, 1)


def test_dtypes_and_dimensions(no_launch):
    for dtype in (torch.bool, torch.int8, torch.int16, torch.int32, torch.int64, torch.float32, torch.float16):
        with pytest.raises(TypeError):
            nuclei.separate_stains(tile(dtype=dtype))
        with pytest.raises(TypeError):
            nuclei.stain_foreground(tile(dtype=dtype))
        with pytest.raises(TypeError):
            nuclei.histogram(plane(dtype=dtype))
        with pytest.raises(TypeError):
            nuclei.otsu_threshold(plane(dtype=dtype))
        with pytest.raises(TypeError):
            nuclei.smooth(plane(dtype=dtype), 1)
    for shape in ((4, 5), (4, 5, 1), (4, 5, 4), (3, 4, 5), (2, 4, 5, 3), (3,)):
        with pytest.raises(ValueError):
            nuclei.separate_stains(tile(*shape))
        with pytest.raises(ValueError):
            nuclei.stain_foreground(tile(*shape))
    for shape in ((5,), (4, 5, 3), (1, 4, 5)):
        with pytest.raises(ValueError):
            nuclei.histogram(plane(*shape))
        with pytest.raises(ValueError):
            nuclei.otsu_threshold(plane(*shape))
        with pytest.raises(ValueError):
            nuclei.smooth(plane(*shape), 1)


def test_order_planes_radius(no_launch):
    for bad in ('BGR', 'gbr', 0, 1, None, ('b', 'g', 'r')):
        with pytest.raises(ValueError, match='order'):
            nuclei.separate_stains(tile(), order=bad)
        with pytest.raises(ValueError, match='order'):
            nuclei.stain_foreground(tile(), order=bad)
    for bad in ((), (3,), (-1,), (0, 0), (1, 0), (0, 1, 2, 2), (0.5,), ('0',), 1, None, (0, 1, 2, 3)):
        with pytest.raises(ValueError, match='planes'):
            nuclei.separate_stains(tile(), planes=bad)
    for bad in (3, -1, 0.5, '0', None, (0,), (0, 1)):
        with pytest.raises(ValueError):
            nuclei.stain_foreground(tile(), stain=bad)
    for bad in (-1, 6, 100, 1.5, '1', None):
        with pytest.raises(ValueError, match='radius'):
            nuclei.smooth(plane(), bad)
        with pytest.raises(ValueError, match='radius'):
            nuclei.stain_foreground(tile(), radius=bad)


def test_within(no_launch):
    for fn in (nuclei.histogram, nuclei.otsu_threshold):
        for other in (plane(5, 4), plane(4, 6), plane(4, 5, 1)):
            with pytest.raises(ValueError):
                fn(plane(), within=other)
        for dtype in (torch.float32, torch.float16):
            with pytest.raises(TypeError):
                fn(plane(), within=plane(dtype=dtype))
        with pytest.raises(TypeError):
            fn(plane(), within=np.ones((4, 5), bool))
        with pytest.raises(ValueError, match='device'):
            fn(plane(), within=torch.zeros(4, 5, dtype=torch.uint8, device='meta'))
    with pytest.raises(ValueError):
        nuclei.stain_foreground(tile(), within=plane(5, 4))
    with pytest.raises(TypeError):
        nuclei.stain_foreground(tile(), within=plane(dtype=torch.float32))
    with pytest.raises(ValueError, match='device'):
        nuclei.stain_foreground(tile(), within=torch.zeros(4, 5, dtype=torch.bool, device='meta'))


def test_stain_matrix_refusals(no_launch):
    good = nuclei.DEFAULT_STAINS
    bad = [
        ((1, 0, 0), (0, 1, 0)),                                                   # shape
        (1, 2, 3),
        [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]],
        'hed',
        ((1, 0, 0), (0, 1, 0), (0, 0, float('nan'))),                            # non-finite
        ((1, 0, 0), (0, float('inf'), 0), (0, 0, 1)),
        ((1, 0, 0), (0, 0, 0), (0, 0, 1)),                                        # a zero row
        ((1, 2, 3), (2, 4, 6), (0, 0, 1)),                                        # singular: two parallel stains
        ((1, 0, 0), (0, 1, 0), (1, 1, 0)),                                        # singular: coplanar
        ((1, 0, 0), (0, 1, 0), (1, 1e-4, 1e-6)),                                  # invertible, but the int32 sum could overflow
    ]
    for stains in bad:
        with pytest.raises(ValueError):
            nuclei.stain_matrix(stains)
        with pytest.raises(ValueError):
            nuclei.separate_stains(tile(), stains=stains)
        with pytest.raises(ValueError):
            nuclei.stain_foreground(tile(), stains=stains)
    m = nuclei.stain_matrix(good)
    assert m.shape == (3, 3) and m.dtype == np.int32
    assert (np.abs(m.astype(np.int64)).sum(axis=0) * kernels.STAIN_OD_MAX < 2 ** 31 - 2 ** 15).all()
    eye = nuclei.stain_matrix(np.eye(3))
    assert eye.tolist() == [[4096, 0, 0], [0, 4096, 0], [0, 0, 4096]]


def test_the_kernel_table_refuses_before_any_copy():
    """HipKernels.stain_separate and binomial_smooth check their plain arguments before they touch a tensor."""
    check = kernels.HipKernels._check_stain_tables
    lut, m = list(nuclei.OD_LUT), nuclei.stain_matrix().tolist()
    assert check(0, lut, m, 7) == (lut, [v for row in m for v in row])
    for order in (2, -1, None, 'bgr'):
        with pytest.raises(ValueError):
            check(order, lut, m, 7)
    for planes in (0, 8, -1, None, 1.5):
        with pytest.raises(ValueError):
            check(0, lut, m, planes)
    for table in (lut[:255], lut + [0], [-1] + lut[1:], [kernels.STAIN_OD_MAX + 1] + lut[1:]):
        with pytest.raises(ValueError):
            check(0, table, m, 7)
    big = (2 ** 31 - 2 ** 15) // kernels.STAIN_OD_MAX                              # the first column sum that is refused
    with pytest.raises(ValueError):
        check(0, lut, [[big + 1, 0, 0], [0, 1, 0], [0, 0, 1]], 7)
    with pytest.raises(ValueError):
        check(0, lut, [[1, 0, 0], [0, 1, -big // 2 - 1], [0, 0, big // 2 + 1]], 7)
    check(0, lut, [[big, 0, 0], [0, -big, 0], [0, 0, big]], 7)
    for radius in (-1, 6, 1.5, None):
        with pytest.raises(ValueError):
            kernels.HipKernels.binomial_smooth(None, None, radius)


def test_signatures_and_documents():
    p = inspect.signature(nuclei.separate_stains).parameters
    assert list(p) == ['image', 'stains', 'order', 'planes'] and [p[k].default for k in list(p)[1:]] == [None, 'bgr', (0, 1, 2)]
    p = inspect.signature(nuclei.stain_foreground).parameters
    assert list(p) == ['image', 'stain', 'radius', 'stains', 'order', 'within']
    assert [p[k].default for k in list(p)[1:]] == [0, 2, None, 'bgr', None]
    assert list(inspect.signature(nuclei.histogram).parameters) == ['image', 'within']
    assert list(inspect.signature(nuclei.otsu_threshold).parameters) == ['image', 'within']
    assert list(inspect.signature(nuclei.smooth).parameters) == ['image', 'radius']
    for fn in (nuclei.separate_stains, nuclei.histogram, nuclei.otsu_threshold, nuclei.smooth, nuclei.stain_foreground):
        assert 'Host syncs' in fn.__doc__, fn.__name__
    assert 'split_touching(fill_holes(fg)' in nuclei.stain_foreground.__doc__ and 'nucleus_features(L' in nuclei.stain_foreground.__doc__
    assert 'stain_foreground' in nuclei.__doc__
    for name in ('stain_separate', 'histogram_u8', 'binomial_smooth'):
        assert getattr(kernels.KernelSpec, name).__doc__
        with pytest.raises(NotImplementedError):
            getattr(kernels.KernelSpec(), name)(*([None] * (len(inspect.signature(getattr(kernels.KernelSpec, name)).parameters) - 1)))
    assert len(nuclei.OD_LUT) == 256 and max(nuclei.OD_LUT) == kernels.STAIN_OD_MAX


# ------------------------------------------------------------------ the library, without a launch
def test_library_refusals(lib):
    einval = -1
    lut = (ctypes.c_int * 256)(*nuclei.OD_LUT)
    m = (ctypes.c_int * 9)(*[int(v) for v in nuclei.stain_matrix().reshape(-1)])
    # cgc_stain_separate(pix, npix, order, lut, m, planes, out, stream)
    for npix in (-1, 2 ** 31, 2 ** 40):
        assert lib.cgc_stain_separate(None, npix, 0, lut, m, 7, None, None) == einval
        assert lib.cgc_histogram_u8(None, npix, None, 0, None, None) == einval
    for order in (-1, 2, 3):
        assert lib.cgc_stain_separate(None, 4, order, lut, m, 7, None, None) == einval
    for planes in (0, 8, -1, 15):                                                  # empty, or a stain that does not exist
        assert lib.cgc_stain_separate(None, 4, 0, lut, m, planes, None, None) == einval
    assert lib.cgc_stain_separate(None, 4, 0, None, m, 7, None, None) == einval    # no tables
    assert lib.cgc_stain_separate(None, 4, 0, lut, None, 7, None, None) == einval
    for v, bad in ((0, -1), (0, kernels.STAIN_OD_MAX + 1), (255, 2 ** 30)):
        table = (ctypes.c_int * 256)(*nuclei.OD_LUT)
        table[v] = bad
        assert lib.cgc_stain_separate(None, 0, 0, table, m, 7, None, None) == einval
    big = (2 ** 31 - 2 ** 15) // kernels.STAIN_OD_MAX
    for matrix in ([big + 1, 0, 0, 0, 1, 0, 0, 0, 1], [1, 0, 0, 0, 1, -big // 2 - 1, 0, 0, big // 2 + 1], [-2 ** 31, 0, 0, 0, 1, 0, 0, 0, 1],
                   [2 ** 31 - 1] * 9):
        assert lib.cgc_stain_separate(None, 0, 0, lut, (ctypes.c_int * 9)(*matrix), 7, None, None) == einval
    assert lib.cgc_stain_separate(None, 0, 0, lut, (ctypes.c_int * 9)(big, 0, 0, 0, -big, 0, 0, 0, big), 7, None, None) == 0
    assert lib.cgc_stain_separate(None, 4, 0, lut, m, 7, None, None) == einval    # NULL images
    assert lib.cgc_stain_separate(None, 0, 1, lut, m, 5, None, None) == 0         # an empty image: nothing to do
    # cgc_histogram_u8(img, npix, within_or_null, within_bytes, hist, stream)
    some = ctypes.addressof(lut)                                                  # any non-NULL address: nothing is launched
    assert lib.cgc_histogram_u8(some, 4, None, 0, None, None) == einval           # no counts
    for bytes_ in (0, 3, 5, 16, -1):
        assert lib.cgc_histogram_u8(some, 4, some, bytes_, some, None) == einval
    assert lib.cgc_histogram_u8(None, 4, None, 0, some, None) == einval           # NULL image
    assert lib.cgc_histogram_chunk_pixels() >= 256 and lib.cgc_histogram_chunk_pixels() % 16 == 0
    # cgc_binomial_smooth_u8(img, H, W, radius, out, stream)
    for H, W in ((65536, 32768), (32768, 65536), (2 ** 31 - 1, 2), (-1, 4), (4, -1)):
        assert lib.cgc_binomial_smooth_u8(None, H, W, 1, None, None) == einval
    for radius in (-1, 6, 100, -2 ** 31):
        assert lib.cgc_binomial_smooth_u8(some, 4, 4, radius, some, None) == einval
    assert lib.cgc_binomial_smooth_u8(None, 4, 4, 1, None, None) == einval        # NULL images
    for radius in range(6):
        assert lib.cgc_binomial_smooth_u8(None, 0, 7, radius, None, None) == 0    # an empty image: nothing to do
        assert lib.cgc_binomial_smooth_u8(None, 7, 0, radius, None, None) == 0
    assert lib.cgc_abi_version() == _abi.ABI_VERSION >= 15
