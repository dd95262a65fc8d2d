"""CPU: the host side of superpixels (csrc/slic.hip; cgc_net_amd.nuclei.superpixels, superpixel_graph, superpixel_features,
regions_at; kernels.HipKernels.slic_iterate, slic_merge, slic_relabel): what is refused before any launch, what the library refuses
without launching, the ABI and the documents.

As in tests/test_outline_host_cpu.py the "on the GPU" refusal is lifted and the kernel table fails the test when it is asked for."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import _abi, kernels, nuclei

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('cgc_slic_max_step', 'cgc_slic_tile_side', 'cgc_slic_table_side', 'cgc_slic_ws_bytes', 'cgc_slic_iterate',
           'cgc_slic_merge_begin', 'cgc_slic_merge_rounds', 'cgc_slic_relabel')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    lib = ctypes.CDLL(kernels.lib_path())
    _abi.declare(lib)
    return lib


@pytest.fixture
def no_launch(monkeypatch):
    check = nuclei._check_image

    def lifted(fn, name, image, dtypes=None, on_gpu=True):
        return check(fn, name, image, on_gpu=False) if dtypes is None else check(fn, name, image, dtypes, on_gpu=False)

    def refuse():
        pytest.fail('a launch was reached')

    monkeypatch.setattr(nuclei, '_check_image', lifted)
    monkeypatch.setattr(kernels, 'get', refuse)


def planes(C=1, H=12, W=14, dtype=torch.uint8):
    return torch.zeros(C, H, W, dtype=dtype)


def view(C, H, W):
    """Planes of any size without memory behind them."""
    return torch.zeros(1, 1, 1, dtype=torch.uint8).expand(C, H, W)


# ------------------------------------------------------------------ the public functions
def test_only_tensors_on_the_gpu():
    for bad in (planes(), np.zeros((1, 12, 14), np.uint8), None, [[[1]]]):
        with pytest.raises(TypeError):
            nuclei.superpixels(bad, 8)


def test_form_of_the_planes(no_launch):
    f = nuclei.superpixels
    for dtype in (torch.bool, torch.int8, torch.int16, torch.int32, torch.int64, torch.float32):
        with pytest.raises(TypeError, match='uint8'):
            f(planes(dtype=dtype), 8)
    for shape in ((12, 14), (1, 1, 12, 14), (12,)):
        with pytest.raises(ValueError):
            f(torch.zeros(shape, dtype=torch.uint8), 8)
    for C in (0, 5, 7):
        with pytest.raises(ValueError, match='1 <= C <= 4'):
            f(planes(C), 8)
    for H, W in ((2 ** 15, 2 ** 14), (2 ** 29, 1), (1, 2 ** 29), (23171, 23171)):
        assert H * W >= 2 ** 29
        with pytest.raises(ValueError, match=r'fewer than 2\^29 pixels'):
            f(view(1, H, W), 8)
    assert nuclei.SLIC_MAX_PIXELS == 2 ** 29


def test_parameters(no_launch):
    f = nuclei.superpixels
    for bad in (3, 257, 0, -8, 8.0, '8', None, True):
        with pytest.raises(ValueError, match='step must be an integer in 4..256'):
            f(planes(), bad)
    for bad in (-1, 1025, 10.0, None, True):
        with pytest.raises(ValueError, match='compactness must be an integer in 0..1024'):
            f(planes(), 8, bad)
    for bad in (0, 65, -1, 2.0, None, False):
        with pytest.raises(ValueError, match='n_iter must be an integer in 1..64'):
            f(planes(), 8, 10, bad)
    for bad in (-1, 2 ** 31, 1.5, '4', True):
        with pytest.raises(ValueError, match='min_size'):
            f(planes(), 8, min_size=bad)
    assert (nuclei.SLIC_MIN_STEP, nuclei.SLIC_MAX_STEP, nuclei.SLIC_MAX_PLANES) == (4, 256, 4)


def test_within(no_launch):
    f = nuclei.superpixels
    for shape in ((14, 12), (12, 15), (1, 12, 14), (12 * 14,)):
        with pytest.raises(ValueError):
            f(planes(), 8, within=torch.ones(shape, dtype=torch.uint8))
    with pytest.raises(ValueError, match='device'):
        f(planes(), 8, within=torch.ones(12, 14, dtype=torch.uint8, device='meta'))
    for dtype in (torch.float32, torch.float64):
        with pytest.raises(TypeError):
            f(planes(), 8, within=torch.ones(12, 14, dtype=dtype))
    with pytest.raises(TypeError):
        f(planes(), 8, within=np.ones((12, 14), np.uint8))


def test_an_empty_image_gives_empty_outputs_without_a_launch(no_launch):
    for C, H, W in ((1, 0, 5), (3, 7, 0), (4, 0, 0)):
        labels, n = nuclei.superpixels(planes(C, H, W), 8)
        assert tuple(labels.shape) == (H, W) and labels.dtype == torch.int32 and n == 0
        labels, n, (centres, count) = nuclei.superpixels(planes(C, H, W), 8, within=torch.ones(H, W, dtype=torch.bool), return_centres=True)
        assert tuple(labels.shape) == (H, W) and n == 0
        assert tuple(centres.shape) == (0, 2 + C) and centres.dtype == torch.int32 and tuple(count.shape) == (0,) and count.dtype == torch.int32
    with pytest.raises(ValueError):                                  # the refusals come first
        nuclei.superpixels(planes(1, 0, 5), 3)


def test_graph_and_feature_arguments(no_launch):
    labels = torch.ones(12, 14, dtype=torch.int32)
    for f in (lambda n: nuclei.superpixel_graph(labels, n), lambda n: nuclei.superpixel_features(labels, planes(), n)):
        for bad in (-1, 2 ** 31 - 1, 1.0, None, True):
            with pytest.raises(ValueError, match='n must be an integer'):
                f(bad)
    with pytest.raises(TypeError):
        nuclei.superpixel_graph(labels.to(torch.int64), 1)
    with pytest.raises(TypeError):
        nuclei.superpixel_features(labels, planes(dtype=torch.int16), 1)
    for bad in (planes(1, 12, 15), planes(5), torch.zeros(12, 14, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            nuclei.superpixel_features(labels, bad, 1)


class Untouchable(object):
    """Stands in for a tensor: any use but its shape fails the test."""
    shape = (1, 12, 14)

    def __getattr__(self, name):
        pytest.fail('a tensor was touched (%s)' % name)


def test_the_kernel_table_refuses_bad_parameters_before_any_tensor():
    call = kernels.HipKernels.slic_iterate
    U = Untouchable()
    for args in ((3, 10, 10), (257, 10, 10), (8, -1, 10), (8, 1025, 10), (8, 10, 0), (8, 10, 65), (True, 10, 10), (8.0, 10, 10)):
        with pytest.raises(ValueError, match='must be an integer in'):
            call(None, U, *args)
    for shape in ((0, 12, 14), (5, 12, 14), (12, 14)):
        bad = Untouchable()
        bad.shape = shape
        with pytest.raises(ValueError, match='1 <= C <= 4'):
            call(None, bad, 8, 10, 10)
    bad = Untouchable()
    bad.shape = (1, 2 ** 15, 2 ** 14)
    with pytest.raises(ValueError, match=r'2\^29'):
        call(None, bad, 8, 10, 10)
    for bad in (-1, 2 ** 31, 1.0, True):
        with pytest.raises(ValueError, match='min_size'):
            kernels.HipKernels.slic_merge(None, U, U, U, bad)
    for within in (torch.ones(14, 12, dtype=torch.uint8), torch.ones(12, 15, dtype=torch.uint8), torch.ones(1, 12, 14, dtype=torch.uint8),
                   torch.ones(12, 14, dtype=torch.uint8, device='meta')):
        with pytest.raises(ValueError, match='within must have the shape and device'):      # before the "on the GPU" refusal
            call(None, torch.zeros(1, 12, 14, dtype=torch.uint8), 8, 10, 10, within)
    assert kernels.HipKernels.slic_grid(37, 53, 8) == (5, 7) and kernels.HipKernels.slic_grid(9, 9, 8) == (1, 1)
    assert kernels.HipKernels.slic_grid(5, 40, 8) == (1, 5) and kernels.HipKernels.slic_grid(3, 3, 256) == (1, 1)


def test_signatures_and_documents():
    p = inspect.signature(nuclei.superpixels).parameters
    assert list(p) == ['planes', 'step', 'compactness', 'n_iter', 'min_size', 'within', 'return_centres']
    assert [p[k].default for k in list(p)[2:]] == [10, 10, None, None, False]
    p = inspect.signature(nuclei.superpixel_graph).parameters
    assert list(p) == ['labels', 'n', 'loop', 'return_attr'] and p['loop'].default is True and p['return_attr'].default is False
    assert list(inspect.signature(nuclei.superpixel_features).parameters) == ['labels', 'planes', 'n']
    assert list(inspect.signature(nuclei.regions_at).parameters) == ['labels', 'points']
    for f in (nuclei.superpixels, nuclei.superpixel_graph, nuclei.superpixel_features, nuclei.regions_at):
        assert 'Host syncs: ' in f.__doc__, f.__name__
    assert nuclei.SUPERPIXEL_FEATURE_NAMES[:5] == ('area', 'centroid_y', 'centroid_x', 'plane0_mean', 'plane0_std')
    assert len(nuclei.SUPERPIXEL_FEATURE_NAMES) == 3 + 2 * nuclei.SLIC_MAX_PLANES
    spec = kernels.KernelSpec.slic_iterate.__doc__
    for text in ('(2 H + S) // (2 S)', 'y * ny // H', '((2 i + 1) H) // (2 ny)', 'computed in 64 bits', 'the smallest k',
                 '(2 * sum + n) // (2 * n)', 'n == 0 keeps', 'CGC_EINVAL', 'no host read', 'bit-identical'):
        assert text in spec, text
    for text in ('count << 32 | ~q', 'BEFORE round r', 'smallest q'):
        assert text in kernels.KernelSpec.slic_merge.__doc__, text
    for name in ('slic_iterate', 'slic_merge', 'slic_relabel'):
        assert name in kernels.KernelSpec.__dict__ and name in kernels.HipKernels.__dict__
    read = lambda name: open(os.path.join(ROOT, name)).read()
    assert re.search(r'^\| F23 .*$', read('SURVEY.md'), flags=re.M)
    assert re.search(r'^#+ .*Superpixels', read('DESIGN.md'), flags=re.M)
    assert 'superpixels' in read('README.md') and 'superpixels' in read('INTEGRATION.md')
    assert os.path.exists(os.path.join(ROOT, 'tools', 'slic_bench.py'))


# ------------------------------------------------------------------ the library
def test_library_refusals(lib):
    einval = -1
    buf = (ctypes.c_int64 * 64)()
    some = ctypes.addressof(buf)

    def iterate(planes=some, C=1, H=12, W=14, step=8, m=10, n_iter=2, within=None, wbytes=0, ws=some, labels=some, centres=some,
                count=some):
        return lib.cgc_slic_iterate(planes, C, H, W, step, m, n_iter, within, wbytes, ws, labels, centres, count, None)

    for C in (0, 5, -1):
        assert iterate(C=C) == einval and lib.cgc_slic_ws_bytes(C, 12, 14, 8) == 0
    for step in (3, 257, 0, -4):
        assert iterate(step=step) == einval and lib.cgc_slic_ws_bytes(1, 12, 14, step) == 0
    for H, W in ((2 ** 15, 2 ** 14), (2 ** 29, 1), (-1, 5), (4, -1), (2 ** 30, 4)):
        assert iterate(H=H, W=W) == einval and lib.cgc_slic_ws_bytes(1, H, W, 8) == 0, (H, W)
    for m in (-1, 1025):
        assert iterate(m=m) == einval
    for n_iter in (0, 65, -1):
        assert iterate(n_iter=n_iter) == einval
    for wbytes in (0, 3, 16, -1):
        assert iterate(within=some, wbytes=wbytes) == einval
    for name in ('planes', 'ws', 'labels', 'centres', 'count'):
        assert iterate(**{name: None}) == einval, name
    assert iterate(H=0, planes=None, ws=None, labels=None, centres=None, count=None) == 0       # nothing to do
    assert iterate(W=0, planes=None, ws=None, labels=None, centres=None, count=None) == 0

    assert lib.cgc_slic_merge_begin(some, -1, 4, some, some, None) == einval
    assert lib.cgc_slic_merge_begin(some, 3, -1, some, some, None) == einval
    assert lib.cgc_slic_merge_begin(None, 3, 4, some, some, None) == einval
    assert lib.cgc_slic_merge_begin(some, 3, 4, None, some, None) == einval
    assert lib.cgc_slic_merge_begin(some, 3, 4, some, None, None) == einval
    for args in ((-1, 3, 2), (2 ** 31, 3, 2), (5, -1, 2), (5, 3, 0), (5, 3, -1), (5, 3, 4097)):
        assert lib.cgc_slic_merge_rounds(some, some, args[0], args[1], args[2], some, some, some, None) == einval, args
    assert lib.cgc_slic_merge_rounds(some, some, 5, 3, 2, some, some, None, None) == einval
    assert lib.cgc_slic_merge_rounds(None, some, 5, 3, 2, some, some, some, None) == einval
    assert lib.cgc_slic_merge_rounds(some, None, 5, 3, 2, some, some, some, None) == einval
    assert lib.cgc_slic_merge_rounds(some, some, 5, 3, 2, None, some, some, None) == einval
    assert lib.cgc_slic_merge_rounds(some, some, 5, 3, 2, some, None, some, None) == einval
    for n in (-1, 2 ** 31):
        assert lib.cgc_slic_relabel(some, n, 3, some, some, None) == einval
    assert lib.cgc_slic_relabel(some, 20, -1, some, some, None) == einval
    assert lib.cgc_slic_relabel(None, 20, 3, some, some, None) == einval
    assert lib.cgc_slic_relabel(some, 20, 3, None, some, None) == einval
    assert lib.cgc_slic_relabel(some, 20, 3, some, None, None) == einval
    assert lib.cgc_slic_relabel(None, 0, 3, None, None, None) == 0


def test_constants_and_workspace(lib):
    assert lib.cgc_slic_max_step() == kernels.SLIC_MAX_STEP == 256
    assert lib.cgc_slic_tile_side() == lib.cgc_region_tile_side() == 64
    table = lib.cgc_slic_table_side()
    assert table == 64 // 8 + 4                                       # every cell a tile meets, from cells of 8 pixels up
    for C, H, W, S in ((1, 9, 9, 8), (4, 37, 53, 8), (3, 3584, 3584, 16), (2, 5, 40, 4), (1, 1, 2 ** 29 - 1, 4)):
        ny, nx = kernels.HipKernels.slic_grid(H, W, S)
        assert lib.cgc_slic_ws_bytes(C, H, W, S) >= 8 * ny * nx * (3 + C)
    source = open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'slic.hip')).read()
    assert 'image_common.hpp' in source and 'image_nonzero(' in source and 'Carver' in source and 'layout_bytes(' in source
    assert 'float' not in source and 'double' not in source           # integer work only
    assert 'slic.hip' in open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'Makefile')).read()


def test_abi_29_in_the_header_the_prototypes_and_the_library(lib):
    header = open(os.path.join(ROOT, 'include', 'cgc_hip.h')).read()
    assert lib.cgc_abi_version() == _abi.ABI_VERSION == int(re.search(r'#define CGC_ABI_VERSION (\d+)', header).group(1)) >= 29
    assert re.search(r'^ \*  29: superpixels', header, flags=re.M) and re.search(r'^/\* ---- F23 ', header, flags=re.M)
    for name in SYMBOLS:
        assert name in _abi.PROTOTYPES and re.search(r'^(int|int64_t) %s\(' % name, header, flags=re.M), name
        assert getattr(lib, name).argtypes == _abi.PROTOTYPES[name]
        declared = re.search(r'^(?:int|int64_t) %s\(([^;]*)\);' % name, header, flags=re.M).group(1)
        assert len([a for a in declared.split(',') if a.strip() != 'void']) == len(_abi.PROTOTYPES[name]), name
    assert lib.cgc_slic_ws_bytes.restype == ctypes.c_int64
