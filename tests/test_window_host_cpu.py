"""CPU: the host side of window sums and local thresholds (csrc/window.hip; cgc_net_amd.nuclei.window_sums, niblack_k64,
local_threshold, local_stain_foreground, kernels.HipKernels.window_sums / local_threshold): what the public functions refuse before
any launch, and what the library refuses without launching.

As in tests/test_adjacency_host_cpu.py the tests lift the "on the GPU" refusal (``on_gpu=False``) and replace the kernel table by one
that fails the test when it is asked for: every refusal checked here is raised before any launch."""
import ctypes
import decimal
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import _abi, kernels, nuclei

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def image(*shape, dtype=torch.uint8):
    return torch.ones(shape or (4, 5), dtype=dtype)


def tile(*shape):
    return torch.ones(shape or (4, 5, 3), dtype=torch.uint8)


def gray_calls():
    return (lambda im, **kw: nuclei.window_sums(im, kw.pop('radius', 2), **kw),
            lambda im, **kw: nuclei.local_threshold(im, kw.pop('radius', 2), **kw))


# ------------------------------------------------------------------ the public functions
def test_only_tensors_on_the_gpu():
    for fn in gray_calls():
        for bad in (image(), np.ones((4, 5), np.uint8), None, [[1, 2]]):
            with pytest.raises(TypeError):
                fn(bad)
    for bad in (tile(), np.ones((4, 5, 3), np.uint8), None):
        with pytest.raises(TypeError):
            nuclei.local_stain_foreground(bad, 20)


def test_form_of_the_image(no_launch):
    for fn in gray_calls():
        for dtype in (torch.bool, torch.int8, torch.int16, torch.int32, torch.int64, torch.float32, torch.float16):
            with pytest.raises(TypeError):
                fn(image(dtype=dtype))
        for shape in ((3, 4, 5), (5,), (1, 4, 5)):
            with pytest.raises(ValueError):
                fn(image(*shape))
    for shape in ((4, 5), (4, 5, 4), (4, 5, 1), (2, 4, 5, 3)):
        with pytest.raises(ValueError):
            nuclei.local_stain_foreground(tile(*shape), 20)
    with pytest.raises(TypeError):
        nuclei.local_stain_foreground(torch.ones(4, 5, 3, dtype=torch.int32), 20)


def test_form_of_within(no_launch):
    calls = gray_calls() + (lambda im, **kw: nuclei.local_stain_foreground(tile(), 20, **kw),)
    for fn in calls:
        for other in (image(5, 4), image(4, 6), image(4, 5, 1), image(20)):
            with pytest.raises(ValueError):
                fn(image(), within=other)
        with pytest.raises(ValueError, match='device'):
            fn(image(), within=torch.zeros(4, 5, dtype=torch.uint8, device='meta'))
        for bad in (image(dtype=torch.float32), np.ones((4, 5), bool), 1):
            with pytest.raises(TypeError):
                fn(image(), within=bad)


def test_window_radius(no_launch):
    for bad in (-1, 128, 1000, 2.0, 2.5, None, '3', True, float('nan')):
        for fn in gray_calls():
            with pytest.raises(ValueError, match='radius'):
                fn(image(), radius=bad)
        with pytest.raises(ValueError, match='radius'):
            nuclei.local_stain_foreground(tile(), bad)
    for bad in (-1, 6, 2.0, None):                                      # the smoothing radius keeps its own range
        with pytest.raises(ValueError, match='radius'):
            nuclei.local_stain_foreground(tile(), 20, radius=bad)
    assert kernels.WINDOW_MAX_RADIUS == 127


def test_rule_parameters(no_launch):
    calls = (lambda **kw: nuclei.local_threshold(image(), 2, **kw), lambda **kw: nuclei.local_stain_foreground(tile(), 20, **kw))
    for fn in calls:
        for bad in (2.01, -2.01, 3, float('nan'), float('inf'), -float('inf'), True, None, '0.2', 1j, decimal.Decimal('0.2')):
            with pytest.raises(ValueError, match='k must'):
                fn(k=bad)
        for bad in (-256, 256, 1.0, 0.5, None, True, '1'):
            with pytest.raises(ValueError, match='offset'):
                fn(offset=bad)
        for bad in (-1, 256, 1.0, True, 'mean', ''):
            with pytest.raises(ValueError, match='floor'):
                fn(floor=bad)
    with pytest.raises(ValueError, match='floor'):
        nuclei.local_threshold(image(), 2, floor='otsu')                # only local_stain_foreground knows the plane's Otsu threshold
    for bad in (-1, 3, 1.5, None):
        with pytest.raises(ValueError):
            nuclei.local_stain_foreground(tile(), 20, stain=bad)
    with pytest.raises(ValueError, match='order'):
        nuclei.local_stain_foreground(tile(), 20, order='gbr')


def test_niblack_k64():
    want = {0: 0, 0.0: 0, 0.2: 13, -0.2: -13, 2: 128, -2: -128, 2.0: 128, 1: 64, 0.5: 32, 1 / 128: 1, -1 / 128: 0, 0.0078: 0,
            Fraction(1, 5): 13, Fraction(-3, 128): -1, 2.0078: 128, -2.0078125: -128, 0.2109375: 14, 0.21: 13}
    for k, k64 in want.items():
        assert nuclei.niblack_k64(k) == k64 and isinstance(nuclei.niblack_k64(k), int), k
    for k64 in range(-128, 129):
        assert nuclei.niblack_k64(k64 / 64) == k64
    for bad in (2.01, -2.01, 2.0079, 100, float('nan'), float('inf'), True, False, None, '1', 1j, [0.2]):
        with pytest.raises(ValueError):
            nuclei.niblack_k64(bad)


# ------------------------------------------------------------------ the kernel table
class Untouchable(object):
    """Stands in for a tensor: any use fails the test."""

    def __getattr__(self, name):
        pytest.fail('a tensor was touched (%s)' % name)


def test_the_kernel_table_refuses_bad_parameters_before_any_tensor():
    for bad in (-1, 128, None, 2.0, True):
        with pytest.raises(ValueError, match='radius'):
            kernels.HipKernels.window_sums(None, Untouchable(), bad)
        with pytest.raises(ValueError, match='radius'):
            kernels.HipKernels.local_threshold(None, Untouchable(), bad, 0, 0, -1)
    for k64, offset, floor, name in ((129, 0, -1, 'k64'), (-129, 0, -1, 'k64'), (0.2, 0, -1, 'k64'), (0, 256, -1, 'offset'),
                                     (0, -256, -1, 'offset'), (0, 0, -2, 'floor'), (0, 0, 256, 'floor'), (0, 0, None, 'floor')):
        with pytest.raises(ValueError, match=name):
            kernels.HipKernels.local_threshold(None, Untouchable(), 3, k64, offset, floor)


def test_signatures_and_documents():
    p = inspect.signature(nuclei.window_sums).parameters
    assert list(p) == ['image', 'radius', 'within'] and p['within'].default is None
    p = inspect.signature(nuclei.niblack_k64).parameters
    assert list(p) == ['k']
    p = inspect.signature(nuclei.local_threshold).parameters
    assert list(p) == ['image', 'radius', 'k', 'offset', 'floor', 'within']
    assert [p[k].default for k in list(p)[2:]] == [0.0, 0, None, None]
    p = inspect.signature(nuclei.local_stain_foreground).parameters
    assert list(p) == ['image', 'window', 'stain', 'radius', 'stains', 'order', 'within', 'k', 'offset', 'floor']
    assert [p[k].default for k in list(p)[2:]] == [0, 2, None, 'bgr', None, 0.0, 0, None]
    p = inspect.signature(nuclei.stain_foreground).parameters           # unchanged
    assert list(p) == ['image', 'stain', 'radius', 'stains', 'order', 'within']
    assert [p[k].default for k in list(p)[1:]] == [0, 2, None, 'bgr', None]
    for fn in (nuclei.window_sums, nuclei.local_threshold):
        assert 'Host syncs: none.' in fn.__doc__
    assert 'Host syncs: none; one' in nuclei.local_stain_foreground.__doc__
    for name, params in (('window_sums', ['self', 'image', 'radius', 'within']),
                         ('local_threshold', ['self', 'image', 'radius', 'k64', 'offset', 'floor', 'within'])):
        p = inspect.signature(getattr(kernels.KernelSpec, name)).parameters
        assert list(p) == params and p['within'].default is None
        assert list(inspect.signature(getattr(kernels.HipKernels, name)).parameters) == params
    doc = kernels.KernelSpec.window_sums.__doc__
    for k in range(1, 7):
        assert '\n        %d.  ' % k in doc, k
    assert 'CLIPPED' in doc and '4 228 250 625' in doc and 'wraps' in doc
    doc = kernels.KernelSpec.local_threshold.__doc__
    for k in range(1, 8):
        assert '\n        %d.  ' % k in doc, k
    for text in ('L = 64 (n v - S - c n)', 'D = n Q - S^2', '2^31.0', '2^62.0', '6.874e13', '1.13e18', 'Equality is not foreground'):
        assert text in doc, text
    with pytest.raises(NotImplementedError):
        kernels.KernelSpec().window_sums(None, 1)
    with pytest.raises(NotImplementedError):
        kernels.KernelSpec().local_threshold(None, 1, 0, 0, -1)
    for name in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, name)).read()
        assert 'local_threshold' in text or 'local_stain_foreground' in text, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '## Window sums and local thresholds (csrc/window.hip)' in design and 'window_bench.json' in design
    assert 'window.hip' in open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'Makefile')).read()
    assert os.path.exists(os.path.join(ROOT, 'profiles', 'window_bench.json'))


# ------------------------------------------------------------------ the library, without a launch
def test_library_refusals(lib):
    einval = -1
    out = (ctypes.c_int64 * 64)()                                       # any non-NULL address: nothing is launched
    some = ctypes.addressof(out)

    # cgc_window_sums(img, within, within_bytes, H, W, radius, n, s, q, stream)
    def sums(img=some, within=None, wbytes=0, H=4, W=5, radius=2, n=some, s=some, q=some):
        return lib.cgc_window_sums(img, within, wbytes, H, W, radius, n, s, q, None)

    # cgc_local_threshold(img, within, within_bytes, H, W, radius, k64, offset, floor, out, stream)
    def rule(img=some, within=None, wbytes=0, H=4, W=5, radius=2, k64=0, offset=0, floor=-1, out=some):
        return lib.cgc_local_threshold(img, within, wbytes, H, W, radius, k64, offset, floor, out, None)

    for fn in (sums, rule):
        for H, W in ((-1, 5), (4, -1), (-4, -5), (2 ** 16, 2 ** 15), (2 ** 31 - 1, 2), (46341, 46341)):
            assert fn(H=H, W=W) == einval
        for radius in (-1, 128, 255, 2 ** 20, -2 ** 31):
            assert fn(radius=radius) == einval
        for wbytes in (0, 3, 5, 16, -1):
            assert fn(within=some, wbytes=wbytes) == einval
        assert fn(img=None) == einval
        for H, W in ((0, 7), (7, 0), (0, 0)):                           # an empty image: nothing to do
            assert fn(H=H, W=W) == 0 and fn(H=H, W=W, img=None) == 0
            assert fn(H=H, W=W, radius=128) == einval                   # ... but still a refusal
    for name in ('n', 's', 'q'):
        assert sums(**{name: None}) == einval
    assert sums(H=0, n=None, s=None, q=None) == 0
    assert rule(out=None) == einval and rule(H=0, out=None) == 0
    for k64 in (-129, 129, 2 ** 20):
        assert rule(k64=k64) == einval and rule(k64=k64, H=0) == einval
    for offset in (-256, 256):
        assert rule(offset=offset) == einval
    for floor in (-2, 256):
        assert rule(floor=floor) == einval


def test_tile_geometry(lib):
    assert lib.cgc_window_max_radius() == 127 == kernels.WINDOW_MAX_RADIUS
    assert lib.cgc_window_tile_rows() == 16
    assert lib.cgc_window_strip_cols(0) == 1024 and lib.cgc_window_strip_cols(1) == 1016 == lib.cgc_window_strip_cols(4)
    assert lib.cgc_window_strip_cols(5) == 1008 and lib.cgc_window_strip_cols(127) == 768
    assert lib.cgc_window_strip_cols(-1) == 0 == lib.cgc_window_strip_cols(128)


def test_abi_19_in_the_header_the_prototypes_and_the_library(lib):
    header = open(os.path.join(ROOT, 'include', 'cgc_hip.h')).read()
    assert lib.cgc_abi_version() == _abi.ABI_VERSION == int(re.search(r'#define CGC_ABI_VERSION (\d+)', header).group(1)) >= 19
    assert re.search(r'^ \*  19: window sums', header, flags=re.M)
    for name in ('cgc_window_max_radius', 'cgc_window_tile_rows', 'cgc_window_strip_cols', 'cgc_window_sums', 'cgc_local_threshold'):
        assert name in _abi.PROTOTYPES and re.search(r'^int %s\(' % name, header, flags=re.M), name
        assert getattr(lib, name).argtypes == _abi.PROTOTYPES[name]
