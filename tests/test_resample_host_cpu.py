"""CPU: the host side of resampling (csrc/resample.hip; cgc_net_amd.nuclei.resize, resize_labels, rescale, rescale_labels,
scale_points; kernels.HipKernels.resample_u8, resample_labels): what the public functions refuse before any launch, the size rule,
the point map, and what the library refuses without launching.

As in tests/test_shape_host_cpu.py the tests lift the "on the GPU" refusal (``on_gpu=False``) and replace the kernel table by one
that fails the test when it is asked for: every refusal checked here is raised before any launch."""
import ctypes
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import _abi, kernels, nuclei

import resample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('cgc_resample_max_side', 'cgc_resample_labels_max_factor', 'cgc_resample_u8', 'cgc_resample_labels')


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


def view(*shape, dtype=torch.uint8):
    """An image of any size without memory behind it."""
    return torch.zeros((1,) * len(shape), dtype=dtype).expand(*shape)


# ------------------------------------------------------------------ the public functions
def test_only_tensors_on_the_gpu():
    for call in (lambda a: nuclei.resize(a, (4, 4)), lambda a: nuclei.resize_labels(a, (4, 4)), lambda a: nuclei.rescale(a, 2),
                 lambda a: nuclei.rescale_labels(a, 2)):
        for bad in (torch.ones(4, 5, dtype=torch.uint8), np.ones((4, 5), np.uint8), None, [[1, 2]]):
            with pytest.raises(TypeError):
                call(bad)


def test_form_of_the_image(no_launch):
    for dtype in (torch.bool, torch.int8, torch.int32, torch.float32):
        with pytest.raises(TypeError, match='image'):
            nuclei.resize(view(4, 5, dtype=dtype), (4, 5))
    for shape in ((20,), (4, 5, 1), (4, 5, 4), (3, 4, 5), (1, 4, 5, 3)):
        with pytest.raises(ValueError, match='image'):
            nuclei.resize(view(*shape), (4, 5))
    for dtype in (torch.float32, torch.float64):
        with pytest.raises(TypeError, match='labels'):
            nuclei.resize_labels(view(4, 5, dtype=dtype), (4, 5))
    for shape in ((20,), (4, 5, 3)):
        with pytest.raises(ValueError, match='labels'):
            nuclei.resize_labels(view(*shape, dtype=torch.int32), (4, 5))


@pytest.mark.parametrize('name', ['resize', 'resize_tile', 'resize_labels'])
def test_item_1_sides(no_launch, name):
    call, img = {'resize': (nuclei.resize, lambda H, W: view(H, W)), 'resize_tile': (nuclei.resize, lambda H, W: view(H, W, 3)),
                 'resize_labels': (nuclei.resize_labels, lambda H, W: view(H, W, dtype=torch.int32))}[name]
    for size in ((0, 5), (5, 0), (-1, 5), (32768, 5), (5, 32768), (2 ** 31, 2)):
        with pytest.raises(ValueError, match='size'):
            call(img(4, 5), size)
    for size in (5, (5,), (4, 5, 6), (4.0, 5), ('4', 5), None):
        with pytest.raises(ValueError, match='size'):
            call(img(4, 5), size)
    for H, W in ((0, 5), (5, 0), (0, 0)):
        with pytest.raises(ValueError, match='empty'):
            call(img(H, W), (4, 5))
    for H, W in ((32768, 2), (2, 32768)):
        with pytest.raises(ValueError, match='sides up to 32767'):
            call(img(H, W), (4, 5))
    for mode in ('bilinear', 'cubic', None, 0, 'majority' if name != 'resize_labels' else 'linear'):
        with pytest.raises(ValueError, match='mode'):
            call(img(4, 5), (4, 5), mode)
    kernels.HipKernels._check_resample('f', (32767, 32767), (32767, 1), 'linear', kernels.RESAMPLE_MODES)
    kernels.HipKernels._check_resample('f', (1, 1), (32767, 32767), 'nearest', kernels.RESAMPLE_LABEL_MODES)


def test_item_4_area_only_shrinks(no_launch):
    for size in ((5, 5), (4, 6), (8, 10)):
        with pytest.raises(ValueError, match="mode 'area' only shrinks"):
            nuclei.resize(view(4, 5), size, 'area')
        with pytest.raises(ValueError, match="mode 'area' only shrinks"):
            nuclei.resize(view(4, 5, 3), size, 'area')
    assert kernels.HipKernels._check_resample('f', (4, 5), (4, 5), 'area', kernels.RESAMPLE_MODES) == (4, 5, 1)
    assert kernels.HipKernels._check_resample('f', (4, 5), (1, 1), 'area', kernels.RESAMPLE_MODES) == (1, 1, 1)


def test_item_7_majority_shrinks_by_at_most_8(no_launch):
    lab = view(16, 24, dtype=torch.int32)
    for size in ((17, 24), (16, 25)):
        with pytest.raises(ValueError, match="mode 'majority' only shrinks"):
            nuclei.resize_labels(lab, size, 'majority')
    for size in ((1, 24), (16, 2), (1, 1)):
        with pytest.raises(ValueError, match="mode 'majority' shrinks by at most 8"):
            nuclei.resize_labels(lab, size, 'majority')
    assert kernels.HipKernels._check_resample('f', (16, 24), (2, 3), 'majority', kernels.RESAMPLE_LABEL_MODES) == (2, 3, 1)
    assert nuclei.RESAMPLE_LABELS_MAX_FACTOR == kernels.RESAMPLE_LABELS_MAX_FACTOR == 8


def test_rescale_size_rule(monkeypatch, no_launch):
    seen = []
    monkeypatch.setattr(nuclei, 'resize', lambda image, size, mode='linear': seen.append((size, mode)))
    monkeypatch.setattr(nuclei, 'resize_labels', lambda labels, size, mode='nearest': seen.append((size, mode)))
    nuclei.rescale(view(7, 5), Fraction(1, 2), 'area')                 # 3.5 and 2.5 round half up
    nuclei.rescale(view(7, 5, 3), 2)
    nuclei.rescale(view(15, 10), 0.1)                                   # the float's exact fraction: a shade above 1/10
    nuclei.rescale(view(15, 10), Fraction(1, 10))
    nuclei.rescale(view(3, 100), (Fraction(1, 100), 3))                 # clamped to side 1
    nuclei.rescale_labels(view(9, 9, dtype=torch.int64), (Fraction(2, 3), 0.5), 'majority')
    assert seen == [((4, 3), 'area'), ((14, 10), 'linear'), ((2, 1), 'linear'), ((2, 1), 'linear'), ((1, 300), 'linear'), ((6, 5), 'majority')]
    for n in (1, 2, 7, 15, 300):
        for f in (Fraction(1, 2), Fraction(1, 3), Fraction(7, 5), 0.1, 0.3, 2, 1e-9):
            assert nuclei._scaled_size((n, n), f) == (ref.scaled_side(n, f),) * 2
    for bad in ('2', None, True, [1, 2, 3], (1, None)):
        with pytest.raises(TypeError, match='factor'):
            nuclei.rescale(view(4, 5), bad)
    for bad in (0, -1, Fraction(-1, 2), 0.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='factor'):
            nuclei.rescale(view(4, 5), bad)


def test_scale_points():
    pts = torch.tensor([[0.0, 0.0], [1.5, 2.5], [3.0, 4.0]], dtype=torch.float64)
    got = nuclei.scale_points(pts, (4, 5), (8, 15))
    assert got.dtype == torch.float64 and got.tolist() == [[0.5, 1.0], [3.5, 8.5], [6.5, 13.0]]      # (c + 1/2) * n2 / n - 1/2
    # the image's corner (-1/2, -1/2) maps to the corner at any size
    assert nuclei.scale_points(torch.tensor([[-0.5, -0.5]]), (4, 5), (9, 3)).tolist() == [[-0.5, -0.5]]
    back = nuclei.scale_points(got, (8, 15), (4, 5))
    assert torch.allclose(back, pts, rtol=0, atol=1e-12)
    rnd = torch.rand(50, 2, dtype=torch.float64) * 300
    there = nuclei.scale_points(rnd, (300, 300), (137, 411))
    assert torch.allclose(nuclei.scale_points(there, (137, 411), (300, 300)), rnd, rtol=0, atol=1e-10)
    assert nuclei.scale_points(pts.float(), (4, 5), (8, 15)).dtype == torch.float32
    assert nuclei.scale_points(torch.zeros(0, 2), (4, 5), (8, 15)).shape == (0, 2)
    for bad in (pts.long(), [[1.0, 2.0]], None):
        with pytest.raises(TypeError, match='points'):
            nuclei.scale_points(bad, (4, 5), (8, 15))
    for bad in (torch.zeros(3), torch.zeros(3, 3)):
        with pytest.raises(ValueError, match='points'):
            nuclei.scale_points(bad, (4, 5), (8, 15))
    with pytest.raises(ValueError, match='from_size'):
        nuclei.scale_points(pts, (0, 5), (8, 15))
    with pytest.raises(ValueError, match='to_size'):
        nuclei.scale_points(pts, (4, 5), (8,))


# ------------------------------------------------------------------ the kernel table
class Untouchable(object):
    """Stands in for a tensor: any use but its shape fails the test."""
    shape = (4, 5)

    def __getattr__(self, name):
        pytest.fail('a tensor was touched (%s)' % name)


def test_the_kernel_table_refuses_bad_parameters_before_any_tensor():
    U = Untouchable()
    for call, modes in ((kernels.HipKernels.resample_u8, ('linear', 'area')), (kernels.HipKernels.resample_labels, ('nearest', 'majority'))):
        for mode in modes:
            for size in ((0, 5), (4, 32768), (4,), None):
                with pytest.raises(ValueError, match='size'):
                    call(None, U, size, mode)
            with pytest.raises(ValueError, match='only shrinks'):
                call(None, U, (5, 5), modes[1])
        with pytest.raises(ValueError, match='mode'):
            call(None, U, (4, 5), 'cubic')
    big = Untouchable()
    big.shape = (32768, 2)
    with pytest.raises(ValueError, match='32767'):
        kernels.HipKernels.resample_u8(None, big, (4, 5), 'linear')
    empty = Untouchable()
    empty.shape = (0, 7)
    with pytest.raises(ValueError, match='empty'):
        kernels.HipKernels.resample_labels(None, empty, (4, 5), 'nearest')


def test_signatures_and_documents():
    sig = {'resize': (['image', 'size', 'mode'], ['linear']), 'resize_labels': (['labels', 'size', 'mode'], ['nearest']),
           'rescale': (['image', 'factor', 'mode'], ['linear']), 'rescale_labels': (['labels', 'factor', 'mode'], ['nearest']),
           'scale_points': (['points', 'from_size', 'to_size'], [])}
    for name, (names, defaults) in sig.items():
        p = inspect.signature(getattr(nuclei, name)).parameters
        assert list(p) == names, name
        assert [p[k].default for k in names[len(names) - len(defaults):]] == defaults, name
        assert 'Host syncs: none' in getattr(nuclei, name).__doc__, name
    for cls in (kernels.KernelSpec, kernels.HipKernels):
        assert list(inspect.signature(cls.resample_u8).parameters) == ['self', 'image', 'size', 'mode']
        assert list(inspect.signature(cls.resample_labels).parameters) == ['self', 'labels', 'size', 'mode']
    doc = kernels.KernelSpec.resample_u8.__doc__
    for k in (1, 2, 3, 4, 5, 8):
        assert '\n        %d.  ' % k in doc, k
    doc = ' '.join(doc.split())
    for text in ('one launch', 'no host read', '32767', 'H * W = 0', 'half-integers', '((2 d + 1) n - m) / (2 m)', 'uint32', '2^31',
                 'floor((2 S + D) / (2 D))', 'D = 4 H2 W2', 'no prefiltering', '11-bit', 'min((d + 1) n, (i + 1) m) - max(d n, i m)',
                 'D = H W', 'independently', 'bit-identical', 'no atomics', 'no float arithmetic', 'equal copy'):
        assert text in doc, text
    doc = kernels.KernelSpec.resample_labels.__doc__
    for k in (1, 2, 6, 7, 8):
        assert '\n        %d.  ' % k in doc, k
    doc = ' '.join(doc.split())
    for text in ('floor((2 d + 1) n / (2 m))', 'np.repeat', 'H <= 8 H2 and W <= 8 W2', 'largest total weight', 'candidate like any other',
                 'smallest value', 'bool as 0 / 1', 'at most 9 pixels', 'bit-identical', 'equal copy'):
        assert text in doc, text
    for name in ('resample_u8', 'resample_labels'):
        with pytest.raises(NotImplementedError):
            getattr(kernels.KernelSpec(), name)(None, (1, 1), 'linear')
    line = "normalize_stains(rescale(tile, Fraction(1, 2), 'area'))"
    assert line in nuclei.__doc__ and 'nucleus_features(L, resize(gray, L.shape))' in nuclei.__doc__
    assert 'keeps its ``ValueError``' in nuclei.__doc__
    for name in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, name)).read()
        assert 'resize_labels' in text and 'scale_points' in text and 'rescale' in text, name
    for name in ('README.md', 'INTEGRATION.md'):
        assert line in open(os.path.join(ROOT, name)).read(), name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '## Resampling (csrc/resample.hip)' in design and 'resample_bench.json' in design
    assert os.path.exists(os.path.join(ROOT, 'tools', 'resample_bench.py'))


def test_nucleus_features_keeps_its_refusal(no_launch):
    with pytest.raises(ValueError):
        nuclei.nucleus_features(torch.ones(4, 5, dtype=torch.int32), torch.ones(8, 10, dtype=torch.uint8), max_label=1)


# ------------------------------------------------------------------ the library, without a launch
def test_library_refusals(lib):
    einval = -1
    buf = (ctypes.c_int64 * 64)()                                       # any non-NULL address: nothing is launched
    some = ctypes.addressof(buf)

    def u8(src=some, H=4, W=5, channels=1, H2=4, W2=5, mode=0, dst=some):
        return lib.cgc_resample_u8(src, H, W, channels, H2, W2, mode, dst, None)

    def lab(src=some, elem=4, H=16, W=24, H2=16, W2=24, mode=0, dst=some):
        return lib.cgc_resample_labels(src, elem, H, W, H2, W2, mode, dst, None)

    for call in (u8, lab):
        for name in ('H', 'W', 'H2', 'W2'):
            for bad in (0, -1, 32768, 2 ** 30):
                assert call(**{name: bad}) == einval, (name, bad)
        for name in ('src', 'dst'):
            assert call(**{name: None}) == einval, name
    for bad in (0, 2, 4, -1):
        assert u8(channels=bad) == einval
    for bad in (-1, 2, 3):
        assert u8(mode=bad) == einval
    for H2, W2 in ((5, 5), (4, 6)):
        assert u8(H2=H2, W2=W2, mode=1) == einval and u8(H2=H2, W2=W2, mode=1, channels=3) == einval
    for bad in (0, 3, 16, -1):
        assert lab(elem=bad) == einval
    for bad in (-1, 3, 4):
        assert lab(mode=bad) == einval
    for elem in (2, 4, 8):
        assert lab(elem=elem, mode=2) == einval                         # the unsigned order is that of one-byte values only
    for mode in (1, 2):
        elem = 1 if mode == 2 else 4
        for H2, W2 in ((17, 24), (16, 25), (1, 24), (16, 2)):
            assert lab(elem=elem, H2=H2, W2=W2, mode=mode) == einval, (mode, H2, W2)


def test_constants(lib):
    source = open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'resample.hip')).read()
    side = int(re.search(r'constexpr int RS_MAX_SIDE = (\d+);', source).group(1))
    factor = int(re.search(r'constexpr int RS_MAX_FACTOR = (\d+);', source).group(1))
    assert lib.cgc_resample_max_side() == side == kernels.RESAMPLE_MAX_SIDE == nuclei.RESAMPLE_MAX_SIDE == 32767
    assert lib.cgc_resample_labels_max_factor() == factor == kernels.RESAMPLE_LABELS_MAX_FACTOR == 8
    assert (2 * (side - 1) + 1) * side < 2 ** 32 and 2 * side * (side - 1) < 2 ** 31 and 255 * 4 * side * side < 2 ** 40
    assert kernels.RESAMPLE_MODES == {'linear': 0, 'area': 1} and kernels.RESAMPLE_LABEL_MODES == {'nearest': 0, 'majority': 1}
    header = open(os.path.join(ROOT, 'include', 'cgc_hip.h')).read()
    for name, value in (('LINEAR', 0), ('AREA', 1), ('NEAREST', 0), ('MAJORITY', 1), ('MAJORITY_UNSIGNED', 2)):
        assert re.search(r'^#define CGC_RESAMPLE_%s %d$' % (name, value), header, flags=re.M), name
    assert not re.search(r'atomic|float|double|for \(;;\)|while \(', source.split('#include <stdint.h>')[1])
    assert 'resample.hip' in open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'Makefile')).read()


def test_abi_27_in_the_header_the_prototypes_and_the_library(lib):
    header = open(os.path.join(ROOT, 'include', 'cgc_hip.h')).read()
    assert lib.cgc_abi_version() == _abi.ABI_VERSION == int(re.search(r'#define CGC_ABI_VERSION (\d+)', header).group(1)) >= 27
    assert re.search(r'^ \*  27: resampling', header, flags=re.M)
    order = [header.index('\nint %s(' % name) for name in SYMBOLS]
    assert order == sorted(order)
    names = list(_abi.PROTOTYPES)
    assert [names.index(name) for name in SYMBOLS] == list(range(names.index(SYMBOLS[0]), names.index(SYMBOLS[0]) + 4))
    assert names[names.index(SYMBOLS[0]) - 1] == 'cgc_region_hull'       # the header's order
    for name in SYMBOLS:
        assert getattr(lib, name).argtypes == _abi.PROTOTYPES[name]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _abi.PROTOTYPES['cgc_resample_u8'] == [P, I, I, I, I, I, I, P, P] == _abi.PROTOTYPES['cgc_resample_labels']
    assert 'resample_u8' in kernels.KernelSpec.__dict__ and 'resample_labels' in kernels.KernelSpec.__dict__
