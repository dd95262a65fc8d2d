"""CPU: the host side of flat morphology (csrc/morph.hip; cgc_net_amd.nuclei.erode, dilate, opening, closing, white_tophat,
black_tophat, morph_gradient, open_by_reconstruction, close_by_reconstruction; kernels.HipKernels.flat_morphology): what the public
functions refuse before any launch, and what the library refuses without launching.

As in tests/test_window_host_cpu.py the tests lift the "on the GPU" refusal (``on_gpu=False``) and replace the kernel table by one
that fails the test when it is asked for: every refusal checked here is raised before any launch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import _abi, kernels, nuclei

import morph_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = ('erode', 'dilate', 'opening', 'closing', 'white_tophat', 'black_tophat', 'morph_gradient')
BY_RECONSTRUCTION = ('open_by_reconstruction', 'close_by_reconstruction')
ALL = PLAIN + BY_RECONSTRUCTION


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


def calls():
    return [(name, (lambda im, _f=getattr(nuclei, name), **kw: _f(im, kw.pop('radius', 2), **kw))) for name in ALL]


# ------------------------------------------------------------------ the public functions
def test_only_tensors_on_the_gpu():
    for name, fn in calls():
        for bad in (image(), image(dtype=torch.bool), np.ones((4, 5), np.uint8), None, [[1, 2]]):
            with pytest.raises(TypeError):
                fn(bad)


def test_form_of_the_image(no_launch):
    for name, fn in calls():
        for dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.float32, torch.float16):     # int32 is out of scope
            with pytest.raises(TypeError):
                fn(image(dtype=dtype))
        for shape in ((3, 4, 5), (5,), (1, 4, 5)):
            with pytest.raises(ValueError):
                fn(image(*shape))
            with pytest.raises(ValueError):
                fn(image(*shape, dtype=torch.bool))
    assert 'int32 images are out of scope' in nuclei.erode.__doc__


def test_form_of_within(no_launch):
    for name, fn in calls():
        for other in (image(5, 4), image(4, 6), image(4, 5, 1), image(20)):
            with pytest.raises(ValueError):
                fn(image(), within=other)
        with pytest.raises(ValueError, match='device'):
            fn(image(), within=torch.zeros(4, 5, dtype=torch.uint8, device='meta'))
        for bad in (image(dtype=torch.float32), np.ones((4, 5), bool), 1):
            with pytest.raises(TypeError):
                fn(image(), within=bad)


def test_radius_and_footprint(no_launch):
    assert kernels.MORPH_MAX_RADIUS == nuclei.MORPH_MAX_RADIUS >= 63
    top = kernels.MORPH_MAX_RADIUS
    for name, fn in calls():
        for bad in (-1, top + 1, 1000, 2.0, 2.5, None, '3', True, float('nan')):
            with pytest.raises(ValueError, match='radius'):
                fn(image(), radius=bad)
        for bad in ('circle', 'Disk', '', None, 1, ('disk',), b'disk', ref.footprint('disk', 1)):
            with pytest.raises(ValueError, match='footprint'):
                fn(image(), footprint=bad)
    for name in BY_RECONSTRUCTION:
        for bad in (0, 3, None, 1.5):
            with pytest.raises(ValueError, match='connectivity'):
                getattr(nuclei, name)(image(), 2, connectivity=bad)
    assert set(nuclei.MORPH_FOOTPRINTS) == {'disk', 'square', 'diamond'} == set(kernels.MORPH_KINDS)


# ------------------------------------------------------------------ the kernel table
class Untouchable(object):
    """Stands in for a tensor: any use fails the test."""

    def __getattr__(self, name):
        pytest.fail('a tensor was touched (%s)' % name)


def test_the_kernel_table_refuses_bad_parameters_before_any_tensor():
    call = kernels.HipKernels.flat_morphology
    for bad in (-1, kernels.MORPH_MAX_RADIUS + 1, None, 2.0, True):
        with pytest.raises(ValueError, match='radius'):
            call(None, Untouchable(), 'disk', bad, 'erode')
    for bad in ('circle', 0, 1, None, 3):
        with pytest.raises(ValueError, match='kind'):
            call(None, Untouchable(), bad, 2, 'erode')
    for bad in ('open', 0, None, 'ERODE'):
        with pytest.raises(ValueError, match='op'):
            call(None, Untouchable(), 'disk', 2, bad)
    for bad in ('minus', 1, 0, 'plain'):
        with pytest.raises(ValueError, match='epilogue'):
            call(None, Untouchable(), 'disk', 2, 'erode', None, Untouchable(), bad)
    with pytest.raises(ValueError, match='together'):
        call(None, Untouchable(), 'disk', 2, 'erode', None, Untouchable(), None)
    with pytest.raises(ValueError, match='together'):
        call(None, Untouchable(), 'disk', 2, 'erode', None, None, 'other_minus')


def test_signatures_and_documents():
    for name in PLAIN:
        p = inspect.signature(getattr(nuclei, name)).parameters
        assert list(p) == ['image', 'radius', 'footprint', 'within'], name
        assert p['footprint'].default == 'disk' and p['within'].default is None and p['radius'].default is inspect.Parameter.empty
        assert 'Host syncs: none.' in getattr(nuclei, name).__doc__
    for name in BY_RECONSTRUCTION:
        p = inspect.signature(getattr(nuclei, name)).parameters
        assert list(p) == ['image', 'radius', 'footprint', 'connectivity', 'within'], name
        assert [p[k].default for k in list(p)[2:]] == ['disk', 1, None]
    # the stage functions keep their signatures and defaults
    p = inspect.signature(nuclei.stain_foreground).parameters
    assert list(p) == ['image', 'stain', 'radius', 'stains', 'order', 'within']
    assert [p[k].default for k in list(p)[1:]] == [0, 2, None, 'bgr', None]
    p = inspect.signature(nuclei.local_stain_foreground).parameters
    assert list(p) == ['image', 'window', 'stain', 'radius', 'stains', 'order', 'within', 'k', 'offset', 'floor']
    assert [p[k].default for k in list(p)[2:]] == [0, 2, None, 'bgr', None, 0.0, 0, None]
    p = inspect.signature(nuclei.split_touching).parameters
    assert list(p) == ['mask', 'core_radius', 'connectivity', 'min_size', 'growth', 'markers', 'h']
    assert [p[k].default for k in list(p)[2:]] == [1, 0, 'euclidean', 'core', None]
    params = ['self', 'image', 'kind', 'radius', 'op', 'within', 'other', 'epilogue']
    for cls in (kernels.KernelSpec, kernels.HipKernels):
        p = inspect.signature(cls.flat_morphology).parameters
        assert list(p) == params and all(p[k].default is None for k in params[5:])
    doc = kernels.KernelSpec.flat_morphology.__doc__
    for k in range(1, 9):
        assert '\n        %d.  ' % k in doc, k
    for text in ('F15', 'CLIPPED', 'w^2 + dy^2 <= r^2', 'neutral', 'other_minus', 'minus_other', 'H * W = 0', 'no host read',
                 'CGC_EINVAL', 'morph_tile_cols'):
        assert text in doc, text
    with pytest.raises(NotImplementedError):
        kernels.KernelSpec().flat_morphology(None, 'disk', 1, 'erode')
    for name in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, name)).read()
        assert 'white_tophat' in text and 'morph_gradient' in text, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '## Flat morphology (csrc/morph.hip)' in design and 'morph_bench.json' in design
    assert 'morph.hip' in open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'Makefile')).read()
    assert os.path.exists(os.path.join(ROOT, 'profiles', 'morph_bench.json'))
    assert os.path.exists(os.path.join(ROOT, 'tools', 'morph_bench.py'))
    assert 'watershed(morph_gradient(plane, 1), markers, within=fg)' in nuclei.__doc__


# ------------------------------------------------------------------ the library, without a launch
def test_library_refusals(lib):
    einval = -1
    out = (ctypes.c_int64 * 64)()                                       # any non-NULL address: nothing is launched
    some = ctypes.addressof(out)
    top = lib.cgc_morph_max_radius()

    # cgc_morph(img, within, within_bytes, H, W, kind, radius, op, other, epilogue, out, stream)
    def morph(img=some, within=None, wbytes=0, H=4, W=5, kind=1, radius=2, op=0, other=None, epilogue=0, out=some):
        return lib.cgc_morph(img, within, wbytes, H, W, kind, radius, op, other, epilogue, out, None)

    for H, W in ((-1, 5), (4, -1), (-4, -5), (2 ** 16, 2 ** 15), (2 ** 31 - 1, 2), (46341, 46341)):
        assert morph(H=H, W=W) == einval
    for radius in (-1, top + 1, 255, 2 ** 20, -2 ** 31):
        assert morph(radius=radius) == einval
    for kind in (-1, 3, 100):
        assert morph(kind=kind) == einval
    for op in (-1, 3, 100):
        assert morph(op=op) == einval
    for epilogue in (-1, 3):
        assert morph(epilogue=epilogue, other=some) == einval
    for epilogue in (1, 2):
        assert morph(epilogue=epilogue, other=None) == einval          # an epilogue needs its image
    for wbytes in (0, 3, 5, 16, -1):
        assert morph(within=some, wbytes=wbytes) == einval
    assert morph(img=None) == einval and morph(out=None) == einval
    for H, W in ((0, 7), (7, 0), (0, 0)):                               # an empty image: nothing to do
        assert morph(H=H, W=W) == 0 and morph(H=H, W=W, img=None, out=None) == 0
        assert morph(H=H, W=W, epilogue=1, other=None) == 0
        assert morph(H=H, W=W, radius=top + 1) == einval                # ... but still a refusal
        assert morph(H=H, W=W, kind=3) == einval and morph(H=H, W=W, op=3) == einval and morph(H=H, W=W, epilogue=3) == einval


def test_tile_geometry_and_constants(lib):
    source = open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'morph.hip')).read()
    header = open(os.path.join(ROOT, 'include', 'cgc_hip.h')).read()

    def constant(name):
        return int(re.search(r'constexpr int %s = (\d+);' % name, source).group(1))

    top = lib.cgc_morph_max_radius()
    assert top == constant('MORPH_MAX_RADIUS') == kernels.MORPH_MAX_RADIUS == ref.MAX_RADIUS >= 63
    assert lib.cgc_morph_tile_rows() == constant('MORPH_ROWS')
    span = constant('MORPH_SPAN')
    for r in range(0, top + 1):
        assert lib.cgc_morph_tile_cols(r) == span - 2 * ((r + 3) // 4 * 4) >= 128
    assert lib.cgc_morph_tile_cols(0) == span and lib.cgc_morph_tile_cols(1) == span - 8 == lib.cgc_morph_tile_cols(4)
    assert lib.cgc_morph_tile_cols(-1) == 0 == lib.cgc_morph_tile_cols(top + 1)
    for name, codes in (('SQUARE', 0), ('DISK', 1), ('DIAMOND', 2), ('ERODE', 0), ('DILATE', 1), ('GRADIENT', 2), ('PLAIN', 0),
                        ('OTHER_MINUS', 1), ('MINUS_OTHER', 2)):
        assert re.search(r'^#define CGC_MORPH_%s %d$' % (name, codes), header, flags=re.M), name
    assert kernels.MORPH_KINDS == {'square': 0, 'disk': 1, 'diamond': 2} and kernels.MORPH_OPS == {'erode': 0, 'dilate': 1, 'gradient': 2}
    assert kernels.MORPH_EPILOGUES == {None: 0, 'other_minus': 1, 'minus_other': 2}


def test_the_library_footprints_are_the_reference_footprints(lib):
    for kind, code in kernels.MORPH_KINDS.items():
        for r in range(0, lib.cgc_morph_max_radius() + 1):
            for dy in range(-r, r + 1):
                assert lib.cgc_morph_footprint_width(code, r, dy) == ref.width(kind, r, dy), (kind, r, dy)
            assert lib.cgc_morph_footprint_width(code, r, r + 1) == -1 == lib.cgc_morph_footprint_width(code, r, -r - 1)
    assert lib.cgc_morph_footprint_width(3, 2, 0) == -1 and lib.cgc_morph_footprint_width(1, 64, 0) == -1
    assert lib.cgc_morph_footprint_width(1, -1, 0) == -1


def test_abi_20_in_the_header_the_prototypes_and_the_library(lib):
    header = open(os.path.join(ROOT, 'include', 'cgc_hip.h')).read()
    assert lib.cgc_abi_version() == _abi.ABI_VERSION == int(re.search(r'#define CGC_ABI_VERSION (\d+)', header).group(1)) >= 20
    assert re.search(r'^ \*  20: flat grey-scale morphology', header, flags=re.M)
    for name in ('cgc_morph_max_radius', 'cgc_morph_tile_rows', 'cgc_morph_tile_cols', 'cgc_morph_footprint_width', 'cgc_morph'):
        assert name in _abi.PROTOTYPES and re.search(r'^int %s\(' % name, header, flags=re.M), name
        assert getattr(lib, name).argtypes == _abi.PROTOTYPES[name]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _abi.PROTOTYPES['cgc_morph'] == [P, P, I, I, I, I, I, I, P, I, P, P]
    assert _abi.PROTOTYPES['cgc_morph_tile_cols'] == [I] and _abi.PROTOTYPES['cgc_morph_footprint_width'] == [I, I, I]
