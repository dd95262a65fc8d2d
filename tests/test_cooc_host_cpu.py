"""CPU: the host side of the region co-occurrence (csrc/region.hip; cgc_net_amd.nuclei.region_cooccurrence, level_lut, cooc_directions,
cooccurrence_properties, texture_features; kernels.HipKernels.region_cooccurrence): what the public functions refuse before any
launch, and what the library refuses without launching.

As in tests/test_region_host_cpu.py the tests lift the "on the GPU" refusal (``on_gpu=False``) and replace the kernel table by one
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

import cooc_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('cgc_region_cooc_max_offset', 'cgc_region_cooc_max_offsets', 'cgc_region_cooccurrence')


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


def labels(*shape, dtype=torch.int32):
    return torch.ones(shape or (4, 5), dtype=dtype)


def tile(*shape):
    return torch.ones(shape or (4, 5, 3), dtype=torch.uint8)


def cooc(lab=None, val=None, **kw):
    kw.setdefault('max_label', 1)
    return nuclei.region_cooccurrence(labels() if lab is None else lab, image() if val is None else val, **kw)


# ------------------------------------------------------------------ the public functions
def test_only_tensors_on_the_gpu():
    for bad in (labels(), np.ones((4, 5), np.int32), None, [[1, 2]]):
        with pytest.raises(TypeError):
            nuclei.region_cooccurrence(bad, image())
    with pytest.raises(TypeError):
        nuclei.texture_features(labels(), tile(), torch.ones(2, dtype=torch.int32))


def test_form_of_the_images(no_launch):
    for dtype in (torch.bool, torch.float32):
        with pytest.raises(TypeError):
            cooc(labels(dtype=dtype))
    for dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.float32):      # uint8 or bool only
        with pytest.raises(TypeError):
            cooc(val=image(dtype=dtype))
    for shape in ((5, 4), (4, 6), (4, 5, 1), (20,)):
        with pytest.raises(ValueError):
            cooc(val=image(*shape))
        with pytest.raises(ValueError):
            cooc(within=image(*shape))
    with pytest.raises(TypeError):
        cooc(within=image(dtype=torch.float32))
    for bad in (-1, 2 ** 31 - 1, 1.0, True):
        with pytest.raises(ValueError, match='max_label|label values'):
            cooc(max_label=bad)
    with pytest.raises(ValueError, match='negative'):
        cooc(labels() - 2, max_label=None)
    # 2^30 pixels: a view without memory behind it
    big = torch.zeros(1, 1, dtype=torch.int32).expand(2 ** 15, 2 ** 15)
    with pytest.raises(ValueError, match='2\\^30'):
        cooc(big, torch.zeros(1, 1, dtype=torch.uint8).expand(2 ** 15, 2 ** 15))
    with pytest.raises(ValueError, match='2\\^30'):
        nuclei.texture_features(big, torch.zeros(1, 1, 1, dtype=torch.uint8).expand(2 ** 15, 2 ** 15, 3), torch.ones(2, dtype=torch.int32),
                                max_label=1)


def test_levels_lut_and_offsets_are_refused_before_a_launch(no_launch):
    for bad in (1, 0, -3, 17, 256, 4.0, '4', None, True):
        with pytest.raises(ValueError, match='levels'):
            cooc(levels=bad)
    good = list(ref.level_lut(4))
    for bad in (good[:255], good + [0], [], [good], np.zeros((2, 128), np.int64), torch.zeros(16, 16, dtype=torch.int64)):
        with pytest.raises(ValueError, match='lut'):
            cooc(levels=4, lut=bad)
    for entry in (4, 5, 255, -1):
        for form in (list, tuple, np.array, torch.tensor):
            with pytest.raises(ValueError, match='lut'):
                cooc(levels=4, lut=form(good[:17] + [entry] + good[18:]))
    with pytest.raises(ValueError, match='lut'):
        cooc(levels=4, lut=ref.level_lut(5))
    for bad in (np.zeros(256, np.float32), torch.zeros(256), [0.5] * 256):
        with pytest.raises(ValueError, match='lut'):
            cooc(levels=4, lut=bad)
    with pytest.raises(TypeError, match='lut'):
        cooc(levels=4, lut=torch.zeros(256, dtype=torch.int64, device='meta'))       # not on the host: it is a launch argument
    for bad in (7, 'abc', {1: 2}):
        with pytest.raises((TypeError, ValueError), match='lut'):
            cooc(levels=4, lut=bad)
    for bad in ([], (), [(0, 1)] * 9, tuple(nuclei.COOC_DIRECTIONS) * 3):
        with pytest.raises(ValueError, match='1 to 8 offsets'):
            cooc(offsets=bad)
    for bad in ([(0, 0)], [(0, 1), (0, 0)], [(17, 0)], [(0, -17)], [(-17, 17)], [(1, 100)]):
        with pytest.raises(ValueError, match='offset'):
            cooc(offsets=bad)
    for bad in (3, None, [1, 2], [(1,)], [(1, 2, 3)], [(0.5, 1)], [('a', 'b')]):
        with pytest.raises(ValueError, match='offsets'):
            cooc(offsets=bad)


def test_level_lut_and_directions():
    for levels in range(2, 17):
        for lo, hi in ((0, 255), (20, 159), (0, 1), (254, 255), (100, 101)):
            lut = nuclei.level_lut(levels, lo, hi)
            assert isinstance(lut, tuple) and all(type(v) is int for v in lut) and list(lut) == ref.level_lut(levels, lo, hi)
    for levels in (2, 4, 8, 16):
        assert nuclei.level_lut(levels) == tuple(v * levels >> 8 for v in range(256))
    assert nuclei.level_lut(np.int64(8), np.uint8(20), np.int32(159)) == nuclei.level_lut(8, 20, 159)
    for bad in (1, 17, 0, 2.0, None, True):
        with pytest.raises(ValueError, match='levels'):
            nuclei.level_lut(bad)
    for lo, hi in ((-1, 255), (0, 256), (10, 10), (11, 10), (0.0, 255), (0, None), (True, 255)):
        with pytest.raises(ValueError, match='lo|hi'):
            nuclei.level_lut(4, lo, hi)
    assert nuclei.COOC_DIRECTIONS == ((0, 1), (1, 1), (1, 0), (1, -1)) == ref.DIRECTIONS == nuclei.cooc_directions() == nuclei.cooc_directions(1)
    assert nuclei.cooc_directions(3) == ((0, 3), (3, 3), (3, 0), (3, -3)) and nuclei.cooc_directions(16)[3] == (16, -16)
    for bad in (0, -1, 17, 1.0, None, True):
        with pytest.raises(ValueError, match='distance'):
            nuclei.cooc_directions(bad)


def test_cooccurrence_properties_on_the_host():
    assert nuclei.COOC_PROPERTIES == ('contrast', 'dissimilarity', 'homogeneity', 'ASM', 'energy', 'correlation', 'entropy') == ref.PROPERTIES
    t = np.zeros((2, 5, 3, 3), np.int32)
    t[0, 0] = [[2, 0, 0], [0, 0, 0], [0, 0, 2]]
    t[0, 1] = [[0, 0, 4], [0, 0, 0], [4, 0, 0]]
    t[0, 2] = [[0, 0, 0], [0, 9, 0], [0, 0, 0]]                           # one level: correlation is 1 by rule
    t[0, 3] = [[0, 3, 5], [0, 0, 0], [0, 0, 0]]                           # one level in the anchors' marginal only
    t[1, 0] = [[0, 0, 0], [3, 0, 0], [5, 0, 0]]                           # ... in the partners' only
    t[1, 1] = np.random.RandomState(1).randint(0, 1000, (3, 3))
    got = nuclei.cooccurrence_properties(torch.from_numpy(t))
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 5, 7)
    want = ref.properties(t)
    assert np.array_equal(got.numpy(), want.astype(np.float32))         # float64, rounded once: here the same float32
    assert got[0, 2].tolist() == [0, 0, 1, 1, 1, 1, 0] and got[0, 4].tolist() == [0] * 7 and got[1, 2].tolist() == [0] * 7
    assert got[0, 3, 5] == 1 and got[1, 0, 5] == 1 and got[0, 0, 5] == 1 and got[0, 1, 5] == -1
    some = nuclei.cooccurrence_properties(torch.from_numpy(t), ('entropy', 'contrast'))
    assert tuple(some.shape) == (2, 5, 2) and torch.equal(some[:, :, 0], got[:, :, 6]) and torch.equal(some[:, :, 1], got[:, :, 0])
    assert torch.equal(nuclei.cooccurrence_properties(torch.from_numpy(t).long(), ['energy'])[:, :, 0], got[:, :, 4])
    for bad in ((), ['contrast', 'mean'], 'contrast', None, 3):
        with pytest.raises(ValueError, match='props'):
            nuclei.cooccurrence_properties(torch.from_numpy(t), bad)
    for bad in (t, None, torch.from_numpy(t).float(), torch.from_numpy(t) > 0):
        with pytest.raises(TypeError):
            nuclei.cooccurrence_properties(bad)
    for bad in (torch.zeros(2, 5, 9, dtype=torch.int32), torch.zeros(2, 5, 3, 4, dtype=torch.int32), torch.zeros(3, 3, dtype=torch.int32)):
        with pytest.raises(ValueError, match='tables'):
            nuclei.cooccurrence_properties(bad)
    assert tuple(nuclei.cooccurrence_properties(torch.zeros(0, 4, 3, 3, dtype=torch.int32)).shape) == (0, 4, 7)


def test_texture_features_refusals(no_launch):
    kept = torch.ones(2, dtype=torch.int32)
    f = nuclei.texture_features
    for bad in (labels(dtype=torch.bool), labels(dtype=torch.float32)):
        with pytest.raises(TypeError):
            f(bad, tile(), kept, max_label=1)
    for bad in (np.ones((4, 5, 3), np.uint8), None):
        with pytest.raises(TypeError):
            f(labels(), bad, kept, max_label=1)
    for bad in (tile(4, 5), tile(4, 5, 4), tile(5, 4, 3), tile(4, 6, 3)):
        with pytest.raises(ValueError):
            f(labels(), bad, kept, max_label=1)
    for bad in ([1, 2], None, kept.to(torch.float32), kept.to(torch.int16)):
        with pytest.raises(TypeError, match='kept_labels'):
            f(labels(), tile(), bad, max_label=1)
    for bad in (kept.reshape(1, 2), kept.to('meta')):
        with pytest.raises(ValueError, match='kept_labels'):
            f(labels(), tile(), bad, max_label=1)
    with pytest.raises(ValueError, match='order'):
        f(labels(), tile(), kept, order='gbr', max_label=1)
    for bad in ((), (3,), (1, 0), (0, 0), 5):
        with pytest.raises(ValueError, match='planes'):
            f(labels(), tile(), kept, planes=bad, max_label=1)
    for bad in (1, 17, 4.0, None):
        with pytest.raises(ValueError, match='levels'):
            f(labels(), tile(), kept, levels=bad, max_label=1)
    for lo, hi in ((-1, None), (0, 256), (100, 100), (200, 159), (0, 159.0)):
        with pytest.raises(ValueError, match='lo|hi'):
            f(labels(), tile(), kept, lo=lo, hi=hi, max_label=1)
    for bad in (0, 17, -1, 1.5, None):
        with pytest.raises(ValueError, match='distance'):
            f(labels(), tile(), kept, distance=bad, max_label=1)
    for bad in (-1, 2 ** 31 - 1, 1.5, True):
        with pytest.raises(ValueError):
            f(labels(), tile(), kept, max_label=bad)
    names = nuclei.TEXTURE_FEATURE_NAMES
    assert len(names) == 12 == len(set(names)) and names[:2] == ('hematoxylin_contrast_mean', 'hematoxylin_contrast_range')
    assert names[-1] == 'hematoxylin_entropy_range' and not any('ASM' in n for n in names)
    assert nuclei.TEXTURE_PROPERTIES == tuple(p for p in nuclei.COOC_PROPERTIES if p != 'ASM')


# ------------------------------------------------------------------ the kernel table
class Untouchable(object):
    """Stands in for a tensor: any use fails the test."""

    def __getattr__(self, name):
        pytest.fail('a tensor was touched (%s)' % name)


def test_the_kernel_table_refuses_bad_parameters_before_any_tensor():
    call = kernels.HipKernels.region_cooccurrence
    lut, offs = ref.level_lut(4), [(0, 1)]
    U = Untouchable()
    for bad in (-1, 2 ** 31 - 1, None, 2.0, True):
        with pytest.raises(ValueError, match='max_label'):
            call(None, U, U, bad, lut, 4, offs, True)
    for bad in (1, 17, None, 4.0, True):
        with pytest.raises(ValueError, match='levels'):
            call(None, U, U, 3, lut, bad, offs, True)
    for bad in (lut[:-1], lut + [0], lut[:-1] + [4], lut[:-1] + [-1], None, [0.5] * 256):
        with pytest.raises(ValueError, match='lut'):
            call(None, U, U, 3, bad, 4, offs, True)
    for bad in ([], [(0, 1)] * 9, [(0, 0)], [(0, 17)], [(-17, 0)], None, [3], [(1, 2, 3)]):
        with pytest.raises(ValueError, match='offset'):
            call(None, U, U, 3, lut, 4, bad, True)
    for dtype in (torch.bool, torch.int8, torch.int32):
        with pytest.raises(TypeError, match='values'):
            call(None, U, torch.ones(2, 2, dtype=dtype), 3, lut, 4, offs, True)
    c_lut, c_offs = kernels.HipKernels._check_cooc(lut, 4, [(1, -1), (0, 16)])
    assert list(c_lut) == lut and list(c_offs) == [1, -1, 0, 16]


def test_signatures_and_documents():
    sig = {'level_lut': (['levels', 'lo', 'hi'], [0, 255]),
           'cooc_directions': (['distance'], [1]),
           'region_cooccurrence': (['labels', 'values', 'offsets', 'levels', 'lut', 'symmetric', 'max_label', 'within'],
                                   [nuclei.COOC_DIRECTIONS, 16, None, True, None, None]),
           'cooccurrence_properties': (['tables', 'props'], [nuclei.COOC_PROPERTIES]),
           'texture_features': (['labels', 'tile', 'kept_labels', 'stains', 'order', 'planes', 'levels', 'lo', 'hi', 'distance', 'max_label'],
                                [None, 'bgr', (0,), 16, 0, None, 1, None])}
    for name, (names, defaults) in sig.items():
        p = inspect.signature(getattr(nuclei, name)).parameters
        assert list(p) == names, name
        assert [p[k].default for k in names[len(names) - len(defaults):]] == defaults, name
        assert 'Host syncs: ' in getattr(nuclei, name).__doc__, name
    assert '1 / 64 of a natural-log unit' in nuclei.texture_features.__doc__ and '160' in nuclei.texture_features.__doc__
    usage = 'x = torch.cat([features, stain_features(L, tile, kept, max_label=n), texture_features(L, tile, kept, hi=159, max_label=n)], 1)'
    assert usage in nuclei.texture_features.__doc__ and usage in nuclei.__doc__
    for cls in (kernels.KernelSpec, kernels.HipKernels):
        assert list(inspect.signature(cls.region_cooccurrence).parameters) == ['self', 'labels', 'values', 'max_label', 'lut', 'levels',
                                                                                'offsets', 'symmetric', 'within']
    doc = kernels.KernelSpec.region_cooccurrence.__doc__
    for k in range(1, 10):
        assert '\n        %d.  ' % k in doc, k
    for text in ('no host read', 'meta[0]', 'once per call', 'CGC_EINVAL', 'H * W = 0', 'H * W < 2^30', 'bit-identical', 'symmetric=True',
                 'decided from its coordinates', 'within = labels != 0'):
        assert text in doc, text
    with pytest.raises(NotImplementedError):
        kernels.KernelSpec().region_cooccurrence(None, None, 1, None, 4, [(0, 1)], True)
    for name in ('README.md', 'DESIGN.md'):
        text = open(os.path.join(ROOT, name)).read()
        assert 'region_cooccurrence' in text and 'texture_features' in text, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '## Region co-occurrence (csrc/region.hip)' in design and 'cooc_bench.json' in design
    assert os.path.exists(os.path.join(ROOT, 'tools', 'cooc_bench.py'))


# ------------------------------------------------------------------ the library, without a launch
def test_library_refusals(lib):
    einval = -1
    buf = (ctypes.c_int64 * 64)()                                       # any non-NULL address: nothing is launched
    some = ctypes.addressof(buf)
    good_lut = (ctypes.c_uint8 * 256)(*ref.level_lut(4))

    # cgc_region_cooccurrence(labels, values, within, wbytes, H, W, max_label, lut, levels, offsets, noff, symmetric, tables, meta, stream)
    def cooc(labels=some, values=some, within=None, wbytes=0, H=4, W=5, max_label=3, lut=good_lut, levels=4, offsets=((0, 1),), noff=None,
             symmetric=1, tables=some, meta=some):
        flat = [v for o in offsets for v in o]
        arr = (ctypes.c_int * max(len(flat), 2))(*flat)
        return lib.cgc_region_cooccurrence(labels, values, within, wbytes, H, W, max_label, lut, levels, arr, len(offsets) if noff is None else noff,
                                           symmetric, tables, meta, None)

    for levels in (1, 0, -1, 17, 256):
        assert cooc(levels=levels) == einval
    assert cooc(levels=3) == einval                                     # the lut of four levels holds a 3
    for v, entry in ((0, 4), (255, 4), (100, 255), (17, 16)):
        lut = list(ref.level_lut(4))
        lut[v] = entry
        assert cooc(lut=(ctypes.c_uint8 * 256)(*lut)) == einval
    for noff in (0, 9, -1, 100):
        assert cooc(offsets=((0, 1),) * 9, noff=noff) == einval
    for bad in ((0, 0), (17, 0), (0, 17), (-17, 1), (1, -17), (2 ** 20, 0)):
        assert cooc(offsets=(bad,)) == einval and cooc(offsets=((0, 1), bad)) == einval
    for H, W in ((2 ** 15, 2 ** 15), (2 ** 30, 1), (1, 2 ** 30), (-1, 5), (4, -1), (2 ** 16, 2 ** 15)):
        assert cooc(H=H, W=W) == einval
    for bad in (-1, 2 ** 31 - 1):
        assert cooc(max_label=bad) == einval and cooc(H=0, W=0, max_label=bad) == einval
    for wbytes in (0, 3, 16, -1):
        assert cooc(within=some, wbytes=wbytes) == einval
    for name in ('labels', 'values', 'lut', 'tables', 'meta'):
        assert cooc(**{name: None}) == einval, name
    for name in ('lut', 'tables', 'meta'):
        assert cooc(H=0, W=3, **{name: None}) == einval, name
    assert lib.cgc_region_cooccurrence(some, some, None, 0, 4, 5, 3, good_lut, 4, None, 1, 1, some, some, None) == einval


def test_constants_and_geometry(lib):
    source = open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'region.hip')).read()

    def constant(name):
        return int(re.search(r'constexpr int %s = (\d+);' % name, source).group(1))

    assert lib.cgc_region_cooc_max_offset() == constant('COOC_MAX_OFFSET') == kernels.COOC_MAX_OFFSET == nuclei.COOC_MAX_OFFSET == 16
    assert lib.cgc_region_cooc_max_offsets() == constant('COOC_MAX_OFFSETS') == kernels.COOC_MAX_OFFSETS == nuclei.COOC_MAX_OFFSETS == 8
    assert constant('COOC_MAX_LEVELS') == kernels.COOC_MAX_LEVELS == nuclei.COOC_MAX_LEVELS == ref.MAX_LEVELS == 16
    assert ref.MAX_OFFSET == 16 and ref.MAX_OFFSETS == 8 and kernels.COOC_MAX_PIXELS == 2 ** 30
    assert constant('COOC_MAX_LEVELS') ** 2 <= 256                      # a table is the 256 bins of a slot
    assert 2 * lib.cgc_region_tile_side() ** 2 < 2 ** 16                # a 16-bit bin holds a tile of symmetric pairs of one label and level
    assert '2 * REGION_TILE * REGION_TILE < (1 << 16)' in source
    assert not re.search(r'for \(;;\)|while \(', source)                # no loop without a bound in this file


def test_abi_24_in_the_header_the_prototypes_and_the_library(lib):
    header = open(os.path.join(ROOT, 'include', 'cgc_hip.h')).read()
    assert lib.cgc_abi_version() == _abi.ABI_VERSION == int(re.search(r'#define CGC_ABI_VERSION (\d+)', header).group(1)) >= 24
    assert re.search(r'^ \*  24: region co-occurrence', header, flags=re.M)
    for name in SYMBOLS:
        assert name in _abi.PROTOTYPES and re.search(r'^int %s\(' % name, header, flags=re.M), name
        assert getattr(lib, name).argtypes == _abi.PROTOTYPES[name]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _abi.PROTOTYPES['cgc_region_cooccurrence'] == [P, P, P, I, I, I, I, P, I, P, I, I, P, P, P]
    assert 'region_cooccurrence' in kernels.KernelSpec.__dict__ and 'cgc_region_cooccurrence' in header
