"""CPU: the host side of the region geometry (csrc/region.hip; cgc_net_amd.nuclei.region_geometry, region_shape, shape_features,
clear_border; kernels.HipKernels.region_geometry): what the public functions refuse before any launch, and what the library refuses
without launching.

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

import shape_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('cgc_region_geometry_max_side', 'cgc_region_geometry')


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


def labels(*shape, dtype=torch.int32):
    return torch.ones(shape or (4, 5), dtype=dtype)


def view(H, W, dtype=torch.int32):
    """An image of any size without memory behind it."""
    return torch.zeros(1, 1, dtype=dtype).expand(H, W)


KEPT = torch.ones(2, dtype=torch.int32)
CALLS = {'region_geometry': lambda lab, **kw: nuclei.region_geometry(lab, **kw),
         'shape_features': lambda lab, **kw: nuclei.shape_features(lab, KEPT, **kw),
         'clear_border': lambda lab, **kw: nuclei.clear_border(lab, **kw)}


# ------------------------------------------------------------------ the public functions
def test_only_tensors_on_the_gpu():
    for call in CALLS.values():
        for bad in (labels(), np.ones((4, 5), np.int32), None, [[1, 2]]):
            with pytest.raises(TypeError):
                call(bad)


@pytest.mark.parametrize('name', sorted(CALLS))
def test_form_of_the_labels(no_launch, name):
    call = CALLS[name]
    for dtype in (torch.bool, torch.float32, torch.float64):
        with pytest.raises(TypeError):
            call(labels(dtype=dtype), max_label=1)
    for shape in ((20,), (4, 5, 1), (1, 4, 5)):
        with pytest.raises(ValueError):
            call(labels(*shape), max_label=1)
    for bad in (-1, 2 ** 31 - 1, 1.0, True, '3'):
        with pytest.raises(ValueError, match='max_label|label values'):
            call(labels(), max_label=bad)
    with pytest.raises(ValueError, match='negative'):
        call(labels() - 2)


@pytest.mark.parametrize('name', sorted(CALLS))
def test_sides_and_quad_count(no_launch, name):
    call = CALLS[name]
    for H, W in ((32768, 4), (4, 32768), (32768, 32768), (65535, 3), (3, 2 ** 20)):
        with pytest.raises(ValueError, match='sides up to 32767'):
            call(view(H, W), max_label=1)
    kernels.HipKernels._check_geometry_dims('f', 32767, 32767)
    kernels.HipKernels._check_geometry_dims('f', 0, 0)


def test_quad_count_guard(monkeypatch):
    """With sides of at most 32767 the quad count (H + 1)(W + 1) <= 2^30 always fits; the second refusal guards the day the side
    limit is raised.  Lifted here, it refuses an image with H W < 2^31 <= (H + 1)(W + 1)."""
    assert nuclei.GEOMETRY_MAX_SIDE == 32767 and (32767 + 1) ** 2 < 2 ** 31
    monkeypatch.setattr(kernels, 'GEOMETRY_MAX_SIDE', 2 ** 31)
    assert 46340 * 46340 < 2 ** 31 <= 46341 * 46341
    with pytest.raises(ValueError, match=r'\(H \+ 1\)\(W \+ 1\) < 2\^31'):
        kernels.HipKernels._check_geometry_dims('f', 46340, 46340)
    kernels.HipKernels._check_geometry_dims('f', 46339, 46340)


def test_within(no_launch):
    for name in ('region_geometry', 'shape_features'):
        call = CALLS[name]
        for shape in ((5, 4), (4, 6), (4, 5, 1), (20,)):
            with pytest.raises(ValueError):
                call(labels(), max_label=1, within=torch.ones(shape, dtype=torch.uint8))
        with pytest.raises(TypeError):
            call(labels(), max_label=1, within=torch.ones(4, 5))
        with pytest.raises(TypeError):
            call(labels(), max_label=1, within=np.ones((4, 5), bool))
        with pytest.raises(ValueError):
            call(labels(), max_label=1, within=torch.ones(4, 5, dtype=torch.bool, device='meta'))


def test_kept_labels(no_launch):
    f = nuclei.shape_features
    for bad in ([1, 2], None, KEPT.to(torch.float32), KEPT.to(torch.int16), KEPT.to(torch.bool)):
        with pytest.raises(TypeError, match='kept_labels'):
            f(labels(), bad, max_label=1)
    for bad in (KEPT.reshape(1, 2), KEPT.to('meta'), KEPT[0]):
        with pytest.raises(ValueError, match='kept_labels'):
            f(labels(), bad, max_label=1)


def test_region_shape_takes_a_geometry():
    for bad in (None, (1, 2), torch.ones(3), {}):
        with pytest.raises(TypeError, match='RegionGeometry'):
            nuclei.region_shape(bad)


def test_names_and_columns():
    names = nuclei.SHAPE_FEATURE_NAMES
    assert names == ('area', 'major_axis', 'minor_axis', 'eccentricity', 'orientation', 'perimeter', 'circularity', 'convexity16',
                     'feret_max', 'feret_min', 'bbox_fill', 'holes', 'touches_border') == ref.FEATURES
    assert len(names) == 13 == len(set(names))
    assert nuclei.GEOMETRY_DIRECTIONS == kernels.GEOMETRY_DIRECTIONS == ref.DIRECTIONS
    assert nuclei.RegionGeometry._fields == ('count', 'sy', 'sx', 'syy', 'sxy', 'sxx', 'extents', 'quads', 'border')
    assert set(nuclei.RegionShape._fields) == set(ref.SHAPE_FLOATS + ref.SHAPE_INTS)


def test_shape_and_columns_on_the_host():
    """region_shape and the column table are tensor arithmetic: on host tensors they run without a GPU, and the column count is that of
    the names.  Compared with the restatement on a small case, float32 against float32."""
    rng = np.random.RandomState(3)
    lab = rng.randint(0, 4, (9, 11)).astype(np.int32)
    g = ref.geometry(lab, 5)
    geometry = nuclei.RegionGeometry(*[torch.from_numpy(g[k]) for k in nuclei.RegionGeometry._fields])
    shape = nuclei.region_shape(geometry)
    want = ref.shape(g)
    for k in ref.SHAPE_INTS:
        assert getattr(shape, k).dtype == torch.int32 and np.array_equal(getattr(shape, k).numpy(), want[k]), k
    for k in ref.SHAPE_FLOATS:
        got = getattr(shape, k)
        assert got.dtype == torch.float32 and tuple(got.shape) == (6,), k
        assert np.allclose(got.numpy(), want[k].astype(np.float32), rtol=2.0 ** -22, atol=0), k
    table = nuclei._shape_table(shape)
    assert tuple(table.shape) == (6, len(nuclei.SHAPE_FEATURE_NAMES)) and table.dtype == torch.float32
    assert np.allclose(table.numpy(), ref.features(want).astype(np.float32), rtol=2.0 ** -22, atol=0)
    assert not table[4:].any()                                          # rows without a pixel


# ------------------------------------------------------------------ the kernel table
class Untouchable(object):
    """Stands in for a tensor: any use but its shape fails the test."""
    shape = (4, 5)

    def __getattr__(self, name):
        pytest.fail('a tensor was touched (%s)' % name)


def test_the_kernel_table_refuses_bad_parameters_before_any_tensor():
    call = kernels.HipKernels.region_geometry
    U = Untouchable()
    for bad in (-1, 2 ** 31 - 1, None, 2.0, True):
        with pytest.raises(ValueError, match='max_label'):
            call(None, U, bad)
    big = Untouchable()
    big.shape = (32768, 2)
    with pytest.raises(ValueError, match='32767'):
        call(None, big, 3)


def test_signatures_and_documents():
    sig = {'region_geometry': (['labels', 'max_label', 'within'], [None, None]),
           'region_shape': (['geometry'], []),
           'shape_features': (['labels', 'kept_labels', 'max_label', 'within'], [None, None]),
           'clear_border': (['labels', 'max_label'], [None])}
    for name, (names, defaults) in sig.items():
        p = inspect.signature(getattr(nuclei, name)).parameters
        assert list(p) == names, name
        assert [p[k].default for k in names[len(names) - len(defaults):]] == defaults, name
        assert 'Host syncs: ' in getattr(nuclei, name).__doc__, name
    doc = nuclei.region_shape.__doc__
    for text in ('CONTAINS the convex hull', 'lower bound of solidity', 'atan2(2 cov, var_x - var_y) / 2', 'n2 + (n1 + n3 + 2 nd) / sqrt(2)',
                 '(n1 - n3 + 2 nd) / 4', '(n1 - n3 - 2 nd) / 4', 'n1 + n2 + n3 + 2 nd', 'shoelace', 'sqrt(4 n / pi)'):
        assert text in doc, text
    usage = 'shape_features(L, kept, max_label=n)], 1)'
    assert usage in nuclei.shape_features.__doc__ and usage in nuclei.__doc__
    for cls in (kernels.KernelSpec, kernels.HipKernels):
        assert list(inspect.signature(cls.region_geometry).parameters) == ['self', 'labels', 'max_label', 'within']
    doc = kernels.KernelSpec.region_geometry.__doc__
    for k in range(1, 10):
        assert '\n        %d.  ' % k in doc, k
    for text in ('no host read', 'CGC_EINVAL', 'H * W = 0', '(H + 1)(W + 1) < 2^31', '32767', 'bit-identical', 'n4 =', 'count == 0',
                 'decided from coordinates'):
        assert text in doc, text
    with pytest.raises(NotImplementedError):
        kernels.KernelSpec().region_geometry(None, 1)
    for name in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, name)).read()
        assert 'region_geometry' in text and 'shape_features' in text, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '## Region geometry (csrc/region.hip)' in design and 'shape_bench.json' in design
    assert re.search(r'^\| F19 ', open(os.path.join(ROOT, 'SURVEY.md')).read(), flags=re.M)
    assert os.path.exists(os.path.join(ROOT, 'tools', 'shape_bench.py'))


# ------------------------------------------------------------------ the library, without a launch
def test_library_refusals(lib):
    einval = -1
    buf = (ctypes.c_int64 * 64)()                                       # any non-NULL address: nothing is launched
    some = ctypes.addressof(buf)

    # cgc_region_geometry(labels, within, wbytes, H, W, max_label, count, sums, extents, quads, border, meta, stream)
    def geom(labels=some, within=None, wbytes=0, H=4, W=5, max_label=3, count=some, sums=some, extents=some, quads=some, border=some,
             meta=some):
        return lib.cgc_region_geometry(labels, within, wbytes, H, W, max_label, count, sums, extents, quads, border, meta, None)

    for H, W in ((32768, 4), (4, 32768), (32768, 32768), (2 ** 30, 1), (1, 2 ** 30), (-1, 5), (4, -1), (2 ** 16, 2 ** 15), (46340, 46340)):
        assert geom(H=H, W=W) == einval, (H, W)
    for bad in (-1, 2 ** 31 - 1):
        assert geom(max_label=bad) == einval and geom(H=0, W=0, max_label=bad) == einval
    for wbytes in (0, 3, 16, -1):
        assert geom(within=some, wbytes=wbytes) == einval
    for name in ('labels', 'count', 'sums', 'extents', 'quads', 'border', 'meta'):
        assert geom(**{name: None}) == einval, name
    for name in ('count', 'sums', 'extents', 'quads', 'border', 'meta'):
        assert geom(H=0, W=3, **{name: None}) == einval, name


def test_constants(lib):
    source = open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'region.hip')).read()
    side = int(re.search(r'constexpr int GEOM_MAX_SIDE = (\d+);', source).group(1))
    assert lib.cgc_region_geometry_max_side() == side == kernels.GEOMETRY_MAX_SIDE == 32767
    assert 2 ** 31 * side * side < 2 ** 63                              # sum x^2 over 2^31 pixels
    t = lib.cgc_region_tile_side()
    assert t * t * (t - 1) * (t - 1) < 2 ** 32                          # a tile's sums in tile coordinates fit 32 bits
    assert lib.cgc_region_table_slots() * 4 == 256                      # the flush gives a slot four threads
    a = [int(v) for v in re.search(r'int geom_a\(int d\) \{ return (.*?); \}', source).group(1).replace('d ==', '').replace('?', ' ').replace(':', ' ').split()]
    b = [int(v) for v in re.search(r'int geom_b\(int d\) \{ return (.*?); \}', source).group(1).replace('d ==', '').replace('?', ' ').replace(':', ' ').split()]
    assert tuple(zip(a[1::2] + a[-1:], b[1::2] + b[-1:])) == kernels.GEOMETRY_DIRECTIONS      # "k value k value ... last"
    assert all(bb >= 0 for _, bb in kernels.GEOMETRY_DIRECTIONS)        # a column run attains its extents at its ends
    assert not re.search(r'for \(;;\)|while \(', source)                # no loop without a bound in this file


def test_abi_25_in_the_header_the_prototypes_and_the_library(lib):
    header = open(os.path.join(ROOT, 'include', 'cgc_hip.h')).read()
    assert lib.cgc_abi_version() == _abi.ABI_VERSION == int(re.search(r'#define CGC_ABI_VERSION (\d+)', header).group(1)) >= 25
    assert re.search(r'^ \*  25: region geometry', header, flags=re.M)
    for name in SYMBOLS:
        assert name in _abi.PROTOTYPES and re.search(r'^int %s\(' % name, header, flags=re.M), name
        assert getattr(lib, name).argtypes == _abi.PROTOTYPES[name]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _abi.PROTOTYPES['cgc_region_geometry'] == [P, P, I, I, I, I, P, P, P, P, P, P, P]
    assert 'region_geometry' in kernels.KernelSpec.__dict__
