"""CPU: the host side of the region hull (csrc/region.hip; cgc_net_amd.nuclei.region_hull, hull_shape, hull_features;
kernels.HipKernels.region_hull): what the public functions refuse before any launch, what the library refuses without launching, and
hull_shape on hand-written integer tables.

As in tests/test_shape_host_cpu.py the tests lift the "on the GPU" refusal (``on_gpu=False``) and replace the kernel table by one
that fails the test when it is asked for: every refusal checked here is raised before any launch."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import _abi, kernels, nuclei

import hull_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('cgc_region_hull_tall_rows', 'cgc_region_hull_ws_bytes', 'cgc_region_hull_spans', 'cgc_region_hull')


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
CALLS = {'region_hull': lambda lab, **kw: nuclei.region_hull(lab, **kw),
         'region_hull_vertices': lambda lab, **kw: nuclei.region_hull(lab, return_vertices=True, **kw),
         'hull_features': lambda lab, **kw: nuclei.hull_features(lab, KEPT, **kw)}


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
    for H, W in ((32768, 4), (4, 32768), (65535, 3)):
        with pytest.raises(ValueError, match='sides up to 32767'):
            call(view(H, W), max_label=1)


def test_within(no_launch):
    for name in ('region_hull', 'hull_features'):
        call = CALLS[name]
        for shape in ((5, 4), (4, 6), (4, 5, 1), (20,)):
            with pytest.raises(ValueError):
                call(labels(), max_label=1, within=torch.ones(shape, dtype=torch.uint8))
        with pytest.raises(TypeError):
            call(labels(), max_label=1, within=torch.ones(4, 5))
        with pytest.raises(ValueError):
            call(labels(), max_label=1, within=torch.ones(4, 5, dtype=torch.bool, device='meta'))


def test_kept_labels(no_launch):
    f = nuclei.hull_features
    for bad in ([1, 2], None, KEPT.to(torch.float32), KEPT.to(torch.int16), KEPT.to(torch.bool)):
        with pytest.raises(TypeError, match='kept_labels'):
            f(labels(), bad, max_label=1)
    for bad in (KEPT.reshape(1, 2), KEPT.to('meta'), KEPT[0]):
        with pytest.raises(ValueError, match='kept_labels'):
            f(labels(), bad, max_label=1)


def hand_tables(rows):
    """RegionHull and RegionGeometry (only its count matters) from rows of (n, vertices (y, x) in hull order or None)."""
    t = {k: [] for k in ref.TABLES}
    for n, verts in rows:
        m = ref.measure([(x, y) for y, x in verts]) if verts else dict(count=0, area2=0, diameter2=0, diameter_ends=((0, 0), (0, 0)),
                                                                       width_cross=0, width_edge=(0, 0), perimeter=0.0)
        for k in ref.TABLES:
            t[k].append(m[k])
    dt = dict(count=torch.int32, area2=torch.int64, diameter2=torch.int64, diameter_ends=torch.int32, width_cross=torch.int64,
              width_edge=torch.int32, perimeter=torch.float64)
    hull = nuclei.RegionHull(*[torch.tensor(t[k], dtype=dt[k]) for k in ref.TABLES])
    R = len(rows)
    z = torch.zeros(R, dtype=torch.int64)
    geometry = nuclei.RegionGeometry(torch.tensor([n for n, _ in rows], dtype=torch.int32), z, z, z, z, z,
                                     torch.zeros(R, 8, 2, dtype=torch.int32), torch.zeros(R, 4, dtype=torch.int32), torch.zeros(R, dtype=torch.int32))
    return hull, geometry


def test_hull_shape_on_hand_tables():
    square = [(0, 0), (1, 0), (1, 1), (0, 1)]
    rect = [(2, 1), (5, 1), (5, 6), (2, 6)]                               # 3 rows x 5 columns
    triangle = [(0, 0), (3, 0), (3, 3), (2, 3), (0, 1)]                   # the squares of x <= y, 0 <= x, y < 3: a right triangle of six squares
    tall = [(0, 0), (4, 0), (4, 1), (0, 1)]                               # a column: the diameter points down and right
    anti = [(0, 1), (1, 0), (2, 0), (2, 1), (1, 2), (0, 2)]               # pixels (0, 1) and (1, 0): the diameter (2, 0) - (0, 2) points up
    hull, geometry = hand_tables([(1, square), (15, rect), (0, None), (6, triangle), (4, tall), (2, anti)])
    s = nuclei.hull_shape(hull, geometry)
    assert isinstance(s, nuclei.HullShape) and all(v.dtype == torch.float32 and tuple(v.shape) == (6,) for v in s)
    f = np.float32
    assert s.convex_area.tolist() == [1.0, 15.0, 0.0, 7.0, 4.0, 3.0]
    assert s.solidity.tolist()[:5] == [1.0, 1.0, 0.0, f(6 / 7.0), 1.0]
    assert s.convex_perimeter.tolist()[:5] == [4.0, 16.0, 0.0, f(3 + 3 + 1 + math.sqrt(8) + 1), 10.0]
    assert s.feret_max.tolist()[:5] == [f(math.sqrt(2)), f(math.sqrt(34)), 0.0, f(math.sqrt(18)), f(math.sqrt(17))]
    assert s.feret_min.tolist()[:5] == [1.0, 3.0, 0.0, f(8 / math.sqrt(8)), 1.0]
    assert s.feret_ratio.tolist()[:3] == [f(1 / math.sqrt(2)), f(3 / math.sqrt(34)), 0.0]
    assert s.feret_angle.tolist()[:5] == [f(math.pi / 4), f(math.atan2(3, 5)), 0.0, f(math.pi / 4), f(math.atan2(4, 1))]
    assert s.feret_angle[5].item() == f(-math.pi / 4)                     # from (2, 0) to (0, 2): dy = -2, dx = 2
    assert s.vertices.tolist() == [4.0, 4.0, 0.0, 5.0, 4.0, 6.0]
    assert [v[2].item() for v in s] == [0.0] * 8                          # a row without a pixel
    up = nuclei.RegionHull(*[t.clone() for t in hull[:7]])
    up.diameter_ends[0] = torch.tensor([[0, 0], [5, 0]])                  # straight down: dx = 0, dy > 0
    up.diameter_ends[1] = torch.tensor([[5, 0], [0, 0]])                  # straight up is the same line
    a = nuclei.hull_shape(up, geometry).feret_angle
    assert a[0].item() == a[1].item() == f(math.pi / 2)


def test_hull_shape_takes_a_hull_and_a_geometry():
    hull, geometry = hand_tables([(1, [(0, 0), (1, 0), (1, 1), (0, 1)])])
    for bad in ((None, geometry), (hull, None), (geometry, hull), (tuple(hull), geometry), (hull, tuple(geometry))):
        with pytest.raises(TypeError, match='RegionHull'):
            nuclei.hull_shape(*bad)
    other = hand_tables([(1, [(0, 0), (1, 0), (1, 1), (0, 1)])] * 2)[1]
    with pytest.raises(ValueError, match='same labels'):
        nuclei.hull_shape(hull, other)


def test_names_and_columns():
    assert nuclei.HULL_FEATURE_NAMES == ('solidity', 'convex_area', 'convex_perimeter', 'feret_max', 'feret_min', 'feret_ratio',
                                         'feret_angle') == ref.FEATURES
    assert nuclei.RegionHull._fields == ref.TABLES + ('vertices', 'ptr')
    assert nuclei.HullShape._fields == ('convex_area', 'solidity', 'convex_perimeter', 'feret_max', 'feret_min', 'feret_ratio', 'feret_angle',
                                        'vertices')
    assert set(nuclei.HULL_FEATURE_NAMES) < set(nuclei.HullShape._fields)


# ------------------------------------------------------------------ the kernel table
class Untouchable(object):
    """Stands in for a tensor: any use but its shape fails the test."""
    shape = (4, 5)

    def __getattr__(self, name):
        pytest.fail('a tensor was touched (%s)' % name)


def test_the_kernel_table_refuses_bad_parameters_before_any_tensor():
    call = kernels.HipKernels.region_hull
    U = Untouchable()
    for bad in (-1, 2 ** 31 - 1, None, 2.0, True):
        with pytest.raises(ValueError, match='max_label'):
            call(None, U, bad, U, U, 0)
    big = Untouchable()
    big.shape = (32768, 2)
    with pytest.raises(ValueError, match='32767'):
        call(None, big, 3, U, U, 0)
    for bad in (-1, 4 * 4 + 1, 1.0, None, True):                          # more rows than 4 labels of 4 image rows have
        with pytest.raises(ValueError, match='span_rows'):
            call(None, U, 3, U, U, bad)
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ValueError, match='tall_rows'):
            call(None, U, 3, U, U, 2, None, bad)


def test_signatures_and_documents():
    sig = {'region_hull': (['labels', 'max_label', 'within', 'return_vertices'], [None, None, False]),
           'hull_shape': (['hull', 'geometry'], []),
           'hull_features': (['labels', 'kept_labels', 'max_label', 'within'], [None, None])}
    for name, (names, defaults) in sig.items():
        p = inspect.signature(getattr(nuclei, name)).parameters
        assert list(p) == names, name
        assert [p[k].default for k in names[len(names) - len(defaults):]] == defaults, name
        assert 'Host syncs: ' in getattr(nuclei, name).__doc__, name
    doc = nuclei.region_hull.__doc__
    for text in ('pixel SQUARES', 'skimage counts', 'cv2 hulls a contour', 'smallest vertex', 'first in hull order', '128 bits', 'strictly convex',
                 'bit-identical'):
        assert text in doc, text
    usage = 'hull_features(L, kept, max_label=n)], 1)'
    assert usage in nuclei.hull_features.__doc__ and usage in nuclei.__doc__
    for cls in (kernels.KernelSpec, kernels.HipKernels):
        assert list(inspect.signature(cls.region_hull).parameters) == ['self', 'labels', 'max_label', 'extents', 'ptr', 'span_rows', 'within',
                                                                      'tall_rows']
        assert list(inspect.signature(cls.region_hull_ptr).parameters) == ['self', 'count', 'extents']
    doc = kernels.KernelSpec.region_hull.__doc__
    for k in range(1, 10):
        assert '\n        %d.  ' % k in doc, k
    for text in ('no host read', 'CGC_EINVAL', 'H * W = 0', 'pixel SQUARES', 'TIE RULE: of', 'TIE RULE: the first edge', '128 bits', '2^93',
                 'bit-identical', 'identical tables', 'lane shuffle'):
        assert text in doc, text
    with pytest.raises(NotImplementedError):
        kernels.KernelSpec().region_hull(None, 1, None, None, 0)
    with pytest.raises(NotImplementedError):
        kernels.KernelSpec().region_hull_ptr(None, None)
    for name in ('README.md', 'DESIGN.md'):
        text = open(os.path.join(ROOT, name)).read()
        assert 'region_hull' in text and 'hull_features' in text, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '## Region hull (csrc/region.hip)' in design
    row = re.search(r'^\| F20 .*$', open(os.path.join(ROOT, 'SURVEY.md')).read(), flags=re.M)
    assert row and 'construct_feature_graph.py:84-88' in row.group(0)


def test_region_hull_ptr_on_the_host():
    """The prefix sum is tensor arithmetic: on host tensors it runs without a GPU."""
    class Table(object):
        _dev = staticmethod(lambda *a: None)
    count = torch.tensor([5, 0, 2, 7], dtype=torch.int32)
    ext = torch.zeros(4, 8, 2, dtype=torch.int32)
    ext[:, 4, 0] = torch.tensor([3, 0, 9, 0])
    ext[:, 4, 1] = torch.tensor([7, 0, 9, 32766])
    ptr = kernels.HipKernels.region_hull_ptr(Table(), count, ext)
    assert ptr.dtype == torch.int64 and ptr.tolist() == [0, 5, 5, 6, 6 + 32767]


# ------------------------------------------------------------------ the library, without a launch
def test_library_refusals(lib):
    einval = -1
    buf = (ctypes.c_int64 * 64)()                                       # any non-NULL address: nothing is launched
    some = ctypes.addressof(buf)

    def spans(labels=some, within=None, wbytes=0, H=4, W=5, max_label=3, extents=some, ptr=some, span_rows=6, out=some):
        return lib.cgc_region_hull_spans(labels, within, wbytes, H, W, max_label, extents, ptr, span_rows, out, None)

    def hull(max_label=3, H=4, extents=some, ptr=some, span_rows=6, spans=some, ws=some, tall_rows=0, count=some, area2=some, diameter2=some,
             ends=some, width_cross=some, width_edge=some, perimeter=some):
        return lib.cgc_region_hull(max_label, H, extents, ptr, span_rows, spans, ws, tall_rows, count, area2, diameter2, ends, width_cross,
                                   width_edge, perimeter, None)

    for H, W in ((32768, 4), (4, 32768), (32768, 32768), (2 ** 30, 1), (1, 2 ** 30), (-1, 5), (4, -1)):
        assert spans(H=H, W=W, span_rows=1) == einval, (H, W)
    for H in (32768, -1, 2 ** 30):
        assert hull(H=H, span_rows=1) == einval
    for bad in (-1, 2 ** 31 - 1):
        assert spans(max_label=bad) == einval and hull(max_label=bad) == einval and lib.cgc_region_hull_ws_bytes(bad, 6) == 0
    for wbytes in (0, 3, 16, -1):
        assert spans(within=some, wbytes=wbytes) == einval
    for rows in (-1, 4 * 4 + 1, 2 ** 40):                               # ptr[R] of 4 labels in 4 image rows is at most 16
        assert spans(span_rows=rows) == einval and hull(span_rows=rows) == einval
    assert spans(H=0, W=3, span_rows=1) == einval and hull(H=0, span_rows=1) == einval
    assert lib.cgc_region_hull_ws_bytes(3, -1) == 0
    for name in ('labels', 'extents', 'ptr', 'out'):
        assert spans(**{name: None}) == einval, name
    for name in ('extents', 'ptr', 'spans', 'ws', 'count', 'area2', 'diameter2', 'ends', 'width_cross', 'width_edge', 'perimeter'):
        assert hull(**{name: None}) == einval, name
    assert hull(tall_rows=-1) == einval
    assert spans(H=0, W=0, span_rows=0, out=None, labels=None) == 0     # an empty image: nothing to launch


def test_constants(lib):
    source = open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'region.hip')).read()
    tall = int(re.search(r'constexpr int HULL_TALL_ROWS = (\d+);', source).group(1))
    assert lib.cgc_region_hull_tall_rows() == tall and 64 <= tall <= 32767
    for S, R in ((0, 1), (6, 4), (1000, 17)):
        assert lib.cgc_region_hull_ws_bytes(R - 1, S) >= 2 * (S + R) * 8       # 2 (h + 1) points of two int32 per label
    side = lib.cgc_region_geometry_max_side() + 1                       # the largest coordinate of a corner
    assert (2 * side * side) ** 2 * (2 * side * side) < 2 ** 128 and (2 * side * side) ** 2 < 2 ** 64      # c^2 |e|^2 in 128 bits, c^2 in 64
    assert not re.search(r'for \(;;\)|while \(', source)                # no loop without a bound in this file
    assert len(re.findall(r'struct RegionSpot \{|struct RegionColumn \{|RegionVerdict region_judge\(|bool region_call\(|void region_launch\(',
                          source)) == 5                                 # the shared pieces are still written once


def test_abi_26_in_the_header_the_prototypes_and_the_library(lib):
    header = open(os.path.join(ROOT, 'include', 'cgc_hip.h')).read()
    assert lib.cgc_abi_version() == _abi.ABI_VERSION == int(re.search(r'#define CGC_ABI_VERSION (\d+)', header).group(1)) >= 26
    assert re.search(r'^ \*  26: region hull', header, flags=re.M) and re.search(r'^/\* ---- F20 ', header, flags=re.M)
    for name in SYMBOLS:
        assert name in _abi.PROTOTYPES and re.search(r'^(int|int64_t) %s\(' % name, header, flags=re.M), name
        assert getattr(lib, name).argtypes == _abi.PROTOTYPES[name]
    assert lib.cgc_region_hull_ws_bytes.restype == ctypes.c_int64
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert _abi.PROTOTYPES['cgc_region_hull_spans'] == [P, P, I, I, I, I, P, P, L, P, P]
    assert _abi.PROTOTYPES['cgc_region_hull'] == [I, I, P, P, L, P, P, I, P, P, P, P, P, P, P, P]
    assert 'region_hull' in kernels.KernelSpec.__dict__
