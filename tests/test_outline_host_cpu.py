"""CPU: the host side of region outlines (csrc/outline.hip; cgc_net_amd.nuclei.region_outlines, outline_tables, outline_polygons;
cgc_net_amd.evalio.outlines_to_geojson; kernels.HipKernels.region_outlines): what is refused before any launch, what the library
refuses without launching, the contract's items, the ABI, and the polygon and GeoJSON layers on tables made by tests/outline_ref.py.

As in tests/test_hull_host_cpu.py the "on the GPU" refusal is lifted and the kernel table fails the test when it is asked for."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import _abi, evalio, kernels, nuclei

import outline_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('cgc_region_outline_rounds', 'cgc_region_outlines_ws_bytes', 'cgc_region_outline_count', 'cgc_region_outline_cracks',
           'cgc_region_outline_loops', 'cgc_region_outline_keys', 'cgc_region_outline_tables', 'cgc_region_outline_scatter',
           'cgc_region_outline_compact')


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


def labels(*shape, dtype=torch.int32):
    return torch.ones(shape or (4, 5), dtype=dtype)


def view(H, W, dtype=torch.int32):
    """An image of any size without memory behind it."""
    return torch.zeros(1, 1, dtype=dtype).expand(H, W)


def outlines_of(a, top, connectivity=1, mode='corners', background=False):
    """A RegionOutlines of host tensors from the restatement."""
    t = ref.outlines(a, top, connectivity, None, mode, background)
    return nuclei.RegionOutlines(*[torch.from_numpy(t[k]) for k in ref.TABLES], meta=torch.zeros(1, dtype=torch.int32))


# ------------------------------------------------------------------ the public function
def test_only_tensors_on_the_gpu():
    for bad in (labels(), np.ones((4, 5), np.int32), None, [[1, 2]]):
        with pytest.raises(TypeError):
            nuclei.region_outlines(bad)


def test_form_of_the_labels_and_sizes(no_launch):
    f = nuclei.region_outlines
    for dtype in (torch.bool, torch.float32, torch.float64):
        with pytest.raises(TypeError):
            f(labels(dtype=dtype), max_label=1)
    for shape in ((20,), (4, 5, 1), (1, 4, 5)):
        with pytest.raises(ValueError):
            f(labels(*shape), max_label=1)
    for bad in (-1, 2 ** 31 - 1, 1.0, True, '3'):
        with pytest.raises(ValueError, match='max_label|label values'):
            f(labels(), max_label=bad)
    with pytest.raises(ValueError, match='negative'):
        f(labels() - 2)
    for H, W in ((32768, 4), (4, 32768), (65535, 3)):
        with pytest.raises(ValueError, match='sides up to 32767'):
            f(view(H, W), max_label=1)
    for H, W in ((32767, 16385), (16385, 32767), (23171, 23171)):
        assert H * W >= 2 ** 29
        with pytest.raises(ValueError, match=r'fewer than 2\^29 pixels'):
            f(view(H, W), max_label=1)
    assert nuclei.OUTLINE_MAX_PIXELS == 2 ** 29


def test_mode_connectivity_and_within(no_launch):
    f = nuclei.region_outlines
    for bad in (0, 3, 4, 8, None, '1', True, 1.5):
        with pytest.raises(ValueError, match='connectivity must be 1 or 2'):
            f(labels(), max_label=1, connectivity=bad)
    for bad in ('corner', 'crack', 'CORNERS', None, 0, ''):
        with pytest.raises(ValueError, match="mode must be 'corners' or 'cracks'"):
            f(labels(), max_label=1, mode=bad)
    for shape in ((5, 4), (4, 6), (4, 5, 1), (20,)):
        with pytest.raises(ValueError):
            f(labels(), max_label=1, within=torch.ones(shape, dtype=torch.uint8))
    with pytest.raises(TypeError):
        f(labels(), max_label=1, within=torch.ones(4, 5))


class Untouchable(object):
    """Stands in for a tensor: any use but its shape fails the test."""
    shape = (4, 5)

    def __getattr__(self, name):
        pytest.fail('a tensor was touched (%s)' % name)


def test_the_kernel_table_refuses_bad_parameters_before_any_tensor():
    call = kernels.HipKernels.region_outlines
    U = Untouchable()
    for bad in (-1, 2 ** 31 - 1, None, 2.0, True):
        with pytest.raises(ValueError, match='max_label'):
            call(None, U, bad)
    big = Untouchable()
    big.shape = (32768, 2)
    with pytest.raises(ValueError, match='32767'):
        call(None, big, 3)
    big.shape = (32767, 32767)
    with pytest.raises(ValueError, match=r'2\^29'):
        call(None, big, 3)
    for bad in (0, 3, True, None):
        with pytest.raises(ValueError, match='connectivity'):
            call(None, U, 3, bad)
    with pytest.raises(ValueError, match='mode'):
        call(None, U, 3, 1, None, 'polygon')


def test_signatures_and_documents():
    p = inspect.signature(nuclei.region_outlines).parameters
    assert list(p) == ['labels', 'max_label', 'connectivity', 'within', 'mode', 'background']
    assert [p[k].default for k in list(p)[1:]] == [None, 1, None, 'corners', False]
    assert list(inspect.signature(nuclei.outline_tables).parameters) == ['outlines']
    p = inspect.signature(nuclei.outline_polygons).parameters
    assert list(p) == ['outlines', 'kept_labels', 'scale'] and p['kept_labels'].default is None and p['scale'].default is None
    p = inspect.signature(evalio.outlines_to_geojson).parameters
    assert list(p) == ['polygons', 'path', 'properties'] and p['properties'].default is None
    for f in (nuclei.region_outlines, nuclei.outline_tables, nuclei.outline_polygons):
        assert 'Host syncs: ' in f.__doc__, f.__name__
    assert 'connectivity 2' in nuclei.outline_polygons.__doc__ and 'two reads' in nuclei.region_outlines.__doc__
    assert nuclei.RegionOutlines._fields == ref.TABLES + ('meta',)
    assert nuclei.OutlineTables._fields == ('outer', 'holes', 'cracks', 'area2')
    for cls in (kernels.KernelSpec, kernels.HipKernels):
        assert list(inspect.signature(cls.region_outlines).parameters) == ['self', 'labels', 'max_label', 'connectivity', 'within', 'mode',
                                                                          'background']
    doc = kernels.KernelSpec.region_outlines.__doc__
    for k in range(1, 10):
        assert '\n        %d.  ' % k in doc, k
    for text in ('items 1, 3 and 4 of', 'region_statistics', '32767', 'H * W < 2^29', 'CGC_EINVAL', '4 (y W + x) + side', '0 top, 1', 'top east',
                 'TIE RULE, connectivity 1', 'TIE RULE, connectivity 2', 'permutation', 'smallest id', 'ordered by start id', 'unique',
                 "mode='cracks'", "mode='corners'", 'NOT the start', 'positive', 'negative for a hole', 'HOST READS: two', 'number of cracks',
                 'number of loops', 'bit-identical', 'no loop is walked', 'ceil(log2(n_cracks))'):
        assert text in doc, text
    with pytest.raises(NotImplementedError):
        kernels.KernelSpec().region_outlines(None, 1)
    for name in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, name)).read()
        assert 'region_outlines' in text, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '## Region outlines (csrc/outline.hip)' in design and 'outlines_to_geojson' in design
    assert re.search(r'^\| F22 .*$', open(os.path.join(ROOT, 'SURVEY.md')).read(), flags=re.M)
    assert os.path.exists(os.path.join(ROOT, 'tools', 'outline_bench.py'))


# ------------------------------------------------------------------ tables, polygons, GeoJSON
def ring_image():
    b = np.zeros((9, 10), np.int32)
    b[1:8, 1:9] = 1
    b[2:7, 2:8] = 0                                                       # a hole of 5 x 6
    b[3:6, 3:6] = 1                                                       # an island of 3 x 3 in it
    b[4, 4] = 0                                                           # with a hole of its own
    b[3:6, 6] = 2                                                         # and another label beside the island
    return b


def test_outline_tables_on_hand_tables():
    b = ring_image()
    for connectivity in (1, 2):
        o = outlines_of(b, 3, connectivity)
        t = nuclei.outline_tables(o)
        assert isinstance(t, nuclei.OutlineTables) and all(v.dtype == torch.int32 and tuple(v.shape) == (4,) for v in t)
        for got, want in zip(t, ref.per_label(ref.outlines(b, 3, connectivity), 3)):
            assert got.tolist() == want.tolist()
        assert t.outer.tolist() == [0, 2, 1, 0] and t.holes.tolist() == [0, 2, 0, 0]
        assert t.area2.tolist() == [0, 2 * int((b == 1).sum()), 6, 0]
    with pytest.raises(TypeError, match='RegionOutlines'):
        nuclei.outline_tables(tuple(o))


def test_outline_polygons_nests_holes_under_their_rings():
    b = ring_image()
    for connectivity in (1, 2):
        for mode in ('corners', 'cracks'):
            o = outlines_of(b, 3, connectivity, mode)
            polys = nuclei.outline_polygons(o)
            assert [len(p) for p in polys] == [0, 2, 1, 0]
            big, island = polys[1]
            assert [len(r) for r in (big, island)] == [2, 2]              # each outer ring with ITS hole, the island's not under the big one
            assert all(r.dtype == np.float64 and r.shape[1] == 2 for r in big + island)
            if mode == 'corners':
                assert big[0].tolist() == [[1, 1], [9, 1], [9, 8], [1, 8]]            # (x, y)
                assert sorted(big[1].tolist()) == [[2, 2], [2, 7], [8, 2], [8, 7]]
                assert island[0].tolist() == [[3, 3], [6, 3], [6, 6], [3, 6]]
                assert sorted(island[1].tolist()) == [[4, 4], [4, 5], [5, 4], [5, 5]]
                assert polys[2][0][0].tolist() == [[6, 3], [7, 3], [7, 6], [6, 6]]
    kept = nuclei.outline_polygons(outlines_of(b, 3), kept_labels=[2, 1, 2])
    assert [len(p) for p in kept] == [1, 2, 1]
    same = nuclei.outline_polygons(outlines_of(b, 3), kept_labels=torch.tensor([2, 1, 2], dtype=torch.int32))
    assert all(np.array_equal(x, y) for p, q in zip(kept, same) for rx, ry in zip(p, q) for x, y in zip(rx, ry))
    for bad in ([4], [-1], torch.tensor([7])):
        with pytest.raises(ValueError, match='kept_labels'):
            nuclei.outline_polygons(outlines_of(b, 3), kept_labels=bad)
    for bad in (torch.tensor([1.0]), torch.tensor([[1]]), 3, ['a']):
        with pytest.raises(TypeError, match='kept_labels'):
            nuclei.outline_polygons(outlines_of(b, 3), kept_labels=bad)
    with pytest.raises(TypeError, match='RegionOutlines'):
        nuclei.outline_polygons(None)


def test_a_hole_that_touches_its_ring_with_connectivity_2():
    a = np.array([[1, 1, 1], [1, 0, 1], [1, 1, 0]], np.int32)            # the hole (1, 1) touches the outside at corner (2, 2)
    one = nuclei.outline_polygons(outlines_of(a, 1, 1))[1]
    assert [len(p) for p in one] == [1]                                   # connectivity 1: the "hole" is open, one loop through (2, 2) twice
    two = nuclei.outline_polygons(outlines_of(a, 1, 2))[1]
    assert [len(p) for p in two] == [2] and sorted(two[0][1].tolist()) == [[1, 1], [1, 2], [2, 1], [2, 2]]


def test_scale_follows_scale_points():
    b = ring_image()
    o = outlines_of(b, 3)
    plain = nuclei.outline_polygons(o)
    sizes = ((9, 10), (27, 25))
    scaled = nuclei.outline_polygons(o, scale=sizes)
    for p, q in zip(plain, scaled):
        for rings, rings2 in zip(p, q):
            for r, r2 in zip(rings, rings2):
                centres = torch.from_numpy(r[:, ::-1].copy()) - 0.5       # the pixel centre half a pixel before a corner, as (row, column)
                want = nuclei.scale_points(centres, *sizes) + 0.5
                assert np.allclose(r2[:, ::-1], want.numpy(), rtol=0, atol=1e-12)
                assert np.array_equal(r2, r * np.array([25 / 10.0, 27 / 9.0]))
    for bad in (3, ((9, 10),), ((9, 10), (0, 5)), ((9, 10), (2.5, 5)), 'ab'):
        with pytest.raises(ValueError, match='scale'):
            nuclei.outline_polygons(o, scale=bad)


def test_geojson(tmp_path):
    b = ring_image()
    polys = nuclei.outline_polygons(outlines_of(b, 3), kept_labels=[1, 2, 3])
    path = str(tmp_path / 'layers' / 'nuclei.geojson')
    props = [{'class': 'tumour'}, {'class': 'stroma', 'label_index': 7}, {'class': 'none'}]
    made = evalio.outlines_to_geojson(polys, path, props)
    read = json.load(open(path))
    assert read == made and read['type'] == 'FeatureCollection'
    feats = read['features']
    assert len(feats) == 3 and all(f['type'] == 'Feature' and f['geometry']['type'] == 'Polygon' for f in feats)
    assert [f['properties'] for f in feats] == [{'class': 'tumour', 'label_index': 0}] * 2 + [{'class': 'stroma', 'label_index': 7}]
    for f in feats:
        for ring in f['geometry']['coordinates']:
            assert ring[0] == ring[-1] and len(ring) >= 5                 # closed
    big, island, other = (f['geometry']['coordinates'] for f in feats)
    assert len(big) == 2 and len(island) == 2 and len(other) == 1         # a hole sits under its outer ring, as an interior ring
    assert big[0] == [[1, 1], [9, 1], [9, 8], [1, 8], [1, 1]]
    xs, ys = [p[0] for p in big[1]], [p[1] for p in big[1]]
    assert (min(xs), max(xs), min(ys), max(ys)) == (2, 8, 2, 7)           # inside the outer ring
    plain = evalio.outlines_to_geojson(polys, str(tmp_path / 'plain.geojson'))
    assert [f['properties'] for f in plain['features']] == [{'label_index': 0}, {'label_index': 0}, {'label_index': 1}]
    with pytest.raises(ValueError, match='properties'):
        evalio.outlines_to_geojson(polys, path, props[:2])
    source = inspect.getsource(evalio.outlines_to_geojson)
    assert 'import json' in source and 'networkx' not in source


# ------------------------------------------------------------------ the library, without a launch
def test_library_refusals(lib):
    einval = -1
    buf = (ctypes.c_int64 * 64)()
    some = ctypes.addressof(buf)

    def count(labels=some, within=None, wbytes=0, H=4, W=5, max_label=3, background=0, mask=some, cnt=some, meta=some):
        return lib.cgc_region_outline_count(labels, within, wbytes, H, W, max_label, background, mask, cnt, meta, None)

    def cracks(labels=some, within=None, wbytes=0, H=4, W=5, max_label=3, connectivity=1, mask=some, off=some, n=6, crack=some, succ=some):
        return lib.cgc_region_outline_cracks(labels, within, wbytes, H, W, max_label, connectivity, mask, off, n, crack, succ, None)

    for H, W in ((32768, 4), (4, 32768), (32767, 32767), (32767, 16385), (-1, 5), (4, -1), (2 ** 30, 1)):
        assert count(H=H, W=W) == einval and cracks(H=H, W=W) == einval, (H, W)
    for bad in (-1, 2 ** 31 - 1):
        assert count(max_label=bad) == einval and cracks(max_label=bad) == einval
    for wbytes in (0, 3, 16, -1):
        assert count(within=some, wbytes=wbytes) == einval and cracks(within=some, wbytes=wbytes) == einval
    for bad in (0, 3, -1):
        assert cracks(connectivity=bad) == einval
    for name in ('labels', 'mask', 'cnt', 'meta'):
        assert count(**{name: None}) == einval, name
    for name in ('labels', 'mask', 'off', 'crack', 'succ'):
        assert cracks(**{name: None}) == einval, name
    for n in (-1, 4 * 20 + 1, 2 ** 31):
        assert cracks(n=n) == einval
    assert cracks(n=0, crack=None, succ=None) == 0                        # nothing to do
    for n in (-1, 2 ** 31):
        assert lib.cgc_region_outlines_ws_bytes(n) == 0 and lib.cgc_region_outline_rounds(n) == einval
        assert lib.cgc_region_outline_loops(n, some, some, some, some, None) == einval
        assert lib.cgc_region_outline_keys(n, 1, some, some, some, some, some, None) == einval
        assert lib.cgc_region_outline_tables(n, 1, some, some, some, some, some, some, some, some, None) == einval
        assert lib.cgc_region_outline_scatter(n, 1, 5, some, some, some, some, some, some, some, some, None, None) == einval
        assert lib.cgc_region_outline_compact(n, 1, some, some, some, some, None) == einval
    assert lib.cgc_region_outline_loops(6, None, some, some, some, None) == einval
    assert lib.cgc_region_outline_loops(6, some, None, some, some, None) == einval
    assert lib.cgc_region_outline_loops(0, None, None, None, None, None) == 0
    for loops in (-1, 7):                                                 # more loops than cracks
        assert lib.cgc_region_outline_keys(6, loops, some, some, some, some, some, None) == einval
        assert lib.cgc_region_outline_tables(6, loops, some, some, some, some, some, some, some, some, None) == einval
        assert lib.cgc_region_outline_scatter(6, loops, 5, some, some, some, some, some, some, some, some, None, None) == einval
        assert lib.cgc_region_outline_compact(6, loops, some, some, some, some, None) == einval
    assert lib.cgc_region_outline_keys(6, 2, some, some, some, some, None, None) == einval
    assert lib.cgc_region_outline_tables(6, 2, some, some, some, some, some, some, None, some, None) == einval
    for W in (0, 32768):
        assert lib.cgc_region_outline_scatter(6, 2, W, some, some, some, some, some, some, some, some, None, None) == einval
    assert lib.cgc_region_outline_scatter(6, 2, 5, some, some, some, some, some, some, some, None, None, None) == einval
    assert lib.cgc_region_outline_compact(6, 2, some, some, some, None, None) == einval
    assert lib.cgc_region_outline_keys(6, 0, None, None, None, None, None, None) == 0
    assert lib.cgc_region_outline_compact(6, 0, None, None, None, None, None) == 0


def test_rounds_and_workspace(lib):
    assert [lib.cgc_region_outline_rounds(n) for n in (0, 1, 2, 3, 4, 5, 3906, 4096, 4097, 32130, 2 ** 31 - 1)] == \
        [0, 0, 1, 2, 2, 3, 12, 12, 13, 15, 31]
    for n in (0, 1, 100, 3906, 10 ** 6):
        assert lib.cgc_region_outlines_ws_bytes(n) >= 16 * n              # two buffers of 64-bit pairs
    source = open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'outline.hip')).read()
    assert not re.search(r'for \(;;\)|while \(', source)                  # no loop without a bound: no loop is walked
    assert 'image_common.hpp' in source and 'image_nonzero(' in source and 'bad_connectivity(' in source and 'Carver' in source
    assert 'outline.hip' in open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'Makefile')).read()


def test_abi_28_in_the_header_the_prototypes_and_the_library(lib):
    header = open(os.path.join(ROOT, 'include', 'cgc_hip.h')).read()
    assert lib.cgc_abi_version() == _abi.ABI_VERSION == int(re.search(r'#define CGC_ABI_VERSION (\d+)', header).group(1)) >= 28
    assert re.search(r'^ \*  28: region outlines', header, flags=re.M) and re.search(r'^/\* ---- F22 ', header, flags=re.M)
    for name in SYMBOLS:
        assert name in _abi.PROTOTYPES and re.search(r'^(int|int64_t) %s\(' % name, header, flags=re.M), name
        assert getattr(lib, name).argtypes == _abi.PROTOTYPES[name]
    assert lib.cgc_region_outlines_ws_bytes.restype == ctypes.c_int64
    assert 'region_outlines' in kernels.KernelSpec.__dict__ and 'region_outlines' in kernels.HipKernels.__dict__
