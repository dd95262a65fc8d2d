"""CPU: the host side of the region statistics (csrc/region.hip; cgc_net_amd.nuclei.region_statistics, region_histogram,
region_quantiles, region_mean_std, ring_labels, stain_features; kernels.HipKernels.region_*): what the public functions refuse before
any launch, and what the library refuses without launching.

As in tests/test_rank_host_cpu.py the tests lift the "on the GPU" refusal (``on_gpu=False``) and replace the kernel table by one
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

import region_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('cgc_region_tile_side', 'cgc_region_table_slots', 'cgc_region_ws_bytes', 'cgc_region_moments', 'cgc_region_histogram',
           'cgc_region_quantiles')


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


def calls():
    """The three functions that take (labels, values, max_label=, within=)."""
    return [('region_statistics', nuclei.region_statistics),
            ('region_histogram', nuclei.region_histogram),
            ('region_quantiles', lambda lab, val, **kw: nuclei.region_quantiles(lab, val, 0.5, **kw))]


# ------------------------------------------------------------------ the public functions
def test_only_tensors_on_the_gpu():
    for name, fn in calls():
        for bad in (labels(), np.ones((4, 5), np.int32), None, [[1, 2]]):
            with pytest.raises(TypeError):
                fn(bad, image())
    with pytest.raises(TypeError):
        nuclei.stain_features(labels(), tile(), torch.ones(2, dtype=torch.int32))
    with pytest.raises(TypeError):
        nuclei.ring_labels(labels(), 3)


def test_form_of_labels_and_values(no_launch):
    for name, fn in calls():
        for dtype in (torch.bool, torch.float32, torch.float16):
            with pytest.raises(TypeError):
                fn(labels(dtype=dtype), image(), max_label=1)
        for dtype in (torch.int64, torch.float32, torch.float64, torch.float16):
            with pytest.raises(TypeError):
                fn(labels(), image(dtype=dtype), max_label=1)
        for bad in (np.ones((4, 5), np.uint8), None, 3):
            with pytest.raises(TypeError):
                fn(labels(), bad, max_label=1)
        for shape in ((3, 4, 5), (20,)):
            with pytest.raises(ValueError):
                fn(labels(*shape), image(*shape), max_label=1)
        for shape in ((5, 4), (4, 6), (4, 5, 1), (20,)):
            with pytest.raises(ValueError):
                fn(labels(), image(*shape), max_label=1)
        with pytest.raises(ValueError, match='device'):
            fn(labels(), torch.ones(4, 5, dtype=torch.uint8, device='meta'), max_label=1)
    for dtype in (torch.int8, torch.int16, torch.int32):                # histograms and quantiles are uint8 / bool only
        for name, fn in calls()[1:]:
            with pytest.raises(TypeError):
                fn(labels(), image(dtype=dtype), max_label=1)


def test_form_of_within_and_max_label(no_launch):
    for name, fn in calls():
        for other in (image(5, 4), image(4, 6), image(4, 5, 1), image(20)):
            with pytest.raises(ValueError):
                fn(labels(), image(), max_label=1, within=other)
        with pytest.raises(ValueError, match='device'):
            fn(labels(), image(), max_label=1, within=torch.zeros(4, 5, dtype=torch.uint8, device='meta'))
        for bad in (image(dtype=torch.float32), np.ones((4, 5), bool), 1):
            with pytest.raises(TypeError):
                fn(labels(), image(), max_label=1, within=bad)
        for bad in (-1, -2 ** 31, 2 ** 31 - 1, 2 ** 40, 1.0, '3', True, (1,)):
            with pytest.raises(ValueError, match='max_label|label values'):
                fn(labels(), image(), max_label=bad)
        # without max_label the range is read from the labels, here on the host: negative labels are refused before any launch
        with pytest.raises(ValueError, match='negative'):
            fn(labels() - 2, image())
        with pytest.raises(ValueError, match='2\\^31'):
            fn(labels(dtype=torch.int64) * (2 ** 31 - 1), image())


def test_quantiles_go_through_rank_q10k(no_launch, monkeypatch):
    for bad in (-0.001, 1.0001, 2, -1, float('nan'), float('inf'), True, None, '0.5', 1 + 0j, Fraction(10001, 10000), np.array([0.5])):
        with pytest.raises(ValueError, match='q'):
            nuclei.region_quantiles(labels(), image(), bad, max_label=1)
        with pytest.raises(ValueError, match='q'):
            nuclei.region_quantiles(labels(), image(), [0.5, bad], max_label=1)
    for bad in ([], (), [0.1] * 9, tuple([0.5] * 20)):
        with pytest.raises(ValueError, match='1 to 8 quantiles'):
            nuclei.region_quantiles(labels(), image(), bad, max_label=1)
    assert nuclei.REGION_MAX_QUANTILES == kernels.REGION_MAX_QUANTILES == ref.MAX_QUANTILES == 8
    seen = []
    real = nuclei.rank_q10k
    monkeypatch.setattr(nuclei, 'rank_q10k', lambda q: seen.append(q) or real(q))
    assert nuclei._q10k_list('f', [0, 0.5, Fraction(1, 3), 1]) == ([0, 5000, 3333, 10000], False)
    assert nuclei._q10k_list('f', 0.05) == ([500], True) and nuclei._q10k_list('f', np.float32(0.5)) == ([5000], True)
    assert seen == [0, 0.5, Fraction(1, 3), 1, 0.05, np.float32(0.5)]
    assert nuclei.STAIN_FEATURE_QUANTILES == (1000, 5000, 9000)


def test_region_mean_std_on_the_host():
    RS = nuclei.RegionStats
    assert RS._fields == ('count', 'sum', 'sumsq', 'min', 'max', 'argmin', 'argmax')
    i32, i64 = torch.int32, torch.int64
    z = torch.zeros(4, dtype=i32)
    st = RS(torch.tensor([0, 4, 2, 1], dtype=i32), torch.tensor([0, 40, -6, 255], dtype=i64), torch.tensor([0, 400, 26, 65025], dtype=i64),
            z, z, z, z)
    mean, std = nuclei.region_mean_std(st)
    assert mean.dtype == std.dtype == torch.float32
    assert mean.tolist() == [0.0, 10.0, -3.0, 255.0] and std.tolist() == [0.0, 0.0, 2.0, 0.0]      # (-1, -5): mean -3, variance 4
    with pytest.raises(ValueError, match='sumsq'):
        nuclei.region_mean_std(st._replace(sumsq=None))
    for bad in (None, tuple(st), 3):
        with pytest.raises(TypeError):
            nuclei.region_mean_std(bad)


def test_stain_features_refusals(no_launch):
    kept = torch.ones(2, dtype=torch.int32)
    f = nuclei.stain_features
    for bad in (labels(dtype=torch.bool), labels(dtype=torch.float32)):
        with pytest.raises(TypeError):
            f(bad, tile(), kept, max_label=1)
    for bad in (np.ones((4, 5, 3), np.uint8), None):
        with pytest.raises(TypeError):
            f(labels(), bad, kept, max_label=1)
    with pytest.raises(TypeError):
        f(labels(), tile().to(torch.int32), kept, max_label=1)
    for bad in (tile(4, 5), tile(4, 5, 4), tile(5, 4, 3), tile(4, 6, 3)):
        with pytest.raises(ValueError):
            f(labels(), bad, kept, max_label=1)
    for bad in ([1, 2], None, np.ones(2, np.int32), kept.to(torch.float32), kept.to(torch.int16)):
        with pytest.raises(TypeError, match='kept_labels'):
            f(labels(), tile(), bad, max_label=1)
    for bad in (kept.reshape(1, 2), kept.to('meta')):
        with pytest.raises(ValueError, match='kept_labels'):
            f(labels(), tile(), bad, max_label=1)
    for bad in (-1, -0.5, float('nan'), True, None, '6'):
        with pytest.raises(ValueError, match='ring'):
            f(labels(), tile(), kept, ring=bad, max_label=1)
    with pytest.raises(ValueError, match='order'):
        f(labels(), tile(), kept, order='gbr', max_label=1)
    for bad in (-1, 2 ** 31 - 1, 1.5, True):
        with pytest.raises(ValueError):
            f(labels(), tile(), kept, max_label=bad)
    assert len(nuclei.STAIN_FEATURE_NAMES) == 16 == len(set(nuclei.STAIN_FEATURE_NAMES))
    assert nuclei.STAIN_FEATURE_NAMES[:4] == ('hematoxylin_mean', 'hematoxylin_std', 'hematoxylin_median', 'hematoxylin_range')
    assert all(n.startswith('ring_') for n in nuclei.STAIN_FEATURE_NAMES[8:]) and nuclei.STAIN_FEATURE_NAMES[12] == 'ring_eosin_mean'


# ------------------------------------------------------------------ the kernel table
class Untouchable(object):
    """Stands in for a tensor: any use fails the test."""

    def __getattr__(self, name):
        pytest.fail('a tensor was touched (%s)' % name)


def test_the_kernel_table_refuses_bad_parameters_before_any_tensor():
    for call in (kernels.HipKernels.region_statistics, kernels.HipKernels.region_histogram):
        for bad in (-1, 2 ** 31 - 1, None, 2.0, True, '1'):
            with pytest.raises(ValueError, match='max_label'):
                call(None, Untouchable(), Untouchable(), bad)
    call = kernels.HipKernels.region_quantiles
    for bad in ([], [0] * 9, None, 5000):
        with pytest.raises(ValueError, match='q10k'):
            call(None, Untouchable(), bad)
    for bad in (-1, 10001, 0.5, None, True, '5000'):
        with pytest.raises(ValueError, match='q10k'):
            call(None, Untouchable(), [5000, bad])
    for dtype in (torch.bool, torch.int64, torch.float32):
        with pytest.raises(TypeError, match='values'):
            kernels.HipKernels.region_statistics(None, Untouchable(), torch.ones(2, 2, dtype=dtype), 3)
    for dtype in (torch.bool, torch.int8, torch.int16, torch.int32):
        with pytest.raises(TypeError, match='values'):
            kernels.HipKernels.region_histogram(None, Untouchable(), torch.ones(2, 2, dtype=dtype), 3)
    assert kernels.REGION_VALUE_DTYPES == {torch.uint8: (1, 0), torch.int8: (1, 1), torch.int16: (2, 1), torch.int32: (4, 1)}


def test_signatures_and_documents():
    sig = {'region_statistics': (['labels', 'values', 'max_label', 'within'], [None, None]),
           'region_histogram': (['labels', 'values', 'max_label', 'within'], [None, None]),
           'region_quantiles': (['labels', 'values', 'q', 'max_label', 'within'], [None, None]),
           'region_mean_std': (['stats'], []),
           'ring_labels': (['labels', 'distance', 'within'], [None]),
           'stain_features': (['labels', 'tile', 'kept_labels', 'stains', 'order', 'ring', 'max_label'], [None, 'bgr', 0, None])}
    for name, (names, defaults) in sig.items():
        p = inspect.signature(getattr(nuclei, name)).parameters
        assert list(p) == names, name
        assert [p[k].default for k in names[len(names) - len(defaults):]] == defaults, name
        assert 'Host syncs: ' in getattr(nuclei, name).__doc__, name
    assert 'inscribed radius squared' in nuclei.region_statistics.__doc__
    for cls in (kernels.KernelSpec, kernels.HipKernels):
        assert list(inspect.signature(cls.region_statistics).parameters) == ['self', 'labels', 'values', 'max_label', 'within']
        assert list(inspect.signature(cls.region_histogram).parameters) == ['self', 'labels', 'values', 'max_label', 'within']
        assert list(inspect.signature(cls.region_quantiles).parameters) == ['self', 'hist', 'q10k']
    for name, items in (('region_statistics', 9), ('region_histogram', 6), ('region_quantiles', 5)):
        doc = getattr(kernels.KernelSpec, name).__doc__
        for k in range(1, items + 1):
            assert '\n        %d.  ' % k in doc, (name, k)
        assert 'F17' in doc and 'no host read' in doc
    doc = kernels.KernelSpec.region_statistics.__doc__
    for text in ('SMALLEST index', 'argmin = argmax = -1', 'meta[0]', 'CGC_EINVAL', 'H * W = 0', 'bit-identical', 'region_slots', '64-bit key'):
        assert text in doc, text
    assert 'min(n - 1, floor(n * q10k / 10000))' in kernels.KernelSpec.region_quantiles.__doc__
    with pytest.raises(NotImplementedError):
        kernels.KernelSpec().region_statistics(None, None, 1)
    with pytest.raises(NotImplementedError):
        kernels.KernelSpec().region_histogram(None, None, 1)
    with pytest.raises(NotImplementedError):
        kernels.KernelSpec().region_quantiles(None, [0])
    for name in ('README.md', 'DESIGN.md'):
        text = open(os.path.join(ROOT, name)).read()
        assert 'region_statistics' in text and 'stain_features' in text and 'region_quantiles' in text, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '## Region statistics (csrc/region.hip)' in design and 'region_bench.json' in design
    assert re.search(r'^\| F17 \|', open(os.path.join(ROOT, 'SURVEY.md')).read(), flags=re.M)
    assert 'region.hip' in open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'Makefile')).read()
    assert os.path.exists(os.path.join(ROOT, 'tools', 'region_bench.py'))
    for text in ('features, cen, kept = nucleus_features(L, gray, max_label=n)',
                 'x = torch.cat([features, stain_features(L, tile, kept, ring=6, max_label=n)], 1)', 'graph_item(x, cen, y)',
                 'region_statistics(L, distance_transform(L != 0))'):
        assert text in nuclei.__doc__, text


# ------------------------------------------------------------------ the library, without a launch
def test_library_refusals(lib):
    einval = -1
    buf = (ctypes.c_int64 * 64)()                                       # any non-NULL, 16-byte aligned address: nothing is launched
    some = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16

    # cgc_region_moments(labels, values, vbytes, vsigned, within, wbytes, H, W, max_label, ws, count, sum, sumsq, min, max, argmin, argmax, meta, stream)
    def moments(labels=some, values=some, vbytes=1, vsigned=0, within=None, wbytes=0, H=4, W=5, max_label=3, ws=some, count=some, total=some,
                sumsq=some, mn=some, mx=some, amin=some, amax=some, meta=some):
        return lib.cgc_region_moments(labels, values, vbytes, vsigned, within, wbytes, H, W, max_label, ws, count, total, sumsq, mn, mx, amin,
                                      amax, meta, None)

    # cgc_region_histogram(labels, values, within, wbytes, H, W, max_label, hist, meta, stream)
    def hist(labels=some, values=some, within=None, wbytes=0, H=4, W=5, max_label=3, hist=some, meta=some):
        return lib.cgc_region_histogram(labels, values, within, wbytes, H, W, max_label, hist, meta, None)

    for fn in (moments, hist):
        for H, W in ((-1, 5), (4, -1), (-4, -5), (2 ** 16, 2 ** 15), (2 ** 31 - 1, 2), (46341, 46341)):
            assert fn(H=H, W=W) == einval
        for bad in (-1, -2 ** 31, 2 ** 31 - 1):
            assert fn(max_label=bad) == einval
            assert fn(H=0, W=0, max_label=bad) == einval
        for wbytes in (0, 3, 5, 16, -1):
            assert fn(within=some, wbytes=wbytes) == einval
        assert fn(labels=None) == einval and fn(values=None) == einval and fn(meta=None) == einval
    for vbytes, vsigned in ((0, 0), (3, 1), (8, 1), (2, 0), (4, 0), (1, 2), (1, -1), (-1, 1), (16, 0)):
        assert moments(vbytes=vbytes, vsigned=vsigned) == einval, (vbytes, vsigned)
    assert moments(vbytes=4, vsigned=1) == einval                       # sumsq asked for 4-byte values
    for name in ('ws', 'count', 'total', 'mn', 'mx', 'amin', 'amax'):
        assert moments(**{name: None}) == einval, name
        assert moments(H=0, W=7, **{name: None}) == einval, name
    assert hist(hist=None) == einval and hist(H=0, W=0, hist=None) == einval
    assert lib.cgc_region_ws_bytes(-1) == 0 == lib.cgc_region_ws_bytes(2 ** 31 - 1)
    assert lib.cgc_region_ws_bytes(0) == 512 and lib.cgc_region_ws_bytes(99) == 2 * 1024      # two tables of 8 bytes per row, 256-aligned

    # cgc_region_quantiles(hist, rows, q10k, nq, out, stream)
    def quant(h=some, rows=3, q=(5000,), nq=None, out=some):
        arr = (ctypes.c_int * max(len(q), 1))(*q)
        return lib.cgc_region_quantiles(h, rows, arr, len(q) if nq is None else nq, out, None)

    for rows in (-1, 2 ** 31, 2 ** 40):
        assert quant(rows=rows) == einval
    for nq in (0, -1, 9, 100):
        assert quant(q=(1,) * 8, nq=nq) == einval
    for bad in (-1, 10001, 2 ** 20, -2 ** 31):
        assert quant(q=(5000, bad)) == einval and quant(q=(bad,)) == einval and quant(rows=0, q=(bad,)) == einval
    assert quant(h=None) == einval and quant(out=None) == einval and quant(h=some + 4) == einval      # hist must be 16-byte aligned
    assert lib.cgc_region_quantiles(some, 3, None, 1, some, None) == einval
    assert quant(rows=0) == 0 and quant(rows=0, h=None, out=None) == 0   # no rows: nothing to do


def test_tile_geometry_and_constants(lib):
    source = open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'region.hip')).read()

    def constant(name):
        return int(re.search(r'constexpr int %s = (\d+);' % name, source).group(1))

    assert lib.cgc_region_tile_side() == constant('REGION_TILE') == 64
    bits = constant('REGION_SLOT_BITS')
    assert lib.cgc_region_table_slots() == 1 << bits == 64
    assert 1 <= constant('REGION_PROBES') <= lib.cgc_region_table_slots()      # a probe sequence is bounded by the slot count
    assert constant('REGION_MAX_Q') == kernels.REGION_MAX_QUANTILES == 8
    assert lib.cgc_region_tile_side() ** 2 < 2 ** 16                    # a 16-bit bin holds a tile of one label and one value
    assert not re.search(r'for \(;;\)|while \(', source)                # no loop without a bound in this file


def test_abi_23_in_the_header_the_prototypes_and_the_library(lib):
    header = open(os.path.join(ROOT, 'include', 'cgc_hip.h')).read()
    assert lib.cgc_abi_version() == _abi.ABI_VERSION == int(re.search(r'#define CGC_ABI_VERSION (\d+)', header).group(1)) >= 23
    assert re.search(r'^ \*  23: region statistics', header, flags=re.M)
    assert '/* ---- F17 (' in header
    for name in SYMBOLS:
        assert name in _abi.PROTOTYPES and re.search(r'^int(64_t)? %s\(' % name, header, flags=re.M), name
        assert getattr(lib, name).argtypes == _abi.PROTOTYPES[name]
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert _abi.PROTOTYPES['cgc_region_moments'] == [P, P, I, I, P, I, I, I, I, P, P, P, P, P, P, P, P, P, P]
    assert _abi.PROTOTYPES['cgc_region_histogram'] == [P, P, P, I, I, I, I, P, P, P]
    assert _abi.PROTOTYPES['cgc_region_quantiles'] == [P, L, P, I, P, P]
    assert lib.cgc_region_ws_bytes.restype == ctypes.c_int64
