"""CPU: the host side of stain normalisation (csrc/stain.hip; cgc_net_amd.nuclei.stain_maxima, recolor_matrix, recolor,
normalize_stains, kernels.HipKernels.concentration_histogram and od_recolor): what the public functions and the kernel table refuse
before a tensor is touched, and what the library refuses without launching.

As in tests/test_macenko_host_cpu.py the tests lift the "on the GPU" refusal (``on_gpu=False``) and replace the kernel table by one
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = [[4096, 0, 0], [0, 4096, 0], [0, 0, 4096]]
M = nuclei.stain_matrix().tolist()
S = np.array(nuclei.DEFAULT_STAINS)
REACH_CONC = (2 ** 31 - 2 ** 15 - 1) // 5674                                     # the largest sum_c |m[c][s]| that is admitted
REACH_RECOLOR = (2 ** 31 - 2 ** 11 - 1) // 5674


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


class Untouchable(object):
    """Stands in for a tensor: any use fails the test."""

    def __getattr__(self, name):
        pytest.fail('a tensor was touched (%s)' % name)


def tile(*shape, dtype=torch.uint8):
    return torch.zeros(shape or (4, 5, 3), dtype=dtype)


def plane(*shape, dtype=torch.uint8):
    return torch.zeros(shape or (4, 5), dtype=dtype)


def public_calls():
    """The three public functions that take a tile, each with otherwise good arguments."""
    return (lambda image, **kw: nuclei.stain_maxima(image, **kw),
            lambda image, **kw: nuclei.normalize_stains(image, **dict(dict(stains=S), **kw)),
            lambda image, **kw: nuclei.normalize_stains(image, **kw),
            lambda image, **kw: nuclei.recolor(image, IDENTITY, **kw))


# ------------------------------------------------------------------ the public functions
def test_only_tensors_on_the_gpu():
    for fn in public_calls():
        for bad in (tile(), np.zeros((4, 5, 3), np.uint8), None):
            with pytest.raises(TypeError):
                fn(bad)


def test_form_of_the_image_order_and_within(no_launch):
    for fn in public_calls():
        for dtype in (torch.bool, torch.int8, torch.int16, torch.int32, torch.int64, torch.float32, torch.float16):
            with pytest.raises(TypeError):
                fn(tile(dtype=dtype))
        for shape in ((4, 5), (4, 5, 1), (4, 5, 4), (3, 4, 5), (2, 4, 5, 3), (3,)):
            with pytest.raises(ValueError):
                fn(tile(*shape))
        for bad in ('BGR', 'gbr', 0, 1, None):
            with pytest.raises(ValueError, match='order'):
                fn(tile(), order=bad)
    for fn in public_calls()[:3]:
        for other in (plane(5, 4), plane(4, 6), plane(4, 5, 1)):
            with pytest.raises(ValueError):
                fn(tile(), within=other)
        with pytest.raises(TypeError):
            fn(tile(), within=plane(dtype=torch.float32))
        with pytest.raises(TypeError):
            fn(tile(), within=np.ones((4, 5), bool))
        with pytest.raises(ValueError, match='device'):
            fn(tile(), within=torch.zeros(4, 5, dtype=torch.bool, device='meta'))


def test_beta_alpha_and_stains(no_launch):
    for fn in public_calls()[:3]:
        for bad in (-0.01, 5674 / 1024 + 1e-9, 6, float('nan'), float('inf'), '0.15', None, True, (0.15,)):
            with pytest.raises(ValueError, match='beta'):
                fn(tile(), beta=bad)
        for bad in (-1, -1e-9, 50, 50.0, 99, float('nan'), float('inf'), '1', None, False, (1,)):
            with pytest.raises(ValueError, match='alpha'):
                fn(tile(), alpha=bad)
    for fn in public_calls()[:2]:
        for bad in ('hed', 'macenko', [[1, 0, 0], [0, 1, 0]], np.zeros((3, 3)), [[1, 0, 0], [1, 0, 0], [0, 0, 1]],
                    [[1, 0, 0], [0, float('nan'), 0], [0, 0, 1]], [[1, 0, 0], [1, 1e-9, 0], [0, 0, 1]]):
            with pytest.raises(ValueError):
                fn(tile(), stains=bad)


def test_bad_targets_are_refused_before_any_launch(no_launch):
    for kw in (dict(target_stains='hed'), dict(target_stains=[[1, 0, 0]]), dict(target_stains=[[1, 0], [0, 1]]),
               dict(target_stains=[[0, 0, 0], [0, 1, 0]]), dict(target_stains=[[1, 0, 0], [0, float('inf'), 0]]),
               dict(target_stains=np.zeros((4, 3))), dict(target_max=(1.0,)), dict(target_max=(1.0, 0.0)), dict(target_max=(-1.0, 1.0)),
               dict(target_max=(1.0, float('nan'))), dict(target_max=(1.0, float('inf'))), dict(target_max='ab'),
               dict(target_max=(1.0, 2.0, 3.0))):
        with pytest.raises(ValueError, match='target'):
            nuclei.normalize_stains(tile(), stains=S, **kw)
        with pytest.raises(ValueError, match='target'):
            nuclei.normalize_stains(tile(), **kw)                                # ... before the estimate's launches too
        with pytest.raises(ValueError, match='target'):
            nuclei.recolor_matrix(S, (1.0, 1.0), **kw)


def test_an_empty_image_has_no_maxima_and_an_empty_recolouring(no_launch):
    for shape in ((0, 5, 3), (4, 0, 3), (0, 0, 3)):
        with pytest.raises(ValueError, match='no stained pixel'):
            nuclei.stain_maxima(tile(*shape))
        with pytest.raises(ValueError, match='no stained pixel'):
            nuclei.normalize_stains(tile(*shape), stains=S, within=plane(*shape[:2], dtype=torch.bool), beta=0, alpha=0)
        with pytest.raises(ValueError, match='too few stained pixels'):
            nuclei.normalize_stains(tile(*shape))


def test_recolor_matrix_refusals():
    good = nuclei.recolor_matrix(S, (Fraction(3, 2), 1))
    assert good.dtype == np.int32 and good.shape == (3, 3)
    for bad in ('hed', [[1, 0, 0], [0, 1, 0]], np.zeros((3, 3)), np.ones((2, 3)), [[1, 0, 0], [2, 0, 0], [0, 0, 1]],
                [[1, 0, 0], [0, float('nan'), 0], [0, 0, 1]], [[1, 0, 0], [0, float('inf'), 0], [0, 0, 1]], None):
        with pytest.raises(ValueError):
            nuclei.recolor_matrix(bad, (1.0, 1.0))
    for bad in ((1.0,), (1.0, 0.0), (0, 1), (-1.0, 1.0), (1.0, float('nan')), (float('inf'), 1.0), (1, 2, 3), 'ab', None, 1.0,
                (Fraction(0), Fraction(1))):
        with pytest.raises(ValueError, match='maxima'):
            nuclei.recolor_matrix(S, bad)
    with pytest.raises(ValueError, match='overflow'):                            # a tiny maximum: a huge scale
        nuclei.recolor_matrix(S, (1e-3, 1.0))
    with pytest.raises(ValueError, match='overflow'):
        nuclei.recolor_matrix(S, (1.0, 1.0), target_max=(1e3, 1.0))
    with pytest.raises(ValueError, match='overflow'):
        nuclei.recolor_matrix(S, (1e-300, 1.0))                                  # a scale beyond float64's integers


def test_recolor_refuses_its_matrix_before_any_launch(no_launch):
    big = REACH_RECOLOR + 1
    for bad in ([[big, 0, 0], [0, 1, 0], [0, 0, 1]], [[1, 0, 0], [0, 1, 0], [0, 0, -big]], [[0, big // 3 + 1, 0]] * 3,
                [[2 ** 31, 0, 0], [0, 1, 0], [0, 0, 1]], IDENTITY[:2], [row[:2] for row in IDENTITY], [4096] * 9, 'abc', None,
                np.eye(3), np.eye(3, dtype=np.float32) * 4096,
                [[0.9, 0, 0], [0, 1, 0], [0, 0, 1]], [[4096.0, 0, 0], [0, 4096, 0], [0, 0, 4096]]):      # floats in a list: not truncated
        with pytest.raises(ValueError):
            nuclei.recolor(tile(), bad)


def test_zero_and_saturated_maxima(monkeypatch):
    """The decisions on the 1024 counts, on counts handed in: a table that returns them stands in for the kernel."""
    counts = [0] * 1024

    class Table(object):
        def concentration_histogram(self, image, order, lut, od_min, m, within=None):
            assert lut is nuclei.OD_LUT and od_min == 154 and m == M
            return torch.tensor(counts, dtype=torch.int32)

    check = nuclei._check_image
    monkeypatch.setattr(nuclei, '_check_image',
                        lambda fn, name, image, dtypes=None, on_gpu=True:
                        check(fn, name, image, on_gpu=False) if dtypes is None else check(fn, name, image, dtypes, on_gpu=False))
    monkeypatch.setattr(kernels, 'get', lambda: Table())
    monkeypatch.setattr(torch.cuda, 'device', lambda dev: __import__('contextlib').nullcontext())

    def maxima(h0, h1, **kw):
        counts[:] = [0] * 1024
        for b, c in h0.items():
            counts[b] = c
        for b, c in h1.items():
            counts[512 + b] = c
        return nuclei.stain_maxima(tile(), **kw)

    assert maxima({100: 99, 300: 1}, {7: 50, 8: 50}) == (Fraction(100, 128), Fraction(8, 128))
    assert maxima({100: 98, 300: 2}, {7: 50, 8: 50}, alpha=1) == (Fraction(300, 128), Fraction(8, 128))
    assert maxima({100: 98, 300: 2}, {7: 50, 8: 50}, alpha=0) == (Fraction(300, 128), Fraction(8, 128))
    assert all(isinstance(v, Fraction) for v in maxima({1: 5}, {510: 5}))
    with pytest.raises(ValueError, match='no stained pixel'):
        maxima({}, {})
    with pytest.raises(ValueError, match='none of stain 0'):
        maxima({0: 100}, {9: 100})
    with pytest.raises(ValueError, match='none of stain 1'):
        maxima({9: 100}, {0: 99, 300: 1})
    with pytest.raises(ValueError, match='stain 0 is saturated'):
        maxima({511: 2, 3: 98}, {9: 100})
    with pytest.raises(ValueError, match='stain 1 is saturated'):
        maxima({9: 100}, {511: 100})
    assert maxima({511: 1, 3: 99}, {9: 100}) == (Fraction(3, 128), Fraction(9, 128))      # one pixel in a hundred: below the percentile
    counts[:] = [0] * 511 + [100] + [0] * 9 + [100] + [0] * 502
    with pytest.raises(ValueError, match='stain 0 is saturated'):                # stain_maxima's refusals are normalize_stains'
        nuclei.normalize_stains(tile(), stains=S)
    counts[:] = [0] * 9 + [100] + [0] * 502 + [100] + [0] * 511
    with pytest.raises(ValueError, match='none of stain 1'):
        nuclei.normalize_stains(tile(), stains=S)


# ------------------------------------------------------------------ the kernel table
def test_the_kernel_table_refuses_before_any_tensor():
    """HipKernels.concentration_histogram and od_recolor check their plain arguments before they touch a tensor (by the class: no
    instance, no library, no GPU)."""
    lut, exp, image = list(nuclei.OD_LUT), nuclei.EXP_LUT, Untouchable()
    conc = lambda *a, **k: kernels.HipKernels.concentration_histogram(None, image, *a, **k)      # noqa: E731
    recolor = lambda *a, **k: kernels.HipKernels.od_recolor(None, image, *a, **k)                # noqa: E731
    for order in (2, -1, None, 'bgr'):
        with pytest.raises(ValueError, match='order'):
            conc(order, lut, 154, M)
        with pytest.raises(ValueError, match='order'):
            recolor(order, lut, IDENTITY, exp)
    for table in (lut[:255], lut + [0], [-1] + lut[1:], [kernels.STAIN_OD_MAX + 1] + lut[1:]):
        with pytest.raises(ValueError, match='table'):
            conc(0, table, 154, M)
        with pytest.raises(ValueError, match='optical-density table'):
            recolor(0, table, IDENTITY, exp)
    for od_min in (-1, kernels.STAIN_OD_MAX + 1, 153.5, None, '154', True):
        with pytest.raises(ValueError, match='od_min'):
            conc(1, lut, od_min, M)
    for table in (None, ['a'] * 256, [0.5] * 256, 7):                               # not integers: a ValueError, not a TypeError
        with pytest.raises(ValueError, match='optical-density table'):
            recolor(0, table, IDENTITY, exp)
    for bad in ([[0.9, 0, 0], [0, 1, 0], [0, 0, 1]], [[4096.0, 0, 0], [0, 4096, 0], [0, 0, 4096]]):
        with pytest.raises(ValueError, match='matrix'):
            recolor(0, lut, bad, exp)
        with pytest.raises(ValueError, match='matrix'):
            conc(0, lut, 154, bad)
    with pytest.raises(ValueError, match='exponential table'):
        recolor(0, lut, IDENTITY, [255.0] + list(exp[1:]))
    for reach, fn in ((REACH_CONC, lambda m: conc(0, lut, 154, m)), (REACH_RECOLOR, lambda m: recolor(0, lut, m, exp))):
        for bad in ([[reach + 1, 0, 0], [0, 1, 0], [0, 0, 1]], [[1, 0, 0], [0, 1, 0], [0, 0, -reach - 1]],
                    [[0, 0, reach // 3 + 1]] * 3, M[:2], [row[:2] for row in M], [1] * 9, 'abc', None, [[1, 2, 'x']] * 3):
            with pytest.raises(ValueError, match='matrix'):
                fn(bad)
    assert REACH_RECOLOR == REACH_CONC + 5                                        # the two slacks differ: 2^15 - 2^11 = 5 * 5674 + 2350
    with pytest.raises(ValueError, match='matrix'):                              # admitted by od_recolor's bound, not by this one
        conc(0, lut, 154, [[REACH_RECOLOR, 0, 0], [0, 1, 0], [0, 0, 1]])
    check = kernels.HipKernels._check_concentration_tables                       # at the bound: accepted
    assert check(0, lut, 5674, [[REACH_CONC, 0, 0], [0, -REACH_CONC, 0], [0, 0, REACH_CONC]])[1][4] == -REACH_CONC
    check = kernels.HipKernels._check_recolor_tables
    flat = check(1, lut, [[REACH_RECOLOR, 1, 0], [0, -REACH_RECOLOR + 1, 0], [0, 0, REACH_RECOLOR]], exp)
    assert flat[1][0] == REACH_RECOLOR and flat[2] == list(exp)
    e = list(exp)
    bad_tables = [e[:-1], e + [0], [254] + e[1:], e[:-1] + [1], [256] + e[1:], e[:-2] + [-1, 0], e[:3000] + [e[3000] + 1] + e[3001:],
                  e[::-1], e[:100] + [e[99] + 1] + e[101:], None, 'abc', 7]
    for table in bad_tables:
        with pytest.raises(ValueError, match='exponential table'):
            recolor(0, lut, IDENTITY, table)
    kernels.HipKernels._check_exp_lut([255] * 6385 + [0])                        # of the accepted kind: a step
    kernels.HipKernels._check_exp_lut([255] + [0] * 6385)


def test_signatures_and_documents():
    p = inspect.signature(nuclei.stain_maxima).parameters
    assert list(p) == ['image', 'stains', 'order', 'alpha', 'beta', 'within']
    assert [p[k].default for k in list(p)[1:]] == [None, 'bgr', 1.0, 0.15, None]
    p = inspect.signature(nuclei.recolor_matrix).parameters
    assert list(p) == ['stains', 'maxima', 'target_stains', 'target_max'] and p['target_stains'].default is None is p['target_max'].default
    p = inspect.signature(nuclei.recolor).parameters
    assert list(p) == ['image', 'a', 'order'] and p['order'].default == 'bgr'
    p = inspect.signature(nuclei.normalize_stains).parameters
    assert list(p) == ['image', 'stains', 'order', 'target_stains', 'target_max', 'alpha', 'beta', 'within', 'return_info']
    assert [p[k].default for k in list(p)[1:]] == [None, 'bgr', None, None, 1.0, 0.15, None, False]
    doc = nuclei.normalize_stains.__doc__
    assert 'Host syncs: three' in doc and 'one with given stains' in doc and 'Macenko' in doc
    for item in ('1.  S = ', '2.  maxima', '3.  a = ', '4.  ', '5.  ', '6.  ``return_info``'):
        assert item in doc, item
    assert 'Host syncs: one' in nuclei.stain_maxima.__doc__ and 'Host syncs: none' in nuclei.recolor.__doc__
    for doc in (nuclei.__doc__, nuclei.stain_foreground.__doc__):
        assert 'norm = normalize_stains(tile)' in doc
        assert 'fg, t, plane = stain_foreground(norm, stains=TARGET_STAINS + residual)' in doc
        assert 'nucleus_features(L, bgr_to_gray(norm), max_label=n)' in doc
    p = inspect.signature(kernels.KernelSpec.concentration_histogram).parameters
    assert list(p) == ['self', 'image', 'order', 'lut', 'od_min', 'm', 'within'] and p['within'].default is None
    p = inspect.signature(kernels.KernelSpec.od_recolor).parameters
    assert list(p) == ['self', 'image', 'order', 'lut', 'a', 'exp_lut']
    for name, items in (('concentration_histogram', 6), ('od_recolor', 7)):
        doc = getattr(kernels.KernelSpec, name).__doc__
        for k in range(1, items + 1):
            assert '\n        %d.  ' % k in doc, (name, k)
        assert list(inspect.signature(getattr(kernels.HipKernels, name)).parameters) == \
            list(inspect.signature(getattr(kernels.KernelSpec, name)).parameters)
        with pytest.raises(NotImplementedError):
            getattr(kernels.KernelSpec(), name)(*([None] * (len(inspect.signature(getattr(kernels.KernelSpec, name)).parameters) - 1)))
    assert kernels.CONC_BINS == 512 == nuclei.CONC_BINS and kernels.EXP_LUT_LEN == 6386 == len(nuclei.EXP_LUT)
    for name in ('README.md', 'INTEGRATION.md', 'DESIGN.md'):
        assert 'normalize_stains' in open(os.path.join(ROOT, name)).read(), name
    assert '## Stain normalisation' in open(os.path.join(ROOT, 'DESIGN.md')).read()


# ------------------------------------------------------------------ the library, without a launch
def test_library_refusals(lib):
    einval = -1
    lut = (ctypes.c_int * 256)(*nuclei.OD_LUT)
    m9 = (ctypes.c_int * 9)(*[v for row in M for v in row])
    a9 = (ctypes.c_int * 9)(*[v for row in IDENTITY for v in row])
    exp = (ctypes.c_int * 6386)(*nuclei.EXP_LUT)
    out = (ctypes.c_int64 * 1200)()                                               # any non-NULL address: nothing is launched
    some = ctypes.addressof(out)

    # cgc_concentration_histogram(pix, npix, order, lut, od_min, m, within, within_bytes, out, stream)
    # cgc_od_recolor(pix, npix, order, lut, a, exp_lut, exp_len, ws, out, stream)
    def conc(npix=4, order=0, lut=lut, od_min=154, m=m9, within=None, wbytes=0, out=some, pix=some):
        return lib.cgc_concentration_histogram(pix, npix, order, lut, od_min, m, within, wbytes, out, None)

    def recolor(npix=4, order=0, lut=lut, a=a9, exp=exp, exp_len=6386, ws=some, out=some, pix=some):
        return lib.cgc_od_recolor(pix, npix, order, lut, a, exp, exp_len, ws, out, None)

    for fn in (conc, recolor):
        for npix in (-1, 2 ** 31, 2 ** 40):
            assert fn(npix=npix) == einval
        for order in (-1, 2, 3):
            assert fn(order=order) == einval
        assert fn(lut=None) == einval
        for v, bad in ((0, -1), (0, kernels.STAIN_OD_MAX + 1), (255, 2 ** 30)):
            table = (ctypes.c_int * 256)(*nuclei.OD_LUT)
            table[v] = bad
            assert fn(lut=table) == einval
            assert fn(lut=table, npix=0) == einval
        assert fn(out=None) == einval
        assert fn(pix=None) == einval                                             # a NULL image of four pixels
    for od_min in (-1, kernels.STAIN_OD_MAX + 1, 2 ** 30, -2 ** 31):
        assert conc(od_min=od_min) == einval
    for wbytes in (0, 3, 5, 16, -1):
        assert conc(within=some, wbytes=wbytes) == einval
    assert conc(out=None, npix=0) == einval
    assert conc(m=None) == einval and recolor(a=None) == einval and recolor(exp=None) == einval and recolor(ws=None) == einval
    for reach, fn, key in ((REACH_CONC, conc, 'm'), (REACH_RECOLOR, recolor, 'a')):
        for rows in ([reach + 1, 0, 0, 0, 1, 0, 0, 0, 1], [1, 0, 0, 0, 1, 0, 0, 0, -reach - 1], [0, 0, reach // 3 + 1] * 3,
                     [2 ** 31 - 1] * 9, [-2 ** 31] * 9):
            assert fn(**{key: (ctypes.c_int * 9)(*rows)}) == einval
            assert fn(**{key: (ctypes.c_int * 9)(*rows), 'npix': 0}) == einval
    assert conc(m=(ctypes.c_int * 9)(REACH_RECOLOR, 0, 0, 0, 1, 0, 0, 0, 1)) == einval
    assert recolor(a=(ctypes.c_int * 9)(REACH_RECOLOR, 0, 0, 0, -REACH_RECOLOR, 0, 0, 0, REACH_RECOLOR), npix=0) == 0      # at the bound
    for exp_len in (0, 6385, 6387, -1, 256):
        assert recolor(exp_len=exp_len) == einval

    def table_with(changes):
        t = list(nuclei.EXP_LUT)
        for k, v in changes.items():
            t[k] = v
        return (ctypes.c_int * 6386)(*t)

    for changes in ({0: 254}, {0: 256}, {6385: 1}, {6385: -1}, {3000: nuclei.EXP_LUT[2999] + 1}, {100: 256}, {6000: -1},
                    {k: nuclei.EXP_LUT[6385 - k] for k in range(6386)}):
        assert recolor(exp=table_with(changes)) == einval
        assert recolor(exp=table_with(changes), npix=0) == einval
    assert recolor(npix=0) == 0 and recolor(npix=0, pix=None, ws=None, out=None) == 0                 # an empty image: nothing to do
    assert recolor(npix=0, exp=table_with({k: 255 if k < 6385 else 0 for k in range(6386)})) == 0     # a step: of the accepted kind
    assert lib.cgc_concentration_bins() == 512 and lib.cgc_exp_lut_len() == 6386 and lib.cgc_od_recolor_ws_bytes() == 6400
    assert lib.cgc_scan_chunk_pixels() == 16384


def test_abi_17_in_the_header_the_prototypes_and_the_library(lib):
    header = open(os.path.join(ROOT, 'include', 'cgc_hip.h')).read()
    assert lib.cgc_abi_version() == _abi.ABI_VERSION == int(re.search(r'#define CGC_ABI_VERSION (\d+)', header).group(1)) >= 17
    assert re.search(r'^ \*  17: stain normalisation', header, flags=re.M)
    for name in ('cgc_concentration_bins', 'cgc_concentration_histogram', 'cgc_exp_lut_len', 'cgc_od_recolor'):
        assert name in _abi.PROTOTYPES and re.search(r'^int %s\(' % name, header, flags=re.M), name
        assert getattr(lib, name).argtypes == _abi.PROTOTYPES[name]
    assert 'cgc_od_recolor_ws_bytes' in _abi.PROTOTYPES and re.search(r'^int64_t cgc_od_recolor_ws_bytes\(void\);', header, flags=re.M)
    assert lib.cgc_od_recolor_ws_bytes.restype is ctypes.c_int64
    assert len(_abi.PROTOTYPES['cgc_concentration_histogram']) == 10 and len(_abi.PROTOTYPES['cgc_od_recolor']) == 10
