"""CPU: the host side of stain estimation (csrc/stain.hip; cgc_net_amd.nuclei.estimate_stains, kernels.HipKernels.od_moments and
angle_histogram): what the public function and the kernel table refuse before a tensor is touched, and what the library refuses
without launching.

As in tests/test_stain_host_cpu.py the tests lift the "on the GPU" refusal (``on_gpu=False``) and replace the kernel table by one that
fails the test when it is asked for: every refusal checked here is raised before any launch."""
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
K = kernels.ANGLE_BINS
BASIS = [[4096, 0, 0], [0, 4096, 0]]


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


# ------------------------------------------------------------------ estimate_stains
def test_only_tensors_on_the_gpu():
    for bad in (tile(), np.zeros((4, 5, 3), np.uint8), None):
        with pytest.raises(TypeError):
            nuclei.estimate_stains(bad)


def test_form_of_the_image_and_within(no_launch):
    for dtype in (torch.bool, torch.int8, torch.int16, torch.int32, torch.int64, torch.float32, torch.float16):
        with pytest.raises(TypeError):
            nuclei.estimate_stains(tile(dtype=dtype))
    for shape in ((4, 5), (4, 5, 1), (4, 5, 4), (3, 4, 5), (2, 4, 5, 3), (3,)):
        with pytest.raises(ValueError):
            nuclei.estimate_stains(tile(*shape))
    for bad in ('BGR', 'gbr', 0, 1, None):
        with pytest.raises(ValueError, match='order'):
            nuclei.estimate_stains(tile(), order=bad)
    for other in (plane(5, 4), plane(4, 6), plane(4, 5, 1)):
        with pytest.raises(ValueError):
            nuclei.estimate_stains(tile(), within=other)
    with pytest.raises(TypeError):
        nuclei.estimate_stains(tile(), within=plane(dtype=torch.float32))
    with pytest.raises(TypeError):
        nuclei.estimate_stains(tile(), within=np.ones((4, 5), bool))
    with pytest.raises(ValueError, match='device'):
        nuclei.estimate_stains(tile(), within=torch.zeros(4, 5, dtype=torch.bool, device='meta'))


def test_beta_and_alpha(no_launch):
    for bad in (-0.01, 5674 / 1024 + 1e-9, 6, float('nan'), float('inf'), '0.15', None, True, (0.15,)):
        with pytest.raises(ValueError, match='beta'):
            nuclei.estimate_stains(tile(), beta=bad)
    for bad in (-1, -1e-9, 50, 50.0, 99, float('nan'), float('inf'), '1', None, False, (1,)):
        with pytest.raises(ValueError, match='alpha'):
            nuclei.estimate_stains(tile(), alpha=bad)


def test_an_empty_image_is_refused_without_a_launch(no_launch):
    for shape in ((0, 5, 3), (4, 0, 3), (0, 0, 3)):
        with pytest.raises(ValueError, match='too few stained pixels'):
            nuclei.estimate_stains(tile(*shape))
        with pytest.raises(ValueError, match='too few stained pixels'):
            nuclei.estimate_stains(tile(*shape), within=plane(*shape[:2], dtype=torch.bool), beta=0, alpha=0)


def test_the_host_steps_refuse_degenerate_moments():
    with pytest.raises(ValueError, match='too few stained pixels'):
        nuclei._plane_of_moments([0] * 10)
    with pytest.raises(ValueError, match='too few stained pixels'):
        nuclei._plane_of_moments([1, 200, 300, 400, 40000, 60000, 80000, 90000, 120000, 160000])
    flat = [5, 5 * 200, 5 * 300, 5 * 400, 5 * 40000, 5 * 60000, 5 * 80000, 5 * 90000, 5 * 120000, 5 * 160000]      # five equal pixels
    with pytest.raises(ValueError, match='one stain only'):
        nuclei._plane_of_moments(flat)
    line = [(200 * k, 300 * k, 400 * k) for k in (1, 2, 3, 5)]                                                  # pixels on one line
    mom = [len(line)] + [sum(o[c] for o in line) for c in range(3)] + \
          [sum(o[i] * o[j] for o in line) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    try:                                                                      # exact integers: C has rank one; eigh may still return
        n, lam, e1, e2 = nuclei._plane_of_moments(mom)                        # a tiny positive second eigenvalue
        assert lam[1] < 1e-9 * lam[2]
    except ValueError as e:
        assert 'one stain only' in str(e)
    e1, e2 = np.array([0.6, 0.6, 0.52]), np.array([0.5, -0.7, 0.5])
    with pytest.raises(ValueError):                                           # both percentiles in one bin: stain_matrix's refusal
        nuclei._stains_of_bins(e1, e2, 500, 500)


# ------------------------------------------------------------------ the kernel table
def test_the_kernel_table_refuses_before_any_tensor():
    """HipKernels.od_moments and angle_histogram check their plain arguments before they touch a tensor (by the class: no instance,
    no library, no GPU)."""
    lut, dirs, image = list(nuclei.OD_LUT), nuclei.ANGLE_DIRS, Untouchable()
    od_moments = lambda *a, **k: kernels.HipKernels.od_moments(None, image, *a, **k)                # noqa: E731
    angle_histogram = lambda *a, **k: kernels.HipKernels.angle_histogram(None, image, *a, **k)      # noqa: E731
    for order in (2, -1, None, 'bgr'):
        with pytest.raises(ValueError, match='order'):
            od_moments(order, lut, 154)
        with pytest.raises(ValueError, match='order'):
            angle_histogram(order, lut, 154, BASIS, dirs)
    for table in (lut[:255], lut + [0], [-1] + lut[1:], [kernels.STAIN_OD_MAX + 1] + lut[1:]):
        with pytest.raises(ValueError, match='table'):
            od_moments(0, table, 154)
        with pytest.raises(ValueError, match='table'):
            angle_histogram(0, table, 154, BASIS, dirs)
    for od_min in (-1, kernels.STAIN_OD_MAX + 1, 153.5, None, '154', True):
        with pytest.raises(ValueError, match='od_min'):
            od_moments(1, lut, od_min)
        with pytest.raises(ValueError, match='od_min'):
            angle_histogram(1, lut, od_min, BASIS, dirs)
    for basis in ([[4097, 0, 0], [0, 4096, 0]], [[4096, 0, 0], [0, -4097, 0]], [[2366, 2365, 2365], [0, 4096, 0]],
                  [[4096, 0, 0], [-2365, 2365, -2366]], [[4096, 0, 0]], [[4096, 0], [0, 4096]], [4096, 0, 0, 0, 4096, 0], None):
        with pytest.raises(ValueError, match='basis'):
            angle_histogram(0, lut, 154, basis, dirs)
    check = kernels.HipKernels._check_angle_tables
    flat_basis, flat_dirs = check([[2365, 2365, 2365], [-2365, 2365, -2365]], dirs)                  # at the bound: accepted
    assert flat_basis == [2365, 2365, 2365, -2365, 2365, -2365] and len(flat_dirs) == 2 * (K - 1)
    assert flat_dirs[:2] == [50, -16384] and flat_dirs[-2:] == [50, 16384]
    d = [list(v) for v in dirs]
    bad_tables = [d[:-1], d + [[1, 16384]], [v + [0] for v in d]]
    for k, v in ((0, [50, -16385]), (511, [16385, 0]), (1022, [50, 16385])):                          # out of range
        bad_tables.append(d[:k] + [v] + d[k + 1:])
    bad_tables.append(d[:300] + [d[299]] + d[301:])                                                   # not increasing: a repeat
    bad_tables.append(d[:300] + [d[301], d[300]] + d[302:])                                           # ... a swap
    bad_tables.append(d[::-1])                                                                        # ... decreasing
    bad_tables.append([[0, -16384]] + d[1:])                                                          # on the edge of the half plane
    bad_tables.append([[-50, -16384]] + d[1:])                                                        # beyond it
    for table in bad_tables:
        with pytest.raises(ValueError, match='dir'):
            angle_histogram(0, lut, 154, BASIS, table)


def test_signatures_and_documents():
    p = inspect.signature(nuclei.estimate_stains).parameters
    assert list(p) == ['image', 'order', 'beta', 'alpha', 'within', 'return_info']
    assert [p[k].default for k in list(p)[1:]] == ['bgr', 0.15, 1.0, None, False]
    doc = nuclei.estimate_stains.__doc__
    assert 'Host syncs: two' in doc and 'Macenko' in doc
    for item in ('1.  od_min', '2.  ', '3.  E[j][c]', '4.  ', '5.  v_lo', '6.  ``return_info``'):
        assert item in doc, item
    assert 'estimate_stains' in nuclei.__doc__ and 'estimate_stains' in nuclei.stain_foreground.__doc__
    assert 'Host syncs' in nuclei.stain_foreground.__doc__
    p = inspect.signature(kernels.KernelSpec.od_moments).parameters
    assert list(p) == ['self', 'image', 'order', 'lut', 'od_min', 'within'] and p['within'].default is None
    p = inspect.signature(kernels.KernelSpec.angle_histogram).parameters
    assert list(p) == ['self', 'image', 'order', 'lut', 'od_min', 'basis', 'dirs', 'within'] and p['within'].default is None
    for name in ('od_moments', 'angle_histogram'):
        assert getattr(kernels.KernelSpec, name).__doc__
        assert list(inspect.signature(getattr(kernels.HipKernels, name)).parameters) == \
            list(inspect.signature(getattr(kernels.KernelSpec, name)).parameters)
        with pytest.raises(NotImplementedError):
            getattr(kernels.KernelSpec(), name)(*([None] * (len(inspect.signature(getattr(kernels.KernelSpec, name)).parameters) - 2)))
    assert kernels.ANGLE_BINS == 1024 == nuclei.ANGLE_BINS and len(nuclei.ANGLE_DIRS) == 1023
    for name in ('README.md', 'INTEGRATION.md', 'DESIGN.md'):
        assert 'estimate_stains' in open(os.path.join(ROOT, name)).read(), name
    assert '## Stain estimation' in open(os.path.join(ROOT, 'DESIGN.md')).read()


def test_stain_foreground_still_takes_no_string(no_launch):
    for bad in ('hed', 'macenko', 'auto', 'estimate'):
        with pytest.raises(ValueError):
            nuclei.stain_foreground(tile(), stains=bad)
        with pytest.raises(ValueError):
            nuclei.separate_stains(tile(), stains=bad)
        with pytest.raises(ValueError):
            nuclei.stain_matrix(bad)
    p = inspect.signature(nuclei.stain_foreground).parameters
    assert list(p) == ['image', 'stain', 'radius', 'stains', 'order', 'within']


# ------------------------------------------------------------------ the library, without a launch
def test_library_refusals(lib):
    einval = -1
    lut = (ctypes.c_int * 256)(*nuclei.OD_LUT)
    basis = (ctypes.c_int * 6)(*[v for row in BASIS for v in row])
    flat = [v for d in nuclei.ANGLE_DIRS for v in d]
    dirs = (ctypes.c_int * len(flat))(*flat)
    out = (ctypes.c_int64 * 1200)()                                               # any non-NULL address: nothing is launched
    some = ctypes.addressof(out)

    # cgc_od_moments(pix, npix, order, lut, od_min, within, within_bytes, out, stream)
    # cgc_angle_histogram(pix, npix, order, lut, od_min, basis, dirs, within, within_bytes, ws, out, stream)
    def moments(npix=4, order=0, lut=lut, od_min=154, within=None, wbytes=0, out=some, pix=some):
        return lib.cgc_od_moments(pix, npix, order, lut, od_min, within, wbytes, out, None)

    def angles(npix=4, order=0, lut=lut, od_min=154, basis=basis, dirs=dirs, within=None, wbytes=0, ws=some, out=some, pix=some):
        return lib.cgc_angle_histogram(pix, npix, order, lut, od_min, basis, dirs, within, wbytes, ws, out, None)

    for fn in (moments, angles):
        for npix in (-1, 2 ** 31, 2 ** 40):
            assert fn(npix=npix) == einval
        for order in (-1, 2, 3):
            assert fn(order=order) == einval
        for od_min in (-1, kernels.STAIN_OD_MAX + 1, 2 ** 30, -2 ** 31):
            assert fn(od_min=od_min) == einval
        assert fn(lut=None) == einval
        for v, bad in ((0, -1), (0, kernels.STAIN_OD_MAX + 1), (255, 2 ** 30)):
            table = (ctypes.c_int * 256)(*nuclei.OD_LUT)
            table[v] = bad
            assert fn(lut=table) == einval
            assert fn(lut=table, npix=0) == einval
        for wbytes in (0, 3, 5, 16, -1):
            assert fn(within=some, wbytes=wbytes) == einval
        assert fn(out=None) == einval
        assert fn(out=None, npix=0) == einval
        assert fn(pix=None) == einval                                             # a NULL image of four pixels
    assert angles(basis=None) == einval and angles(dirs=None) == einval and angles(ws=None) == einval
    for rows in ([4097, 0, 0, 0, 4096, 0], [4096, 0, 0, 0, -4097, 0], [2366, 2365, 2365, 0, 4096, 0], [4096, 0, 0, -2365, 2365, -2366],
                 [2 ** 31 - 1] * 6, [-2 ** 31] * 6):
        assert angles(basis=(ctypes.c_int * 6)(*rows)) == einval
        assert angles(basis=(ctypes.c_int * 6)(*rows), npix=0) == einval

    def table_with(changes):
        t = list(flat)
        for k, (c, s) in changes.items():                                         # direction k = 1..K-1
            t[2 * (k - 1)], t[2 * (k - 1) + 1] = c, s
        return (ctypes.c_int * len(t))(*t)

    d = nuclei.ANGLE_DIRS
    for changes in ({1: (50, -16385)}, {512: (16385, 0)}, {1023: (50, 16385)}, {7: (2 ** 31 - 1, 2 ** 31 - 1)},      # out of range
                    {301: d[299]}, {301: d[301], 302: d[300]}, {1: (0, -16384)}, {1: (-50, -16384)}, {1023: (0, 16384)}):
        assert angles(dirs=table_with(changes)) == einval
        assert angles(dirs=table_with(changes), npix=0) == einval
    # an empty image: the result is zeroed by an asynchronous fill of host memory the test may not ask for, so only the checks above
    # run on npix = 0; the constants
    assert lib.cgc_angle_bins() == K and lib.cgc_angle_histogram_ws_bytes() == 4 * K
    assert lib.cgc_scan_chunk_pixels() == 16384
    header = open(os.path.join(ROOT, 'include', 'cgc_hip.h')).read()
    assert lib.cgc_abi_version() == _abi.ABI_VERSION == int(re.search(r'#define CGC_ABI_VERSION (\d+)', header).group(1)) >= 16
    for name in ('cgc_od_moments', 'cgc_angle_histogram'):
        assert name in _abi.PROTOTYPES and re.search(r'^int %s\(' % name, header, flags=re.M)
