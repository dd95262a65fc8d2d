"""Exact distance transform on the GPU (csrc/edt.hip through cgc_net_amd.nuclei.distance_transform / expand_labels /
split_touching) against tests/edt_ref.py (scipy's distances, a two-phase numpy restatement for the nearest site; pinned to a brute
force by tests/test_edt_ref_cpu.py).  Every comparison is exact.

The kernels cut columns into segments of 64 rows and walk a row with 256 threads: the shapes sit under, on and one over 64 and 128
rows and 256 columns, plus rows and columns longer than one workgroup."""
import functools

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import nuclei

import edt_ref as ref
from image_cases import DEV, gpu, tissue, two_discs

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 37), (41, 1), (7, 5), (31, 33), (64, 64), (65, 63), (64, 65), (7, 293), (129, 257), (300, 300), (3, 2100), (2100, 3),
          (63, 9), (127, 3), (128, 3), (5, 255), (5, 256), (5, 257)]
DENSITIES = [0.0, 0.001, 0.02, 0.3, 0.9, 1.0]


def run(image, **kw):
    t = image if torch.is_tensor(image) else gpu(image)
    d2, near = nuclei.distance_transform(t, return_nearest=True, **kw)
    for o in (d2, near):
        assert o.dtype == torch.int32 and o.device == t.device and tuple(o.shape) == tuple(t.shape) and o.is_contiguous()
    return d2.cpu().numpy(), near.cpu().numpy()


def check_sites(site, want=None):
    """Both ``sites`` modes on the site mask ``site`` against the oracle (computed once)."""
    wd2, wnear = ref.edt(site, 'nonzero') if want is None else want
    for image, mode in ((site, 'nonzero'), (~site, 'zero')):
        d2, near = run(image, sites=mode)
        assert np.array_equal(d2, wd2), (mode, np.argwhere(d2 != wd2)[:5])
        assert np.array_equal(near, wnear), (mode, np.argwhere(near != wnear)[:5])
    return wd2, wnear


# ------------------------------------------------------------------ random sites
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_random_sites(shape):
    for density in DENSITIES:
        site = np.random.RandomState(int(1000 * density) + 7).rand(*shape) < density
        wd2, wnear = check_sites(site)
        if not site.any():
            assert (wd2 == nuclei.EDT_INF).all() and (wnear == -1).all()


def test_default_is_scipy_squared():
    from scipy import ndimage
    img = np.random.RandomState(5).rand(97, 131) < 0.7
    d2 = nuclei.distance_transform(gpu(img))
    assert torch.is_tensor(d2) and d2.dtype == torch.int32
    want = ndimage.distance_transform_edt(img)
    assert np.array_equal(np.sqrt(d2.cpu().numpy().astype(np.float64)), want)


# ------------------------------------------------------------------ structured sites
def structured():
    N = 300
    for name, (y, x) in dict(tl=(0, 0), tr=(0, N - 1), bl=(N - 1, 0), br=(N - 1, N - 1)).items():
        m = np.zeros((N, N), bool)
        m[y, x] = True
        yield 'corner_' + name, m
    for name, sl in dict(row=np.s_[137, :], column=np.s_[:, 201], last_row=np.s_[-1, :], last_column=np.s_[:, -1]).items():
        m = np.zeros((150, 270), bool)
        m[sl] = True
        yield name, m
    for pitch in (2, 3, 8):
        m = np.zeros((131, 259), bool)
        m[::pitch, ::pitch] = True
        yield 'lattice%d' % pitch, m
        m = np.zeros((131, 259), bool)
        m[1::pitch, pitch - 1::pitch] = True
        yield 'lattice%d_offset' % pitch, m
    yy, xx = np.mgrid[0:130, 0:261]
    yield 'checkerboard', (yy + xx) % 2 == 0


STRUCTURED = dict(structured())


@pytest.mark.parametrize('name', sorted(STRUCTURED))
def test_structured_sites(name):
    check_sites(STRUCTURED[name])


# ------------------------------------------------------------------ input forms
@functools.lru_cache(maxsize=None)
def form_case():
    img = (np.random.RandomState(11).rand(70, 133) < 0.05) * np.random.RandomState(12).randint(-3, 4, size=(70, 133))
    return img, ref.edt(img, 'nonzero'), ref.edt(img, 'zero')


@pytest.mark.parametrize('dtype', [torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64], ids=str)
def test_dtypes(dtype):
    img, want_nz, want_z = form_case()
    if dtype in (torch.bool, torch.uint8):
        img = img != 0
    t = gpu(img).to(dtype)
    for mode, want in (('nonzero', want_nz), ('zero', want_z)):
        d2, near = run(t, sites=mode)
        assert np.array_equal(d2, want[0]) and np.array_equal(near, want[1])


def test_non_contiguous_view():
    img, _, _ = form_case()
    t = gpu(img.astype(np.int32)).t()
    assert not t.is_contiguous()
    wd2, wnear = ref.edt(img.T, 'nonzero')
    d2, near = run(t, sites='nonzero')
    assert np.array_equal(d2, wd2) and np.array_equal(near, wnear)
    wide = gpu(np.repeat(img.astype(np.int16), 2, axis=1))[:, ::2]
    d2, near = run(wide, sites='nonzero')
    assert np.array_equal(d2, form_case()[1][0]) and np.array_equal(near, form_case()[1][1])


# ------------------------------------------------------------------ max_distance
@functools.lru_cache(maxsize=None)
def bound_case():
    site = np.random.RandomState(21).rand(140, 270) < 0.004
    site[60:80] = False                      # a band that is farther than 10 from any site of its own rows
    return site, ref.edt(site, 'nonzero')


@pytest.mark.parametrize('max_distance,d2max', [(0, 0), (1, 1), (1.5, 2), (2 ** 0.5, 2), (3, 9), (10, 100)])
def test_max_distance(max_distance, d2max):
    site, (wd2, wnear) = bound_case()
    assert nuclei._d2max(max_distance, 'max_distance') == d2max
    keep = wd2 <= d2max
    d2, near = run(site, sites='nonzero', max_distance=max_distance)
    assert np.array_equal(d2, np.where(keep, wd2, nuclei.EDT_INF))
    assert np.array_equal(near, np.where(keep, wnear, -1))
    od2, onear = ref.edt(site, 'nonzero', max_distance)                 # the oracle's own float comparison selects the same set
    assert np.array_equal(d2, od2) and np.array_equal(near, onear)
    d2, near = run(~site, sites='zero', max_distance=float(max_distance))
    assert np.array_equal(d2, np.where(keep, wd2, nuclei.EDT_INF)) and np.array_equal(near, np.where(keep, wnear, -1))


def test_without_nearest_and_twice():
    site, (wd2, _) = bound_case()
    t = gpu(site)
    only = nuclei.distance_transform(t, sites='nonzero')
    assert torch.is_tensor(only) and np.array_equal(only.cpu().numpy(), wd2)
    a = nuclei.distance_transform(t, sites='nonzero', max_distance=3, return_nearest=True)
    b = nuclei.distance_transform(t, sites='nonzero', max_distance=3, return_nearest=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    only3 = nuclei.distance_transform(t, sites='nonzero', max_distance=3)
    assert torch.equal(only3, a[0])


def test_empty_images():
    for shape in ((0, 5), (4, 0), (0, 0)):
        t = torch.zeros(shape, dtype=torch.uint8, device=DEV)
        d2, near = nuclei.distance_transform(t, return_nearest=True)
        assert tuple(d2.shape) == shape and tuple(near.shape) == shape and d2.dtype == near.dtype == torch.int32
        out = nuclei.expand_labels(t, 2)
        assert tuple(out.shape) == shape and out.dtype == torch.uint8
        lab, n = nuclei.split_touching(t, 2)
        assert tuple(lab.shape) == shape and lab.dtype == torch.int32 and n == 0


# ------------------------------------------------------------------ expand_labels
@pytest.mark.parametrize('distance', [0, 1, 2.5, 6])
def test_expand_labels_tissue(distance):
    labels, _, within = tissue()
    t = gpu(labels)
    for w in (None, within):
        out = nuclei.expand_labels(t, distance, within=None if w is None else gpu(w))
        assert out.dtype == t.dtype and out.device == t.device and tuple(out.shape) == labels.shape
        got = out.cpu().numpy()
        want = ref.expand_labels(labels, distance, within=w)
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
        assert np.array_equal(got[labels != 0], labels[labels != 0])           # labelled pixels never change
        if w is not None:
            assert (got[(labels == 0) & ~w] == 0).all()
    assert np.array_equal(t.cpu().numpy(), labels)                             # the input is left alone
    if distance == 0:
        assert np.array_equal(got, labels)


@pytest.mark.parametrize('dtype', [torch.uint8, torch.int16, torch.int32, torch.int64, torch.bool], ids=str)
def test_expand_labels_dtype(dtype):
    lab = np.zeros((40, 70), np.int64)
    lab[10, 10], lab[30, 50], lab[12, 60] = 3, 120, 77
    t = gpu(lab).to(dtype)
    out = nuclei.expand_labels(t, 4.5)
    assert out.dtype == dtype
    want = ref.expand_labels(t.cpu().numpy(), 4.5)
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize('gap', [1, 2, 3])
def test_expand_labels_facing_labels(gap):
    for transpose in (False, True):
        lab = np.zeros((70, 4 + gap), np.int32)
        lab[:, :2] = 9
        lab[:, 2 + gap:] = 4
        want = lab.copy()
        want[:, 2:2 + (gap + 1) // 2] = 9      # the middle of an odd gap is equally near to both: the smaller raster index decides,
        want[:, 2 + (gap + 1) // 2:2 + gap] = 4    # which is the left label, and the upper one after transposing
        if transpose:
            lab, want = np.ascontiguousarray(lab.T), np.ascontiguousarray(want.T)
        out = nuclei.expand_labels(gpu(lab), 5).cpu().numpy()
        assert np.array_equal(out, want)
        assert np.array_equal(out, ref.expand_labels(lab, 5))


# ------------------------------------------------------------------ split_touching
def test_split_two_discs():
    m = two_discs()
    t = gpu(m)
    assert nuclei.label_instances(t)[1] == 1
    d2 = nuclei.distance_transform(t)
    assert nuclei.label_instances(d2 > 49)[1] == 1 and nuclei.label_instances(d2 > 64)[1] == 2
    lab, n = nuclei.split_touching(t, 8)
    assert type(n) is int and n == 2 and lab.dtype == torch.int32
    got = lab.cpu().numpy()
    assert np.array_equal(got != 0, m)                                   # every mask pixel is labelled, nothing else is
    want, wn = ref.split_touching(m, 8)
    assert wn == 2 and np.array_equal(got, want)
    lab7, n7 = nuclei.split_touching(t, 7)
    want7, wn7 = ref.split_touching(m, 7)
    assert n7 == wn7 == 1 and np.array_equal(lab7.cpu().numpy(), want7)


@pytest.mark.parametrize('core_radius,connectivity,min_size', [(2, 1, 0), (4, 1, 0), (2, 2, 0), (4, 1, 10), (2.5, 2, 10)])
def test_split_tissue(core_radius, connectivity, min_size):
    labels, _, _ = tissue()
    m = labels > 0
    lab, n = nuclei.split_touching(gpu(m), core_radius, connectivity, min_size)
    want, wn = ref.split_touching(m, core_radius, connectivity, min_size)
    got = lab.cpu().numpy()
    assert n == wn and np.array_equal(got, want), (n, wn, np.argwhere(got != want)[:5])
    if min_size == 0:
        assert np.array_equal(got != 0, m)                               # no foreground pixel is dropped


@pytest.mark.parametrize('connectivity,min_size', [(1, 0), (2, 0), (1, 10)])
def test_split_radius_zero_is_label_instances(connectivity, min_size):
    labels, _, _ = tissue()
    for image in (gpu(labels > 0), gpu(labels)):
        lab, n = nuclei.split_touching(image, 0, connectivity, min_size)
        want, wn = nuclei.label_instances(image != 0, connectivity, min_size)
        assert n == wn and torch.equal(lab, want)


def test_split_feeds_nucleus_features():
    labels, gray, _ = tissue()
    lab, n = nuclei.split_touching(gpu(labels > 0), 3, min_size=10)
    assert n > nuclei.label_instances(gpu(labels > 0), min_size=10)[1]             # the tile has touching nuclei
    feats, cen, kept = nuclei.nucleus_features(lab, gpu(gray), max_label=n)
    assert tuple(feats.shape) == (n, nuclei.NUM_FEATURES) and tuple(cen.shape) == (n, 2)
    assert np.array_equal(kept.cpu().numpy(), np.arange(1, n + 1))


# ------------------------------------------------------------------ argument errors
def test_argument_errors():
    ok = torch.zeros(8, 9, dtype=torch.uint8, device=DEV)
    for fn in (lambda t: nuclei.distance_transform(t), lambda t: nuclei.expand_labels(t, 1), lambda t: nuclei.split_touching(t, 1)):
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 8, 9, dtype=torch.uint8, device=DEV))
        with pytest.raises(TypeError):
            fn(torch.zeros(8, 9, dtype=torch.float32, device=DEV))
        with pytest.raises(TypeError):
            fn(torch.zeros(8, 9, dtype=torch.uint8))
        with pytest.raises(TypeError):
            fn(np.zeros((8, 9), np.uint8))
        with pytest.raises(ValueError):
            fn(torch.zeros(1, 40000, dtype=torch.bool, device=DEV))
        with pytest.raises(ValueError):
            fn(torch.zeros(40000, 1, dtype=torch.bool, device=DEV))
    for bad in (-1, -0.5, float('nan')):
        with pytest.raises(ValueError):
            nuclei.distance_transform(ok, max_distance=bad)
        with pytest.raises(ValueError):
            nuclei.expand_labels(ok, bad)
        with pytest.raises(ValueError):
            nuclei.split_touching(ok, bad)
    with pytest.raises(ValueError):
        nuclei.distance_transform(ok, sites='both')
    with pytest.raises(ValueError):
        nuclei.expand_labels(ok, 1, within=torch.zeros(9, 8, dtype=torch.bool, device=DEV))
    with pytest.raises(TypeError):
        nuclei.expand_labels(ok, 1, within=torch.zeros(8, 9, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        nuclei.split_touching(ok, 1, connectivity=3)
    with pytest.raises(ValueError):
        nuclei.split_touching(ok, 1, min_size=-1)


def test_library_refuses_long_sides():
    from cgc_net_amd import kernels
    lib = kernels.get().lib
    assert lib.cgc_edt_ws_bytes(32767, 32767) > 0 and lib.cgc_edt_ws_bytes(32768, 1) == 0
    assert lib.cgc_edt(None, 1, 1, 40000, 0, -1, None, None, None, None) == -1           # CGC_EINVAL before anything is touched
    assert lib.cgc_edt(None, 3, 4, 4, 0, -1, None, None, None, None) == -1
