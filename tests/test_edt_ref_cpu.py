"""CPU: tests/edt_ref.py, the oracle of the GPU distance transform, pinned to a brute force over all pixel-site pairs (distances and
the tie rule "smallest raster index") and to scipy.ndimage.distance_transform_edt; its expand_labels against the definition; the
two-disc case of split_touching."""
import numpy as np
import pytest
from scipy import ndimage

import edt_ref as ref
import label_ref

SHAPES = [(1, 1), (1, 9), (8, 1), (5, 7), (16, 16), (24, 24), (13, 22)]


def patterns(shape):
    H, W = shape
    for density in (0.0, 0.02, 0.3, 0.9, 1.0):
        yield np.random.RandomState(int(100 * density) + H * 31 + W).rand(H, W) < density
    for pitch in (2, 3):
        m = np.zeros(shape, bool)
        m[::pitch, ::pitch] = True
        yield m
    yy, xx = np.mgrid[0:H, 0:W]
    yield (yy + xx) % 2 == 0
    m = np.zeros(shape, bool)
    m[H - 1, W - 1] = True
    yield m


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_oracle_equals_brute_force(shape):
    for site in patterns(shape):
        bd2, bnear = ref.brute(site)
        for image, sites in ((site, 'nonzero'), (~site, 'zero'), (site.astype(np.int32) * 7, 'nonzero')):
            d2, near = ref.edt(image, sites)
            assert d2.dtype == np.int32 and near.dtype == np.int32
            assert np.array_equal(d2, bd2)
            assert np.array_equal(near, bnear), np.argwhere(near != bnear)[:5]
        if not site.any():
            assert (bd2 == ref.EDT_INF).all() and (bnear == -1).all()
        if site.all():
            assert (bd2 == 0).all() and np.array_equal(bnear.ravel(), np.arange(site.size))


def test_oracle_dist2_equals_scipy():
    for seed, shape in enumerate([(40, 57), (64, 64), (3, 200), (130, 7)]):
        site = np.random.RandomState(seed).rand(*shape) < 0.03
        d2, near = ref.edt(site, 'nonzero')
        want = ndimage.distance_transform_edt(~site)
        assert np.array_equal(d2, np.rint(want * want).astype(np.int32))
        assert np.array_equal(np.sqrt(d2.astype(np.float64)), want)
        H, W = shape
        ny, nx = np.divmod(near, W)
        yy, xx = np.mgrid[0:H, 0:W]
        assert site[ny, nx].all() and np.array_equal((yy - ny) ** 2 + (xx - nx) ** 2, d2)


@pytest.mark.parametrize('max_distance', [0, 1, 1.5, 2 ** 0.5, 3])
def test_oracle_bound(max_distance):
    site = np.random.RandomState(3).rand(20, 23) < 0.02
    d2, near = ref.edt(site, 'nonzero')
    b2, bnear = ref.edt(site, 'nonzero', max_distance)
    keep = d2 <= int(np.floor(max_distance * max_distance + 1e-9))
    assert np.array_equal(b2, np.where(keep, d2, ref.EDT_INF)) and np.array_equal(bnear, np.where(keep, near, -1))


def test_oracle_expand_labels_ties_and_within():
    for gap in (1, 2, 3):
        lab = np.zeros((5, 4 + gap), np.int16)
        lab[:, :2] = 9
        lab[:, 2 + gap:] = 4
        out = ref.expand_labels(lab, 5)
        assert out.dtype == lab.dtype and (out != 0).all()
        want = lab.copy()
        want[:, 2:2 + (gap + 1) // 2] = 9        # the middle column of an odd gap is equally near: the left site has the smaller index
        want[:, 2 + (gap + 1) // 2:2 + gap] = 4
        assert np.array_equal(out, want)
    lab = np.zeros((7, 7), np.int32)
    lab[3, 3] = 5
    assert (ref.expand_labels(lab, 1) != 0).sum() == 5 and (ref.expand_labels(lab, 2 ** 0.5) != 0).sum() == 9
    within = np.zeros((7, 7), bool)
    within[3] = True
    out = ref.expand_labels(lab, 2, within=within)
    assert np.array_equal(np.argwhere(out != 0), [[3, 1], [3, 2], [3, 3], [3, 4], [3, 5]])


def two_discs():
    yy, xx = np.mgrid[0:48, 0:48]
    return ((yy - 24) ** 2 + (xx - 17) ** 2 <= 100) | ((yy - 24) ** 2 + (xx - 31) ** 2 <= 100)


def test_oracle_two_discs():
    m = two_discs()
    assert label_ref.label(m)[1] == 1
    dist = ndimage.distance_transform_edt(m)
    assert ndimage.label(dist > 7)[1] == 1 and ndimage.label(dist > 8)[1] == 2
    lab7, n7 = ref.split_touching(m, 7)
    lab, n = ref.split_touching(m, 8)
    assert n == 2 and np.array_equal(lab != 0, m)
    assert np.array_equal(lab7 != 0, m)
    left, right = lab[24, 10], lab[24, 38]
    assert {left, right} == {1, 2}
    assert (lab[:, :20][m[:, :20]] == left).all() and (lab[:, 29:][m[:, 29:]] == right).all()
    lab0, n0 = ref.split_touching(m, 0)
    want, wn, _ = label_ref.label(m)
    assert n0 == wn and np.array_equal(lab0, want)
