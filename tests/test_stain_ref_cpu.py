"""CPU: pins tests/stain_ref.py, the reference the GPU tests of the stain front end compare against (tests/test_stain_gpu.py), and the
host-side tables of cgc_net_amd.nuclei (OD_LUT, stain_matrix, the Otsu decision)."""
import math
from fractions import Fraction

import numpy as np
import pytest
from scipy.ndimage import correlate1d

import cgc_net_amd  # noqa: F401
from cgc_net_amd import nuclei

import stain_ref as ref

OTHER_STAINS = ((0.9, 0.3, 0.3), (0.2, 0.9, 0.4), (0.3, 0.3, 0.9))      # the inverse's column absolute sums: 1.77, 2.01, 2.21


def test_od_lut():
    lut = ref.od_lut()
    assert tuple(lut.tolist()) == nuclei.OD_LUT
    assert lut[255] == 0 and lut[0] == lut[1] == ref.OD_MAX == lut.max() and (np.diff(lut[1:]) <= 0).all()
    # floor(x + 0.5) changes where x + 0.5 is an integer: no entry comes near, so a libm that is off by an ulp gives the same table
    for v in range(256):
        x = 1024.0 * math.log(255.0 / max(v, 1)) + 0.5
        assert min(x - math.floor(x), math.ceil(x) - x) > 1e-4 or x == math.floor(x) + 0.5, v


def test_default_matrix():
    want = [[7679, -4121, -2285], [-270, 4641, -557], [-2461, -1965, 6465]]
    assert ref.stain_matrix().tolist() == want
    m = nuclei.stain_matrix()
    assert m.dtype == np.int32 and m.tolist() == want
    assert nuclei.stain_matrix(nuclei.DEFAULT_STAINS).tolist() == want
    assert nuclei.stain_matrix(10.0 * np.array(nuclei.DEFAULT_STAINS)).tolist() == want      # rows are normalised
    assert nuclei.stain_matrix(OTHER_STAINS).tolist() == ref.stain_matrix(OTHER_STAINS).tolist()


def _pixels():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    corners = np.array([[a, b, c] for a in (0, 255) for b in (0, 255) for c in (0, 255)], np.uint8)
    rnd = np.random.RandomState(0).randint(0, 256, (200000, 3)).astype(np.uint8)
    return np.concatenate([grey, corners, rnd])


@pytest.mark.parametrize('stains', [ref.DEFAULT_STAINS, OTHER_STAINS])
def test_within_one_level_of_the_float_formula(stains):
    """(a / 2048 + 3 * 5.55 / 8192) * 64 + 1/2 < 1 for a column absolute sum a <= 4 of inv(S): the table's rounding through the
    matrix, the matrix's rounding times the largest OD, and the final rounding."""
    S = np.array(stains, np.float64)
    S = S / np.sqrt((S * S).sum(axis=1))[:, None]
    a = np.abs(np.linalg.inv(S)).sum(axis=0).max()
    assert a <= 4 and (a * 0.5 / 1024 + 3 * 5.55 * 0.5 / 4096) * 64 + 0.5 < 1
    pix = _pixels()
    M = ref.stain_matrix(stains)
    for order in (0, 1):
        err = np.abs(ref.separate(pix, M, order).astype(np.float64) - ref.separate_float(pix, stains, order)).max()
        print('order %d: largest difference %.4f levels' % (order, err))
        assert err < 1.0
    assert np.array_equal(ref.separate(pix, M, 0), ref.separate(pix[:, ::-1], M, 1))
    assert np.array_equal(ref.separate(pix, M, 0, (0, 2)), ref.separate(pix, M, 0)[[0, 2]])


def test_one_level_is_a_64th_of_a_unit():
    tile = ref.render_tile(np.ones((1, 1)), c_nucleus=2.1, c_eosin=0.0)
    h, e, r = ref.separate(tile, ref.stain_matrix())[:, 0, 0]
    assert abs(int(h) - 2.1 * 64) <= 2 and e <= 2 and r <= 2


@pytest.mark.parametrize('radius', range(6))
@pytest.mark.parametrize('shape', [(1, 1), (1, 9), (9, 1), (3, 4), (70, 66)])
def test_binomial_smooth_is_two_correlations_and_one_rounding(radius, shape):
    img = np.random.RandomState(radius * 100 + shape[0]).randint(0, 256, shape).astype(np.uint8)
    w = np.array([math.comb(2 * radius, k) for k in range(2 * radius + 1)], np.int64)
    assert w.sum() == 4 ** radius
    a = correlate1d(correlate1d(img.astype(np.int64), w, axis=1, mode='nearest'), w, axis=0, mode='nearest')
    if radius:
        a = (a + (1 << (4 * radius - 1))) >> (4 * radius)
    out = ref.binomial_smooth(img, radius)
    assert out.dtype == np.uint8 and np.array_equal(out, a)
    if radius == 0:
        assert np.array_equal(out, img)
    flat = np.full(shape, 255, np.uint8)
    assert np.array_equal(ref.binomial_smooth(flat, radius), flat)                # the largest sum still fits and rounds to 255


def test_histogram():
    img = np.random.RandomState(1).randint(0, 256, (37, 41)).astype(np.uint8)
    within = np.random.RandomState(2).rand(37, 41) < 0.3
    h = ref.histogram(img)
    assert h.sum() == img.size and h[17] == (img == 17).sum()
    hw = ref.histogram(img, within)
    assert hw.sum() == within.sum() and hw[17] == ((img == 17) & within).sum()
    assert ref.histogram(img, np.zeros_like(within)).sum() == 0


def _counts(**bins):
    h = [0] * 256
    for v, c in bins.items():
        h[int(v[1:])] = c
    return h


@pytest.mark.parametrize('otsu', [ref.otsu, nuclei._otsu], ids=['reference', 'package'])
def test_otsu_cases(otsu):
    assert otsu(_counts(v40=10, v200=3)) == 40                 # two values: every t in 40..199 scores the same, the smallest wins
    assert otsu(_counts(v0=1, v255=1)) == 0
    assert otsu(_counts(v254=5, v255=1)) == 254
    for v in (0, 7, 255):
        assert otsu(_counts(**{'v%d' % v: 9})) == v           # one value: that value, nothing is above it
    assert otsu([0] * 256) == 0                                # an empty selection
    # an exact tie between two different cuts: the histogram is symmetric, so cutting below the middle value (t = 10..19) and above
    # it (t = 20..29) score the same, 20000 / 3: the smallest t wins
    h = _counts(v10=4, v20=2, v30=4)
    n = sum(h)
    s = sum(v * c for v, c in enumerate(h))

    def score(t):
        w0, s0 = sum(h[:t + 1]), sum(v * h[v] for v in range(t + 1))
        return Fraction((w0 * s - n * s0) ** 2, w0 * (n - w0))

    assert score(10) == score(19) == score(20) == score(29) == Fraction(20000, 3)
    assert otsu(h) == 10


@pytest.mark.parametrize('seed', range(4))
def test_otsu_random_histograms_against_brute_force(seed):
    rng = np.random.RandomState(seed)
    h = rng.randint(0, 10 ** (2 + 2 * seed), 256)
    if seed == 3:
        h[rng.rand(256) < 0.8] = 0                             # sparse: many t have equal w0
    n, s = int(h.sum()), int((np.arange(256) * h).sum())
    best, best_t = None, None
    for t in range(255):
        w0, s0 = int(h[:t + 1].sum()), int((np.arange(t + 1) * h[:t + 1]).sum())
        if 0 < w0 < n:
            f = Fraction((w0 * s - n * s0) ** 2, w0 * (n - w0))
            if best is None or f > best:
                best, best_t = f, t
    assert ref.otsu(h) == best_t == nuclei._otsu(h)


def test_end_to_end_on_a_rendered_tile():
    labels, tile, within = ref.tile_case()
    assert tile.shape == (192, 160, 3) and tile.dtype == np.uint8
    fg, t, plane = ref.stain_foreground(tile, radius=0)
    assert len(np.unique(plane)) == 2 and t == plane.min()     # noise free: one level per class
    assert np.array_equal(fg, labels > 0)
    fgw, tw, _ = ref.stain_foreground(tile, radius=0, within=within)
    assert tw == t and np.array_equal(fgw, fg)
    rgb = ref.render_tile(labels, order=1)
    assert np.array_equal(rgb, tile[..., ::-1])
    assert np.array_equal(ref.stain_foreground(rgb, radius=0, order=1)[0], fg)
    fg2, t2, plane2 = ref.stain_foreground(tile, radius=2)
    assert plane.min() < t2 < plane.max() and (fg2 != fg).mean() < 0.05      # smoothing only moves the rim
