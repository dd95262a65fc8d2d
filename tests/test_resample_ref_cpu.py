"""CPU: pins tests/resample_ref.py, the restatement the GPU tests compare with bit for bit, against independent formulations: scipy's
zoom in float64, block means, a float64 coverage-matrix product, np.repeat, round trips, hand-written cases and Python integers.

Bounds.  The restatement rounds the exact rational value once, half up, so it lies within 1/2 level of that value; scipy's and the
coverage product's float64 results carry an error of a few 2^-53 * 255 < 1e-12 levels.  Both comparisons are therefore held to
1/2 + 1e-9 level."""
from fractions import Fraction

import numpy as np
import pytest
from scipy import ndimage

import resample_ref as ref

HALF = 0.5 + 1e-9


def image(H, W, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (H, W)).astype(np.uint8)


@pytest.mark.parametrize('shape,size', [((37, 53), (74, 106)), ((37, 53), (61, 40)), ((37, 53), (18, 26)), ((40, 64), (13, 9)),
                                        ((5, 7), (64, 3)), ((1, 9), (3, 4))])
def test_linear_against_scipy_zoom(shape, size):
    img = image(*shape, seed=1)
    want = ndimage.zoom(img.astype(np.float64), (size[0] / shape[0], size[1] / shape[1]), order=1, mode='nearest', grid_mode=True)
    assert want.shape == size
    diff = np.abs(ref.linear(img, size).astype(np.float64) - want).max()
    print('linear %s -> %s: largest difference %.15f' % (shape, size, diff))
    assert diff <= HALF


@pytest.mark.parametrize('fy,fx', [(2, 2), (3, 2), (8, 4)])
def test_area_integer_factors_are_block_means(fy, fx):
    img = image(5 * fy, 7 * fx, seed=2)
    blocks = img.reshape(5, fy, 7, fx).astype(np.int64).sum(axis=(1, 3))
    want = (2 * blocks + fy * fx) // (2 * fy * fx)
    assert np.array_equal(ref.area(img, (5, 7)), want)


def coverage(n, m):
    """[m, n] float64: the length of source pixel i inside [d n / m, (d + 1) n / m), over the box length n / m."""
    d, i = np.arange(m, dtype=np.float64)[:, None], np.arange(n, dtype=np.float64)[None, :]
    return np.clip(np.minimum((d + 1) * n / m, i + 1) - np.maximum(d * n / m, i), 0, None) * m / n


@pytest.mark.parametrize('shape,size', [((37, 53), (18, 26)), ((40, 64), (13, 9)), ((33, 33), (32, 1))])
def test_area_against_coverage_product(shape, size):
    img = image(*shape, seed=3)
    want = coverage(shape[0], size[0]) @ img.astype(np.float64) @ coverage(shape[1], size[1]).T
    diff = np.abs(ref.area(img, size).astype(np.float64) - want).max()
    print('area %s -> %s: largest difference %.6f' % (shape, size, diff))
    assert diff <= HALF


@pytest.mark.parametrize('k', [2, 3])
def test_nearest_upscale_is_repeat(k):
    lab = np.random.RandomState(4).randint(-5, 6, (9, 11)).astype(np.int32)
    assert np.array_equal(ref.nearest(lab, (9 * k, 11 * k)), np.repeat(np.repeat(lab, k, 0), k, 1))


def test_round_trips():
    img = image(11, 13, seed=5)
    lab = np.random.RandomState(6).randint(0, 4, (11, 13)).astype(np.int16)
    for ky, kx in ((2, 2), (3, 2), (8, 5)):
        up = np.repeat(np.repeat(img, ky, 0), kx, 1)
        assert np.array_equal(ref.area(up, img.shape), img)
        assert np.array_equal(ref.majority(np.repeat(np.repeat(lab, ky, 0), kx, 1), lab.shape), lab)
    for mode in ('linear', 'area'):
        assert np.array_equal(ref.resize(img, img.shape, mode), img)
    tile = np.stack([img, img[::-1], img[:, ::-1]], 2)
    for mode in ('linear', 'area'):
        assert np.array_equal(ref.resize(tile, img.shape, mode), tile)
    for mode in ('nearest', 'majority'):
        assert np.array_equal(ref.resize_labels(lab, lab.shape, mode), lab)
    assert np.array_equal(ref.majority(lab > 1, lab.shape), lab > 1)


def test_rounding_and_ties_by_hand():
    u8 = lambda a: np.array(a, np.uint8)
    assert ref.area(u8([[0, 255], [255, 0]]), (1, 1)).tolist() == [[128]]                  # 127.5 rounds up
    assert ref.linear(u8([[0, 255]]), (1, 4)).tolist() == [[0, 64, 191, 255]]              # 63.75, 191.25
    assert ref.majority(u8([[0, 5], [5, 0]]), (1, 1)).tolist() == [[0]]
    assert ref.majority(u8([[7, 5], [5, 7]]), (1, 1)).tolist() == [[5]]
    box = np.array([[9, 3, 9], [3, 1, 3], [9, 3, 9]], np.int32)                             # counts 4 / 4 / 1
    assert ref.majority(box, (1, 1)).tolist() == [[3]]
    assert ref.majority(np.array([[-2, 4], [4, -2]], np.int16), (1, 1)).tolist() == [[-2]]      # signed order
    assert ref.majority(np.array([[200, 4], [4, 200]], np.uint8), (1, 1)).tolist() == [[4]]     # unsigned order
    assert ref.majority(np.array([[True, False]]), (1, 1)).tolist() == [[False]]
    # fractional weights: 3 -> 2, the middle pixel is shared; [a, b, b] -> boxes {a: 2, b: 1}, {b: 3}
    assert ref.majority(np.array([[6, 2, 2]], np.int32), (1, 2)).tolist() == [[6, 2]]


def test_the_32_bit_edge_against_python_integers():
    n = 32767
    row = np.random.RandomState(7).randint(0, 256, (1, n)).astype(np.uint8)
    p = [int(v) for v in row[0]]
    m = 32766
    assert (2 * (m - 1) + 1) * n > 2 ** 31 - 2 ** 18                      # next to the int32 limit
    want = []
    for d in range(m):
        num = min(max((2 * d + 1) * n - m, 0), 2 * m * (n - 1))
        i0 = num // (2 * m)
        f = num - i0 * 2 * m
        S = (p[i0] * (2 * m - f) + p[min(i0 + 1, n - 1)] * f) * 2          # the row axis: H = H2 = 1, weight 2
        want.append((2 * S + 4 * m) // (8 * m))
    assert ref.linear(row, (1, m))[0].tolist() == want
    assert ref.nearest(row, (1, m))[0].tolist() == [p[(2 * d + 1) * n // (2 * m)] for d in range(m)]
    m = 16383
    want = []
    for d in range(m):
        S = sum(p[i] * (min((d + 1) * n, (i + 1) * m) - max(d * n, i * m)) for i in range(d * n // m, ((d + 1) * n - 1) // m + 1))
        want.append((2 * S + n) // (2 * n))
    assert ref.area(row, (1, m))[0].tolist() == want


def test_size_rule():
    assert ref.scaled_side(7, Fraction(1, 2)) == 4 and ref.scaled_side(5, Fraction(1, 2)) == 3 and ref.scaled_side(1, Fraction(1, 8)) == 1
    assert ref.scaled_side(10, 0.1) == 1 and ref.scaled_side(15, Fraction(1, 10)) == 2 and ref.scaled_side(15, 0.1) == 2
