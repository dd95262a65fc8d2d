"""CPU: pins tests/reconstruct_ref.py, the oracle of the morphological-reconstruction stage, to independent statements of the same
definitions: scipy's binary propagation and hole filling on 0/1 images, a brute-force max-min path closure on tiny gray images, a
plateau labelling for the regional maxima, and Python's integer square root for the distance in eighths of a pixel."""
import math

import numpy as np
import pytest
from scipy import ndimage

import reconstruct_ref as ref

INT32_MIN, INT32_MAX = ref.INT32_MIN, ref.INT32_MAX


@pytest.mark.parametrize('connectivity', [1, 2])
def test_binary_images_against_binary_propagation(connectivity):
    rng = np.random.RandomState(3 + connectivity)
    for shape, fill in (((1, 1), 0.5), ((1, 9), 0.7), ((13, 1), 0.7), ((17, 23), 0.6), ((40, 31), 0.55), ((40, 31), 0.8)):
        mask = rng.rand(*shape) < fill
        marker = mask & (rng.rand(*shape) < 0.05)
        want = ndimage.binary_propagation(marker, structure=ref.FOOTPRINTS[connectivity], mask=mask)
        got = ref.reconstruct(marker, mask, 'dilation', connectivity)
        assert np.array_equal(got != 0, want) and set(np.unique(got)) <= {0, 1}
        # the dual: erosion of the complements
        ero = ref.reconstruct(~marker, ~mask, 'erosion', connectivity)
        assert np.array_equal(ero != 0, ~want)


@pytest.mark.parametrize('connectivity', [1, 2])
def test_gray_images_against_the_path_closure(connectivity):
    rng = np.random.RandomState(11 + connectivity)
    for shape in ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 4), (7, 7), (6, 7)):
        for kind in range(3):
            if kind == 0:
                mask = rng.randint(0, 3, size=shape).astype(np.int64)
            elif kind == 1:
                mask = rng.randint(-50, 50, size=shape).astype(np.int64)
            else:
                mask = rng.randint(INT32_MIN, INT32_MAX + 1, size=shape, dtype=np.int64)
                mask.ravel()[rng.randint(mask.size)] = INT32_MIN
                mask.ravel()[rng.randint(mask.size)] = INT32_MAX
            low = max(int(mask.min()) - 5, INT32_MIN)
            marker = np.where(rng.rand(*shape) < 0.3, mask - rng.randint(0, 4, size=shape), low)
            marker = np.clip(marker, INT32_MIN, INT32_MAX)
            marker[rng.rand(*shape) < 0.1] = INT32_MAX                  # above the mask: clamped
            got = ref.reconstruct(marker, mask, 'dilation', connectivity)
            assert np.array_equal(got, ref.brute_closure(marker, mask, connectivity)), (shape, kind)
            assert (got <= mask).all() and (got >= np.minimum(marker, mask)).all()
            ero = ref.reconstruct(marker, mask, 'erosion', connectivity)
            assert np.array_equal(ero, ~ref.brute_closure(~marker, ~mask, connectivity)), (shape, kind)
            assert (ero >= mask).all() and (ero <= np.maximum(marker, mask)).all()


def test_corner_contact_conducts_only_with_eight_neighbours():
    mask = np.zeros((4, 4), np.int64)
    mask[0, 0] = mask[1, 1] = mask[2, 2] = 9
    marker = np.full((4, 4), -1, np.int64)
    marker[0, 0] = 7
    r1 = ref.reconstruct(marker, mask, 'dilation', 1)
    r2 = ref.reconstruct(marker, mask, 'dilation', 2)
    assert r1[0, 0] == 7 and r1[1, 1] == 0 and r1[2, 2] == 0
    assert r2[0, 0] == r2[1, 1] == r2[2, 2] == 7 and r2[0, 1] == 0


@pytest.mark.parametrize('connectivity', [1, 2])
def test_regional_maxima_against_plateau_labelling(connectivity):
    rng = np.random.RandomState(29 + connectivity)
    for shape, levels in (((1, 1), 2), ((1, 12), 3), ((9, 1), 3), ((12, 15), 2), ((20, 17), 4), ((25, 25), 50)):
        image = rng.randint(0, levels, size=shape)
        assert np.array_equal(ref.regional_maxima(image, connectivity), ref.plateau_maxima(image, connectivity))
    wide = rng.randint(INT32_MIN, INT32_MAX + 1, size=(15, 14), dtype=np.int64)
    wide[3, 3], wide[9, 9] = INT32_MIN, INT32_MAX
    assert np.array_equal(ref.regional_maxima(wide, connectivity), ref.plateau_maxima(wide, connectivity))
    flat = np.full((5, 6), 4)
    assert ref.regional_maxima(flat, connectivity).all()


def test_h_maxima_counts_the_dynamic():
    row = np.array([[0, 5, 5, 3, 9, 9, 2, 4, 0]])                       # summits 5 (dynamic 2), 9 (highest), 4 (dynamic 2)
    for h, want in ((1, [0, 1, 1, 0, 1, 1, 0, 1, 0]), (2, [0, 1, 1, 0, 1, 1, 0, 1, 0]), (3, [0, 0, 0, 0, 1, 1, 0, 0, 0]),
                    (9, [0, 0, 0, 0, 1, 1, 0, 0, 0]), (INT32_MAX, [0, 0, 0, 0, 1, 1, 0, 0, 0])):
        assert ref.h_maxima(row, h).astype(int).tolist() == [want], h
    low = np.array([[INT32_MIN, INT32_MIN + 3, INT32_MIN]])              # image - h saturates: nothing stands h above the floor
    assert not ref.h_maxima(low, 10).any() and ref.h_maxima(low, 3)[0, 1]


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_fill_holes_against_scipy(seed):
    rng = np.random.RandomState(seed)
    for shape, fill in (((1, 1), 0.5), ((1, 8), 0.5), ((3, 3), 0.7), ((30, 41), 0.45), ((30, 41), 0.6), ((50, 50), 0.75)):
        image = rng.rand(*shape) < fill
        assert np.array_equal(ref.fill_holes(image, 1), ndimage.binary_fill_holes(image))
        want2 = ndimage.binary_fill_holes(image, structure=ref.FOOTPRINTS[2])          # background joined over corners too
        assert np.array_equal(ref.fill_holes(image, 2), want2)
    ring = np.zeros((7, 7), bool)
    ring[1:6, 1:6] = True
    ring[2:5, 2:5] = False
    assert ref.fill_holes(ring).sum() == 25
    ring[1, 1] = False                                                  # a diagonal gap: closed for 4 neighbours, open for 8
    assert ref.fill_holes(ring, 1).sum() == 24 and np.array_equal(ref.fill_holes(ring, 2), ring)


def test_fill_holes_of_an_instance_mask():
    lab = np.zeros((9, 12), np.int32)
    lab[1:8, 1:6], lab[1:8, 6:11] = 3, 8
    lab[3:6, 3:9] = 0                                                   # one hole between two labels
    out = ref.fill_holes(lab)
    assert (out[3:6, 3:6] == 3).all() and (out[3:6, 6:9] == 8).all()
    assert np.array_equal(out[lab != 0], lab[lab != 0]) and (out[0] == 0).all() and out.dtype == lab.dtype


def test_eighths_is_the_integer_square_root():
    d = np.array([0, 1, 2, 3, 4, 5, 99, 100, 101, 2 ** 20 - 1, 2 ** 20, 2 ** 31 - 2, 2 ** 31 - 1], np.int64)
    t = ref.eighths(d)
    assert t.dtype == np.int32 and t.tolist() == [math.isqrt(64 * int(v)) for v in d]
    assert all(int(a) ** 2 <= 64 * int(v) < (int(a) + 1) ** 2 for a, v in zip(t, d))
    assert [ref.h8_of(h) for h in (0.125, 0.2, 1, 1.5, 2.99, 3)] == [1, 1, 8, 12, 23, 24]
