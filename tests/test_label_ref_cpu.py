"""tests/label_ref.py, the oracle of the GPU labelling tests, against a brute-force flood fill on small images."""
import numpy as np
import pytest

import label_ref as ref


def _images():
    rng = np.random.RandomState(0)
    for k in range(60):
        H, W = rng.randint(1, 13), rng.randint(1, 13)
        yield (rng.rand(H, W) < rng.choice([0.2, 0.45, 0.59, 0.8])), 'bool %d' % k
        yield rng.randint(0, 4, size=(H, W)).astype(np.int32), 'int %d' % k
        yield rng.randint(-2, 3, size=(H, W)).astype(np.int64), 'signed %d' % k


@pytest.mark.parametrize('connectivity', [1, 2])
def test_oracle_equals_flood_fill(connectivity):
    for img, name in _images():
        lab, n, sizes = ref.label(img, connectivity)
        flab, fn = ref.flood_fill(img, connectivity)
        assert n == fn and np.array_equal(lab, flab), name
        assert np.array_equal(sizes, np.bincount(flab.ravel(), minlength=fn + 1)[1:]), name


@pytest.mark.parametrize('connectivity', [1, 2])
@pytest.mark.parametrize('min_size', [1, 2, 4])
def test_oracle_min_size_equals_filtered_flood_fill(connectivity, min_size):
    for img, name in _images():
        lab, n, sizes = ref.label(img, connectivity, min_size)
        flab, fn = ref.flood_fill(img, connectivity)
        counts = np.bincount(flab.ravel(), minlength=fn + 1)
        keep = counts >= min_size
        keep[0] = False
        new = np.zeros(fn + 1, np.int32)
        new[keep] = np.arange(1, keep.sum() + 1)          # flood-fill numbers are in first-pixel order already
        assert n == int(keep.sum()) and np.array_equal(lab, new[flab]), name
        assert np.array_equal(sizes, counts[keep]), name


def test_binary_image_is_scipy_label_itself():
    from scipy import ndimage
    rng = np.random.RandomState(3)
    img = rng.rand(40, 50) < 0.55
    for c in (1, 2):
        want, n = ndimage.label(img, structure=ndimage.generate_binary_structure(2, c))
        lab, k, _ = ref.label(img, c)
        assert k == n and np.array_equal(lab, want)
    assert ref.label(np.zeros((0, 5), bool))[1] == 0 and ref.label(np.zeros((4, 4), np.uint8))[1] == 0
