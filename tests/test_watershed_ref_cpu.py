"""CPU: pins tests/watershed_ref.py, the oracle of the seeded-watershed stage, to independent statements of the same contract
(kernels.KernelSpec.watershed_flood): a relaxation in shuffled order reaches the keys of the Dijkstra sweep, the level is the
reconstruction by erosion of the height under the seeds, the reached set is the seeded components of the domain, every region is
8-connected, every parent has a strictly smaller key, and on two touching discs of unequal size the flood cuts at the neck where the
geodesic growth cuts on the midline."""
import functools

import numpy as np
import pytest
from scipy import ndimage

import edt_ref
import geodesic_ref
import reconstruct_ref
import watershed_ref as ref

INT32_MIN, INT32_MAX = ref.INT32_MIN, ref.INT32_MAX
EIGHT = ndimage.generate_binary_structure(2, 2)


def random_case(rng, i):
    """(height, seeds, within or None, connectivity, metric): 1..11 x 1..11 pixels, heights in 0..3 or constant, random domains."""
    shape = (rng.randint(1, 12), rng.randint(1, 12))
    kind = rng.randint(6)
    if kind == 4:
        height = np.full(shape, 5, np.int64)
    elif kind == 5:
        height = np.full(shape, INT32_MIN, np.int64)
    else:
        height = rng.randint(0, 4, size=shape).astype(np.int64)
    seeds = rng.rand(*shape) < rng.choice([0.03, 0.1, 0.3])
    if rng.randint(5) != 4:                                                # every fifth case may have no seed at all
        seeds.ravel()[rng.randint(seeds.size)] = True
    within = None if rng.randint(3) == 0 else rng.rand(*shape) < rng.choice([0.5, 0.7, 0.9])
    metric = ('chamfer', 'cityblock', 'chessboard', (3, 4))[rng.randint(4)]
    return height, seeds, within, 1 + i % 2, metric


CASES = 72


@functools.lru_cache(maxsize=None)
def solved(i):
    height, seeds, within, connectivity, metric = random_case(np.random.RandomState(1000 + i), i)
    keys = ref.flood_keys(height, seeds, within, metric, connectivity)
    level, source = ref.flood(height, seeds, within, metric, connectivity)
    return height, seeds, within, connectivity, metric, keys, level, source


def test_relaxation_in_shuffled_order_gives_the_keys_of_dijkstra():
    seen = set()
    for i in range(CASES):
        height, seeds, within, connectivity, metric, keys, _, _ = solved(i)
        for trial in range(2):
            got = ref.relax_shuffled(height, seeds, within, metric, connectivity, np.random.RandomState(77 * i + trial))
            assert got == keys, (i, trial)
        seen.add((connectivity, int(height.min()) == INT32_MIN, within is None))
    assert len(seen) == 8                                                # both connectivities x INT32_MIN or not x with and without a domain


def test_level_is_the_reconstruction_by_erosion():
    checked = 0
    for i in range(3 * CASES):
        rng = np.random.RandomState(5000 + i)
        height, seeds, _, _, _ = random_case(rng, i)
        if i % 3 == 2:
            height = rng.randint(INT32_MIN, INT32_MAX + 1, size=height.shape, dtype=np.int64)
        for metric, connectivity in (('chamfer', 2), ('chessboard', 2), ('cityblock', 1)):
            level, source = ref.flood(height, seeds, None, metric, connectivity)
            g = np.where(seeds, INT32_MIN, INT32_MAX).astype(np.int64)
            want = reconstruct_ref.reconstruct(g, np.minimum(height, g), 'erosion', connectivity)
            wet = (source >= 0) & ~seeds
            assert np.array_equal(level[wet], want[wet]), (i, metric)
            assert np.array_equal(level[~wet], height[~wet].astype(np.int32))      # height on seeds and where no seed reaches
            checked += int(wet.sum())
    assert checked > 5000


def test_reached_set_is_the_seeded_components():
    for i in range(CASES):
        height, seeds, within, connectivity, metric, keys, level, source = solved(i)
        comp = 1 if geodesic_ref.steps_of(metric)[1] == 0 else connectivity      # without diagonal steps: the 4-connected components
        want = geodesic_ref.seeded_components(seeds, within, comp)
        assert np.array_equal(source >= 0, want), i
        W = seeds.shape[1]
        assert all(source[p // W, p % W] == p for p in keys if seeds[p // W, p % W])       # a seed is its own root
        assert seeds.ravel()[source[source >= 0]].all()                                    # every root is a seed
        if not seeds.any():
            assert (source == -1).all() and np.array_equal(level, height)


def test_regions_are_8_connected():
    split4 = 0
    for i in range(CASES):
        _, seeds, _, connectivity, _, _, _, source = solved(i)
        for s in np.unique(source[source >= 0]):
            assert ndimage.label(source == s, structure=EIGHT)[1] == 1, (i, s)
            split4 += ndimage.label(source == s)[1] > 1
    assert split4 > 0                                                    # not necessarily 4-connected: a diagonal step passes beside another region


def test_every_parent_has_a_strictly_smaller_key():
    for i in range(CASES):
        height, seeds, within, connectivity, metric, keys, _, source = solved(i)
        parent = ref.parents_of(keys, height, seeds, within, metric, connectivity)
        W = seeds.shape[1]
        assert set(parent) == set(keys)
        for p, q in parent.items():
            if seeds[p // W, p % W]:
                assert q == p and keys[p] == ref.SEED_KEY
            else:
                assert keys[q] < keys[p] and keys[p] == ref.extend(keys[q], int(height[p // W, p % W]), _cost(p, q, W, metric))
        root = ref.roots_of(parent)
        assert all(source[p // W, p % W] == r for p, r in root.items())


def _cost(p, q, W, metric):
    a, b = geodesic_ref.steps_of(metric)
    return a if (p // W == q // W or p % W == q % W) else b


def test_a_rim_pixel_follows_the_steepest_descent():
    """A bowl with a seed at the bottom: the pixel on the rim takes as parent the lower neighbour that was flooded first, not the
    first of its lower neighbours in raster order."""
    height = np.array([[9, 9, 9, 9, 9],
                       [9, 3, 2, 1, 9],
                       [9, 9, 9, 0, 9]], np.int64)
    seeds = np.zeros(height.shape, bool)
    seeds[2, 3] = True
    keys = ref.flood_keys(height, seeds, None, 'chamfer', 2)
    parent = ref.parents_of(keys, height, seeds, None, 'chamfer', 2)
    assert keys[1 * 5 + 3] == (1, 0) and keys[1 * 5 + 2] == (2, 0) and keys[1 * 5 + 1] == (3, 0)
    assert parent[0 * 5 + 2] == 1 * 5 + 3                # (0, 2) at 9: offers (9, 0) from (1, 1), (1, 2), (1, 3); (1, 3) was flooded first
    assert parent[0 * 5 + 0] == 1 * 5 + 1                # (0, 0): (1, 1) at level 3 beats its level-9 neighbours


def test_two_discs_are_cut_at_the_neck():
    mask, big = ref.disc_pair()
    d2 = edt_ref.dist2_scipy(~mask)
    assert abs(35 + int(np.argmin(d2[35, 35:76])) - ref.NECK) <= 1           # the distance map's minimum between the centres: column 62
    lab, n = ref.split_touching_flood(mask, None, markers='h_maxima', h=2)
    assert n == 2 and np.array_equal(lab > 0, mask)
    cut, large, small = ref.cut_of(lab)
    assert abs(cut - ref.NECK) <= 2 and abs(large - big) <= 0.01 * big and large + small == mask.sum()
    glab, gn = reconstruct_ref.split_touching_h_maxima(mask, 2)
    gcut, glarge, gsmall = ref.cut_of(glab)
    assert gn == 2 and gcut == 55 and gcut < ref.NECK - 2                    # the geodesic midline lies inside the large disc
    assert big - glarge > 0.05 * big and glarge + gsmall == mask.sum()   # and hands its pixels to the small one
