"""CPU: tests/shape_ref.py, the numpy restatement of the region geometry and of region_shape, pinned against per-pixel Python
loops, scipy.ndimage (each region taken as a binary mask), scipy.spatial.ConvexHull and cases whose numbers are written out here."""
import math

import numpy as np
import pytest
from scipy import ndimage
from scipy.spatial import ConvexHull

import shape_ref as ref

FOUR = ndimage.generate_binary_structure(2, 1)
EIGHT = ndimage.generate_binary_structure(2, 2)


def loops(labels, max_label, within=None):
    """The tables by the definition, one pixel and one quad at a time."""
    H, W = labels.shape
    R = max_label + 1
    g = dict(count=np.zeros(R, np.int32), border=np.zeros(R, np.int32), quads=np.zeros((R, 4), np.int32),
             extents=np.zeros((R, 8, 2), np.int32))
    for k in ('sy', 'sx', 'syy', 'sxy', 'sxx'):
        g[k] = np.zeros(R, np.int64)

    def at(y, x):
        if not (0 <= y < H and 0 <= x < W) or not 0 <= labels[y, x] <= max_label or (within is not None and not within[y, x]):
            return None
        return int(labels[y, x])

    for y in range(H):
        for x in range(W):
            L = at(y, x)
            if L is None:
                continue
            for k, (a, b) in enumerate(ref.DIRECTIONS):
                v = a * x + b * y
                g['extents'][L, k] = (v, v) if g['count'][L] == 0 else (min(g['extents'][L, k, 0], v), max(g['extents'][L, k, 1], v))
            g['count'][L] += 1
            g['sy'][L] += y
            g['sx'][L] += x
            g['syy'][L] += y * y
            g['sxy'][L] += x * y
            g['sxx'][L] += x * x
            g['border'][L] += int(y in (0, H - 1) or x in (0, W - 1))
    for y in range(-1, H):
        for x in range(-1, W):
            p = [at(y, x), at(y, x + 1), at(y + 1, x), at(y + 1, x + 1)]
            for L in set(p) - {None}:
                m = [v == L for v in p]
                n = sum(m)
                if n == 1:
                    g['quads'][L, 0] += 1
                elif n == 3:
                    g['quads'][L, 3] += 1
                elif n == 2:
                    g['quads'][L, 2 if m in ([True, False, False, True], [False, True, True, False]) else 1] += 1
    return g


def same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


def one_region(mask):
    """(geometry, shape in float64) of row 1 of a binary mask."""
    g = ref.geometry(np.asarray(mask).astype(np.int32), 1)
    return {k: v[1] for k, v in g.items()}, {k: (v[1] if isinstance(v, np.ndarray) else v) for k, v in ref.shape(g).items()}


# ------------------------------------------------------------------ against loops
@pytest.mark.parametrize('seed', range(6))
def test_tables_against_per_pixel_loops(seed):
    rng = np.random.RandomState(seed)
    H, W = rng.randint(1, 9, 2)
    labels = rng.randint(-1, 5, (H, W)).astype(np.int32)             # -1 and 4 lie outside [0, 3]
    same(ref.geometry(labels, 3), loops(labels, 3))
    within = rng.rand(H, W) < 0.6
    same(ref.geometry(labels, 3, within), loops(labels, 3, within))
    assert ref.refused(labels, 3) == int(((labels < 0) | (labels > 3)).sum())


def test_empty_images_and_empty_rows():
    for shape in ((0, 5), (5, 0), (0, 0)):
        g = ref.geometry(np.zeros(shape, np.int32), 2)
        assert all(not v.any() for v in g.values()) and g['extents'].shape == (3, 8, 2) and g['quads'].shape == (3, 4)
    g = ref.geometry(np.full((3, 3), 2, np.int32), 4)
    s = ref.shape(g)
    for r in (0, 1, 3, 4):
        assert all(not np.any(v[r]) for v in g.values())
        assert all(not np.any(s[k][r]) for k in ref.SHAPE_FLOATS + ref.SHAPE_INTS)
    assert not ref.features(s)[[0, 1, 3, 4]].any()


# ------------------------------------------------------------------ against scipy.ndimage, region by region
def holes(mask, structure):
    """The bounded components of the complement, by ``structure``."""
    comp, n = ndimage.label(~np.pad(mask, 1), structure=structure)
    return n - 1                                                     # the padding joins everything unbounded into one


@pytest.mark.parametrize('seed', range(8))
def test_regions_against_ndimage(seed):
    rng = np.random.RandomState(100 + seed)
    H, W = rng.randint(3, 14, 2)
    labels = rng.randint(0, 4, (H, W)).astype(np.int32)
    g = ref.geometry(labels, 3)
    s = ref.shape(g)
    full = ref.n4(g)
    for L in range(4):
        mask = labels == L
        if not mask.any():
            continue
        sl = ndimage.find_objects(mask.astype(np.int32))[0]
        assert s['bbox'][L].tolist() == [sl[0].start, sl[1].start, sl[0].stop, sl[1].stop]
        cy, cx = ndimage.center_of_mass(mask)
        assert abs(s['centroid_y'][L] - cy) < 1e-12 and abs(s['centroid_x'][L] - cx) < 1e-12
        assert 4 * s['euler4'][L] == 4 * (ndimage.label(mask, structure=FOUR)[1] - holes(mask, EIGHT))
        assert 4 * s['euler8'][L] == 4 * (ndimage.label(mask, structure=EIGHT)[1] - holes(mask, FOUR))
        p = np.pad(mask, 1)
        assert s['perimeter_crack'][L] == int((p[1:] != p[:-1]).sum() + (p[:, 1:] != p[:, :-1]).sum())
        n1, n2, nd, n3 = g['quads'][L].tolist()
        assert n1 + 2 * n2 + 2 * nd + 3 * n3 + 4 * int(full[L]) == 4 * int(g['count'][L])
        yy, xx = np.nonzero(mask)
        assert abs(s['var_y'][L] - yy.var()) < 1e-10 and abs(s['var_x'][L] - xx.var()) < 1e-10
        assert abs(s['cov'][L] - ((yy - yy.mean()) * (xx - xx.mean())).mean()) < 1e-10


# ------------------------------------------------------------------ hand cases
def test_one_pixel():
    mask = np.zeros((5, 6), bool)
    mask[2, 3] = True
    g, s = one_region(mask)
    assert g['quads'].tolist() == [4, 0, 0, 0] and g['count'] == 1 and g['border'] == 0
    assert (g['sy'], g['sx'], g['syy'], g['sxy'], g['sxx']) == (2, 3, 4, 6, 9)
    assert g['extents'].tolist() == [[3, 3], [8, 8], [5, 5], [7, 7], [2, 2], [1, 1], [-1, -1], [-4, -4]]
    assert s['perimeter_crack'] == 4 and s['euler4'] == 1 and s['euler8'] == 1
    assert s['widths'][0] == 1.0 and s['widths'][4] == 1.0           # the axis directions: a pixel is one wide
    assert s['widths'][2] == 2 / math.sqrt(2) and s['widths'][1] == 3 / math.sqrt(5)
    assert s['bbox'].tolist() == [2, 3, 3, 4] and s['bbox_fill'] == 1.0 and s['polygon_area'] == 1.0 and s['convexity16'] == 1.0
    assert s['major_axis'] == 0 and s['minor_axis'] == 0 and s['eccentricity'] == 0 and s['orientation'] == 0
    assert s['perimeter'] == 4 / math.sqrt(2)
    assert (s['centroid_y'], s['centroid_x']) == (2.0, 3.0)


def test_two_by_two_square():
    mask = np.zeros((4, 4), bool)
    mask[1:3, 1:3] = True
    g, s = one_region(mask)
    assert g['quads'].tolist() == [4, 4, 0, 0] and ref.n4({k: v[None] for k, v in g.items()})[0] == 1
    assert s['perimeter_crack'] == 8 and s['euler4'] == 1 and s['euler8'] == 1
    assert s['var_y'] == 0.25 and s['var_x'] == 0.25 and s['cov'] == 0
    assert s['major_axis'] == 2.0 and s['minor_axis'] == 2.0 and s['eccentricity'] == 0 and s['orientation'] == 0      # isotropic: exact
    assert s['perimeter'] == 4 + 4 / math.sqrt(2) and s['polygon_area'] == 4.0 and s['bbox_fill'] == 1.0
    assert s['feret_min'] == 2.0 and s['feret_max'] == 4 / math.sqrt(2)
    assert (s['centroid_y'], s['centroid_x']) == (1.5, 1.5)


def test_l_tromino():
    mask = np.zeros((4, 4), bool)
    mask[1, 1] = mask[2, 1] = mask[2, 2] = True
    g, s = one_region(mask)
    # corners of the L: five convex ones (n1) and the concave one (n3); two straight edge pieces (n2)
    assert g['quads'].tolist() == [5, 2, 0, 1]
    assert s['perimeter_crack'] == 8 and s['euler4'] == 1 and s['euler8'] == 1
    assert s['bbox'].tolist() == [1, 1, 3, 3] and s['bbox_fill'] == 0.75
    assert s['polygon_area'] == 3.5 and s['convexity16'] == 3 / 3.5   # the hull of an L-tromino: the square minus half a pixel


def test_two_pixels_on_a_diagonal():
    mask = np.zeros((4, 4), bool)
    mask[1, 1] = mask[2, 2] = True
    g, s = one_region(mask)
    assert g['quads'].tolist() == [6, 0, 1, 0]
    assert s['euler4'] == 2 and s['euler8'] == 1 and s['perimeter_crack'] == 8
    assert s['var_y'] == 0.25 and s['var_x'] == 0.25 and s['cov'] == 0.25
    assert s['orientation'] == math.pi / 4 and s['eccentricity'] == 1.0 and s['minor_axis'] == 0
    mask = mask[:, ::-1]
    g, s = one_region(mask)
    assert g['quads'].tolist() == [6, 0, 1, 0] and s['orientation'] == -math.pi / 4


def test_three_by_three_ring():
    mask = np.ones((3, 3), bool)
    mask[1, 1] = False
    g, s = one_region(np.pad(mask, 1))
    assert g['quads'].tolist() == [4, 8, 0, 4]                       # 4 + 2 * 8 + 3 * 4 = 32 = 4 * 8 pixels: no quad lies inside
    assert s['euler4'] == 0 and s['euler8'] == 0 and s['perimeter_crack'] == 16
    assert ref.features(ref.shape(ref.geometry(np.pad(mask, 1).astype(np.int32), 1)))[1, ref.FEATURES.index('holes')] == 1
    assert s['bbox_fill'] == 8 / 9 and s['polygon_area'] == 9.0 and s['eccentricity'] == 0 and s['orientation'] == 0


def test_bars():
    mask = np.zeros((5, 9), bool)
    mask[2, 1:8] = True                                              # 1 x 7, horizontal
    g, s = one_region(mask)
    assert g['quads'].tolist() == [4, 12, 0, 0]
    assert s['var_y'] == 0 and s['var_x'] == 4.0 and s['cov'] == 0       # (7^2 - 1) / 12
    assert s['orientation'] == 0 and s['eccentricity'] == 1.0 and s['major_axis'] == 8.0 and s['minor_axis'] == 0
    assert s['feret_min'] == 1.0 and s['feret_max'] == 7.0 and abs(s['widths'][1] - 15 / math.sqrt(5)) < 1e-15      # (2, 1): 2 * 6 + 3
    mask2 = np.zeros((5, 9), bool)
    mask2[1:4, 1:8] = True                                           # 3 x 7: eccentricity from arithmetic
    g, s = one_region(mask2)
    assert s['var_y'] == 8 / 12 and s['var_x'] == 4.0
    assert abs(s['eccentricity'] - math.sqrt(1 - (8 / 12) / 4.0)) < 1e-15 and s['orientation'] == 0
    g, s = one_region(mask2.T)                                       # the same bar transposed
    assert s['orientation'] == math.pi / 2 and abs(s['eccentricity'] - math.sqrt(1 - (8 / 12) / 4.0)) < 1e-15
    g, s = one_region(mask.T)
    assert s['orientation'] == math.pi / 2 and s['var_x'] == 0 and s['var_y'] == 4.0


def test_region_on_the_frame():
    labels = np.zeros((4, 5), np.int32)
    labels[0, :3] = 1                                                # three pixels of the top row, one of them the corner
    labels[1, 0] = 1
    labels[2, 2] = 2                                                 # interior
    labels[3, 4] = 3                                                 # the opposite corner
    g = ref.geometry(labels, 3)
    assert g['border'].tolist() == [9, 4, 0, 1]                       # 14 pixels on the frame of a 4 x 5 image
    assert g['quads'][3].tolist() == [4, 0, 0, 0]                    # the frame belongs to nobody: a corner pixel still has four corners
    s = ref.shape(g)
    assert ref.features(s)[:, ref.FEATURES.index('touches_border')].tolist() == [1, 1, 0, 1]
    out = ref.clear_border(labels)
    assert out.tolist() == [[0] * 5, [0] * 5, [0, 0, 2, 0, 0], [0] * 5]
    whole = ref.geometry(np.ones((4, 5), np.int32), 1)
    assert whole['quads'][1].tolist() == [4, 2 * 3 + 2 * 4, 0, 0] and whole['border'][1] == 2 * 4 + 2 * 5 - 4


# ------------------------------------------------------------------ the 16-gon contains the hull
@pytest.mark.parametrize('seed', range(12))
def test_polygon_contains_the_convex_hull(seed):
    rng = np.random.RandomState(200 + seed)
    a, b, phi = rng.uniform(3, 14), rng.uniform(3, 14), rng.uniform(0, math.pi)
    r = int(max(a, b)) + 2
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    u, v = xx * math.cos(phi) + yy * math.sin(phi), -xx * math.sin(phi) + yy * math.cos(phi)
    mask = (u / a) ** 2 + (v / b) ** 2 <= 1.0
    g, s = one_region(mask)
    ys, xs = np.nonzero(mask)
    corners = np.concatenate([np.stack([xs + dx, ys + dy], 1) for dx in (-0.5, 0.5) for dy in (-0.5, 0.5)])
    hull = ConvexHull(corners).volume                                # the area, in two dimensions
    assert s['polygon_area'] >= hull - 1e-9
    assert s['polygon_area'] <= s['bbox_fill'] ** -1 * s['area'] + 1e-9      # and lies inside the bounding box
    assert s['convexity16'] <= s['area'] / hull + 1e-12
    assert s['feret_max'] <= math.hypot(*(corners.max(0) - corners.min(0))) + 1e-9


def test_float64_against_longdouble_on_random_regions():
    """The float64 evaluation against the same formulas in numpy.longdouble: on small regions every product of the moments is exact,
    so the columns agree to a few float64 roundings."""
    rng = np.random.RandomState(7)
    labels = rng.randint(0, 6, (24, 31)).astype(np.int32)
    g = ref.geometry(labels, 5)
    s, w = ref.shape(g), ref.shape(g, np.longdouble)
    assert s['exact']
    for k in ref.SHAPE_FLOATS:
        if k == 'minor_axis':
            assert (np.abs(s[k] - w[k]) <= 2.0 ** -24 * w['major_axis'] + 2.0 ** -50 * np.abs(w[k])).all()
        else:
            assert (np.abs(s[k] - w[k]) <= 2.0 ** -48 * np.abs(w[k])).all(), k
