"""CPU: tests/hull_ref.py, the restatement the GPU hull is held to, pinned against independent computations: Qhull
(scipy.spatial.ConvexHull) over the same corners for the vertex set and the area, and scans over ALL corners -- not only the hull's
vertices -- for the diameter and the width.

The area bound.  Qhull sums, over the k facets (edges) of the hull, facet length x distance from an interior point to the facet's line
/ 2.  With coordinates of at most C every length and distance is at most sqrt(2) C, so a facet's term is at most C^2; it comes out of
a normalised normal, an offset and a few products -- fewer than 16 float64 roundings of relative size 2^-53 each -- and the sum adds
at most k roundings of the running total, itself at most k C^2.  |volume - area2 / 2| <= (16 + k) k C^2 2^-53.  For the cases here (k <=
64, C <= 48) that is below 2^-30: far under 1/4, and area2 / 2 is a multiple of 1/2, so the comparison pins area2 itself."""
import math
from fractions import Fraction

import numpy as np
import pytest

import hull_ref as ref


def disc(r):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return yy * yy + xx * xx <= r * r


HAND = [np.ones((1, 1), bool), np.ones((1, 9), bool), np.ones((9, 1), bool), np.ones((3, 5), bool), np.eye(7, dtype=bool),
        np.eye(7, dtype=bool)[::-1], disc(7), disc(6) & ~np.pad(disc(3), 3),
        np.array([[1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [1, 1, 1, 1]], bool),
        np.array([[1, 1, 1, 1], [1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [1, 1, 1, 1]], bool)]


def blobs():
    rng = np.random.RandomState(23)
    out = list(HAND)
    for i in range(100):
        H, W = rng.randint(1, 25, 2)
        m = rng.rand(H, W) < (0.08, 0.4, 0.85)[i % 3]
        if not m.any():
            m[rng.randint(H), rng.randint(W)] = True
        out.append(m)
    return out


BLOBS = blobs()


def test_hand_values():
    t, v = ref.hull_of_mask(np.ones((1, 1), bool))
    assert v == [(0, 0), (1, 0), (1, 1), (0, 1)]
    assert t == dict(count=4, area2=2, diameter2=2, diameter_ends=((0, 0), (1, 1)), width_cross=1, width_edge=(1, 0), perimeter=4.0)
    t, v = ref.hull_of_mask(np.ones((3, 5), bool))
    assert v == [(0, 0), (3, 0), (3, 5), (0, 5)]
    assert (t['area2'], t['diameter2'], t['diameter_ends'], t['width_cross'], t['width_edge']) == (30, 34, ((0, 0), (3, 5)), 15, (0, 5))
    assert t['perimeter'] == 16.0
    t, v = ref.hull_of_mask(np.eye(3, dtype=bool))                      # the staircase: corners on the two long edges are dropped
    assert v == [(0, 0), (1, 0), (3, 2), (3, 3), (2, 3), (0, 1)]
    assert t['area2'] == 2 * 3 + 4 and t['diameter2'] == 18 and t['diameter_ends'] == ((0, 0), (3, 3))
    assert (t['width_cross'], t['width_edge']) == (4, (2, 2))            # across the band: 4 / sqrt(8)
    assert ref.hull_of_mask(np.zeros((3, 3), bool)) is None


def test_order_and_strict_convexity():
    for m in BLOBS:
        _, v = ref.hull_of_mask(m)
        k = len(v)
        assert len(set(v)) == k >= 4
        assert v[0] == min(v)                                            # (y, x): the top line's left end
        assert v[1][0] > v[0][0] and v[-1][0] == v[0][0]                 # down the left side first; the top line's right end last
        for i in range(k):
            (ay, ax), (by, bx), (cy, cx) = v[i - 1], v[i], v[(i + 1) % k]
            assert (bx - ax) * (cy - by) - (by - ay) * (cx - bx) < 0     # a strict turn, always the same way


def test_against_qhull():
    scipy_spatial = pytest.importorskip('scipy.spatial')
    for m in BLOBS:
        pts = np.array(sorted(ref.corners(m)), np.float64)
        t, v = ref.hull_of_mask(m)
        hull = scipy_spatial.ConvexHull(pts)
        assert set((int(y), int(x)) for x, y in pts[hull.vertices]) == set(v)
        k, C = t['count'], float(pts.max())
        bound = (16 + k) * k * C * C * 2.0 ** -53
        assert k <= 64 and C <= 48 and bound < 2.0 ** -30
        assert abs(hull.volume - t['area2'] / 2.0) <= bound
        assert abs(hull.area - t['perimeter']) <= 64 * k * 2.0 ** -53 * t['perimeter']      # Qhull's facet lengths: a loose cross-check


def test_against_scans_over_all_corners():
    for n, m in enumerate(BLOBS):
        pts = sorted(ref.corners(m))
        t, v = ref.hull_of_mask(m)
        a = np.array(pts, np.int64)
        d2 = ((a[:, None, :] - a[None, :, :]) ** 2).sum(2)
        assert int(d2.max()) == t['diameter2']
        (y0, x0), (y1, x1) = t['diameter_ends']
        assert (y0 - y1) ** 2 + (x0 - x1) ** 2 == t['diameter2'] and (y0, x0) in v and (y1, x1) in v and v.index((y0, x0)) < v.index((y1, x1))
        # the width over every direction spanned by two corners: none is narrower than the reported edge (the minimum is attained at
        # a hull edge), compared as rationals
        dy, dx = t['width_edge']
        mine = Fraction(t['width_cross'] ** 2, dy * dy + dx * dx)
        k = len(v)
        assert any((v[(i + 1) % k][0] - v[i][0], v[(i + 1) % k][1] - v[i][1]) == (dy, dx) for i in range(k))
        proj = a[:, 0] * dy - a[:, 1] * dx                               # dy x - dx y
        assert int(proj.max() - proj.min()) == t['width_cross']
        dirs = set()
        if n % 4:                                                        # the scan over directions: every fourth case
            continue
        for i in range(0, len(pts), max(1, len(pts) // 40)):
            for j in range(len(pts)):
                ex, ey = pts[j][0] - pts[i][0], pts[j][1] - pts[i][1]
                g = math.gcd(ex, ey)
                if g:
                    dirs.add((ex // g, ey // g))
        for ex, ey in dirs:
            p = a[:, 0] * ey - a[:, 1] * ex
            assert Fraction(int(p.max() - p.min()) ** 2, ex * ex + ey * ey) >= mine


def test_tables_and_within():
    lab = np.zeros((9, 10), np.int32)
    lab[1:4, 2:7] = 2
    lab[6, 1] = 4
    t = ref.tables(lab, 5)
    assert t['count'].tolist() == [4, 0, 4, 0, 4, 0] and t['ptr'].tolist() == [0, 4, 4, 8, 8, 12, 12]
    assert t['vertices'][4:8].tolist() == [[1, 2], [4, 2], [4, 7], [1, 7]] and t['area2'][0] == 180
    within = np.ones(lab.shape, bool)
    within[1] = False
    w = ref.tables(lab, 5, within)
    assert w['vertices'][w['ptr'][2]:w['ptr'][3]].tolist() == [[2, 2], [4, 2], [4, 7], [2, 7]]
    s = ref.shape(t, np.bincount(lab.ravel(), minlength=6))
    assert s['solidity'][2] == 1.0 and s['convex_area'][2] == 15.0 and s['feret_min'][2] == 3.0 and s['solidity'][1] == 0.0
    assert ref.features(s).shape == (6, len(ref.FEATURES))
