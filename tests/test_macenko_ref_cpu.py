"""CPU: the contract of stain estimation (kernels.KernelSpec.od_moments / angle_histogram, nuclei.estimate_stains) as restated in
tests/macenko_ref.py, pinned from the other side: the direction table to the angles it stands for, the integer cross-product count to
atan2, the intermediate bounds at their extremes, the percentile rule to a brute-force sort, and the integer rule to a float64
Macenko within the bound DESIGN.md ("Stain estimation") derives."""
import math
from fractions import Fraction

import numpy as np
import pytest

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, nuclei

import macenko_ref as ref

K = ref.K


def test_direction_table_is_stable_and_increasing():
    """No entry within 1e-6 of a rounding boundary (every libm builds the same table), the package's table is the restated one, and
    the rounded directions lie in the open right half plane with strictly increasing angles -- exactly, by integer cross products."""
    margin = 1.0
    for t in ref.angle_thetas():
        for v in (16384.0 * math.cos(t), 16384.0 * math.sin(t)):
            margin = min(margin, abs(abs(v - math.floor(v)) - 0.5))
    assert margin > 1e-6
    assert 3.5e-4 < margin < 4.5e-4                                              # the nearest boundary: 4.0e-4 away
    d = ref.angle_dirs()
    assert nuclei.ANGLE_DIRS == tuple((int(c), int(s)) for c, s in d) and len(nuclei.ANGLE_DIRS) == K - 1 == kernels.ANGLE_BINS - 1
    assert (d[:, 0] > 0).all() and np.abs(d).max() <= ref.DIR_MAX
    assert (d[:-1, 0] * d[1:, 1] - d[:-1, 1] * d[1:, 0] > 0).all()
    kernels.HipKernels._check_angle_tables([[4096, 0, 0], [0, 4096, 0]], nuclei.ANGLE_DIRS)      # the refusal accepts it
    assert ref.table_rounding() < 0.5 * math.sqrt(2.0) / 16384 / 0.999              # half a diagonal of the integer grid, seen from 16384


def test_prefix_property_and_count_against_atan2():
    """For p_1 > 0 the directions with c_k p_2 - s_k p_1 >= 0 are a prefix of 1..K-1, so a binary search finds the count; and the
    count is the bin of atan2 wherever the angle is farther from a boundary than the table's own rounding of it."""
    rng = np.random.RandomState(5)
    p = rng.randint(-ref.P_MAX, ref.P_MAX + 1, (20000, 2)).astype(np.int64)
    p[:, 0] = np.abs(p[:, 0]) + (p[:, 0] == 0)
    p[:200, 0] = rng.randint(1, 4, 200)                                          # steep: next to +-pi/2
    p[200:400, 1] = rng.randint(-3, 4, 200)                                      # flat: next to 0
    p[400:404] = [[ref.P_MAX, ref.P_MAX], [ref.P_MAX, -ref.P_MAX], [1, ref.P_MAX], [1, -ref.P_MAX]]
    d = ref.angle_dirs()
    cross = p[:, 1:2] * d[None, :, 0] - p[:, 0:1] * d[None, :, 1]
    assert np.abs(cross).max() <= 16384 * 2 * ref.P_MAX < 2 ** 31
    ge = cross >= 0
    count = ge.sum(axis=1)
    assert (ge[:, :-1] >= ge[:, 1:]).all()                                       # a prefix: never False before True
    assert np.array_equal(count, ref.count_bins(p, d))
    lo = np.zeros(len(p), np.int64)                                              # the 10-step search over entries 1..K-1
    half = K // 2
    while half >= 1:
        k = lo + half
        lo = np.where(d[k - 1, 0] * p[:, 1] - d[k - 1, 1] * p[:, 0] >= 0, k, lo)
        half //= 2
    assert np.array_equal(lo, count)
    width = ref.table_rounding()
    phi = np.arctan2(p[:, 1].astype(np.float64), p[:, 0].astype(np.float64))
    scaled = (phi + 0.5 * math.pi) * K / math.pi
    clear = np.abs(scaled - np.rint(scaled)) * math.pi / K > width + 1e-12
    assert clear.mean() > 0.9
    assert np.array_equal(count[clear], np.floor(scaled[clear]).astype(np.int64))
    assert 0 <= count.min() and count.max() <= K - 1


def test_pixels_on_a_boundary_count_it():
    """p = a table direction itself (scaled down to the range of p): the cross product is zero, '>=' holds, the bin is k."""
    d = ref.angle_dirs()
    for k in (1, 2, 255, 511, 512, 513, 700, 1022, 1023):
        c, s = d[k - 1]
        p = np.array([[c // 2, s // 2]], np.int64) if (c % 2 == 0 and s % 2 == 0) else None
        if p is not None:
            assert ref.count_bins(p, d)[0] == k
    c, s = d[512 - 1]
    assert (c, s) == (16384, 0) and ref.count_bins(np.array([[5, 0], [9829, -1], [9829, 1]], np.int64), d).tolist() == [512, 511, 512]


def test_intermediate_bounds_at_their_extremes():
    assert ref.OD_MAX == kernels.STAIN_OD_MAX == max(nuclei.OD_LUT) and tuple(ref.od_lut()) == nuclei.OD_LUT
    assert ref.E_REACH == math.ceil(4096 * math.sqrt(3)) == kernels.ANGLE_E_REACH and ref.E_MAX == kernels.ANGLE_E_MAX
    assert ref.OD_MAX * ref.E_REACH < 2 ** 26
    assert (ref.OD_MAX * ref.E_REACH + 2 ** 11) >> 12 == 9828 <= ref.P_MAX == 9829      # the extremes stay inside the stated bound
    assert (-ref.OD_MAX * ref.E_REACH + 2 ** 11) >> 12 == -9828
    assert ref.DIR_MAX * 2 * ref.P_MAX < 2 ** 31 and ref.DIR_MAX == kernels.ANGLE_DIR_MAX
    assert ref.OD_MAX ** 2 * (2 ** 31 - 1) < 2 ** 63
    assert 64 * ref.OD_MAX ** 2 < 2 ** 32 < 67 * 2 * ref.OD_MAX ** 2          # a lane's 64 pixels fit uint32; int32 ends near 67
    o = np.full((1, 3), ref.OD_MAX, np.int64)
    assert ref.project(o, [[2365, 2365, 2365], [-2365, -2365, -2365]]).tolist() == [[9828, -9828]]
    for e in np.random.RandomState(1).randn(200, 3):                             # rint(4096 unit vector) obeys the basis bound
        q = np.rint(4096.0 * e / np.linalg.norm(e)).astype(np.int64)
        assert np.abs(q).max() <= ref.E_MAX and np.abs(q).sum() <= ref.E_REACH
    assert ref.od_min_of(0.15) == 154 and ref.od_min_of(0) == 0 and ref.od_min_of(Fraction(154, 1024)) == 154
    assert nuclei._od_min(0.15) == 154 and nuclei._od_min(0.0) == 0 and nuclei._od_min(5674 / 1024) == 5674
    flat = np.zeros((200, 160, 3), np.uint8)                                     # the largest sums of products of the GPU tests
    mom = ref.od_moments(flat, 0, ref.od_lut(), 0)
    assert mom[0] == 32000 and mom[4] == 32000 * ref.OD_MAX ** 2 > 2 ** 39


@pytest.mark.parametrize('alpha', [0, 0.5, 1.0, 1, 2.5, 10, 49.9, Fraction(1, 3)])
def test_percentile_rule_against_a_sort(alpha):
    rng = np.random.RandomState(3)
    cases = [rng.randint(0, 5, K), np.where(rng.rand(K) < 0.02, rng.randint(1, 1000, K), 0), np.eye(K, dtype=np.int64)[17] * 7,
             np.eye(K, dtype=np.int64)[0] + np.eye(K, dtype=np.int64)[K - 1], np.ones(K, np.int64) * 100]
    a = Fraction(alpha)
    for bins in cases:
        bins = [int(c) for c in bins]
        M = sum(bins)
        order = [b for b, c in enumerate(bins) for _ in range(c)]                # the bin index of every pixel, sorted
        want = (order[max(math.ceil(a * M / 100), 1) - 1], order[math.ceil((100 - a) * M / 100) - 1])
        assert ref.percentile_bins(bins, alpha) == want
        assert nuclei._percentile_bins(bins, alpha) == want
        assert want[0] <= want[1]


@pytest.mark.parametrize('pair', [0, 1])
@pytest.mark.parametrize('shape', ref.TILE_SHAPES)
def test_integer_rule_within_the_derived_bound_of_float64(shape, pair):
    """Both rules on a rendered tile: they select the same pixels, nothing is skipped, and each vector of the integer rule lies
    within the derived bound B = 2 tau + asin(kappa sin tau) + gamma + delta + pi / 2K + rho of the float64 rule's.
    Measured gap (haematoxylin, eosin) / bound, degrees, per pair and shape:
        pair 0: 0.021, 0.045 / 0.88;  0.003, 0.059 / 0.76;  0.044, 0.042 / 0.82
        pair 1: 0.059, 0.027 / 0.42;  0.063, 0.077 / 0.40;  0.065, 0.054 / 0.42"""
    tile, S, info, z, F = ref.rendered_case(shape, pair)
    assert info['skipped'] == 0 and info['od_min'] == 154 and info['n'] > 0.5 * shape[0] * shape[1]
    bound, terms = ref.derived_bound(tile)
    gaps = [ref.angle_deg(S[s], F[s]) for s in range(3)]
    print('gaps', gaps, 'bound', bound, terms)
    assert bound < 1.0                                                           # a bound worth the name: under a degree on these tiles
    assert gaps[0] <= bound and gaps[1] <= bound
    assert gaps[2] <= 2 * bound / math.sin(math.radians(ref.angle_deg(F[0], F[1])))      # the cross product of two such vectors
    assert np.allclose((S * S).sum(axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize('pair', [0, 1])
def test_recovery_of_known_stains(pair):
    """A tile rendered from two known vectors (30 % background, 10 % pure in each stain, unit noise).  The float64 reference recovers
    haematoxylin to 0.49-0.65 degrees and eosin to 0.08-0.31 degrees (alpha = 1 leaves it a little inside the pure pixels); asserted
    at 1 degree, and the integer rule at that plus its derived distance from the reference."""
    for shape in ref.TILE_SHAPES:
        tile, S, info, z, F = ref.rendered_case(shape, pair)
        bound, _ = ref.derived_bound(tile)
        for s, true in enumerate(ref.true_stains(pair)):
            off = ref.angle_deg(F[s], true)
            print(pair, shape, s, off, ref.angle_deg(S[s], true))
            assert off < 1.0
            assert ref.angle_deg(S[s], true) <= off + bound
        m = nuclei.stain_matrix(S)                                               # ready for separate_stains
        assert m.shape == (3, 3)
