"""CPU: the contract of stain normalisation (kernels.KernelSpec.concentration_histogram / od_recolor, nuclei.stain_maxima,
recolor_matrix, normalize_stains) as restated in tests/normalize_ref.py, pinned from the other side: the exponential table to the
function it stands for and to the optical-density table it inverts, the percentile rule to a brute-force rank, the dropped residual to
least squares, the int32 bounds at their extremes, and the integer rules to the float64 formulas within the bounds DESIGN.md ("Stain
normalisation") derives."""
import math
from fractions import Fraction

import numpy as np
import pytest

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, nuclei

import macenko_ref
import normalize_ref as ref

IDENTITY = [[4096, 0, 0], [0, 4096, 0], [0, 0, 4096]]


def random_pixels(n, seed):
    """uint8 [1, n, 3], uniform random bytes with the extremes 0, 1, 254, 255 over-represented."""
    rng = np.random.RandomState(seed)
    pix = rng.randint(0, 256, (1, n, 3)).astype(np.uint8)
    extreme = rng.rand(*pix.shape) < 0.1
    pix[extreme] = rng.choice(np.array([0, 1, 254, 255], np.uint8), size=int(extreme.sum()))
    return pix


# ------------------------------------------------------------------ the exponential table
def test_exp_lut_is_stable_and_the_package_holds_it():
    table = ref.exp_lut()
    assert nuclei.EXP_LUT == tuple(int(v) for v in table) and all(type(v) is int for v in nuclei.EXP_LUT)
    assert len(table) == 6386 == kernels.EXP_LUT_LEN == ref.EXP_LEN
    assert table[0] == 255 and table[-1] == 0 and (table[:-1] > 0).all()         # 0 only last
    assert (np.diff(table) <= 0).all()
    kernels.HipKernels._check_exp_lut(nuclei.EXP_LUT)                            # the refusal accepts it
    margin, at = min((abs(v - round(v)), k) for k, v in ((k, 255.0 * math.exp(-k / 1024.0) + 0.5) for k in range(6386)))
    assert margin > 1e-6                                                         # every libm builds the same table
    assert at == 6384 and 1.7e-5 < margin < 1.9e-5                               # the nearest integer: 1.79e-5 away


def test_exp_lut_inverts_the_od_table():
    lut, table = ref.od_lut(), ref.exp_lut()
    assert tuple(int(v) for v in lut) == nuclei.OD_LUT
    assert [int(table[lut[v]]) for v in range(1, 256)] == list(range(1, 256))
    assert table[lut[0]] == 1 and lut[0] == lut[1] == ref.OD_MAX


@pytest.mark.parametrize('order', [0, 1])
def test_identity_matrix_is_the_identity_except_zero(order):
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    for pix in (grey, random_pixels(5000, 3)):
        out = ref.od_recolor(pix, order, ref.od_lut(), IDENTITY, ref.exp_lut())
        assert out.dtype == np.uint8 and out.shape == pix.shape
        assert np.array_equal(out, np.maximum(pix, 1))
    assert (random_pixels(5000, 3) == 0).any()


def test_channel_orders_agree():
    pix = random_pixels(3000, 4)
    a = ref.recolor_matrix(ref.DEFAULT_STAINS, (1.5, 0.9))
    assert np.array_equal(ref.od_recolor(pix, 0, ref.od_lut(), a, ref.exp_lut())[..., ::-1],
                          ref.od_recolor(pix[..., ::-1], 1, ref.od_lut(), a, ref.exp_lut()))
    m = ref.stain_matrix()
    assert np.array_equal(ref.concentration_histogram(pix, 0, ref.od_lut(), 154, m),
                          ref.concentration_histogram(pix[..., ::-1], 1, ref.od_lut(), 154, m))


# ------------------------------------------------------------------ the percentile rule
def brute_force_bin(values, alpha):
    """The bin of the ceil((100 - alpha) n / 100)-th smallest value (the first for a rank below one)."""
    v = sorted(values)
    rank = max(math.ceil((100 - Fraction(alpha)) * len(v) / 100), 1)
    return v[rank - 1]


def test_percentile_rule_against_a_sorted_rank():
    rng = np.random.RandomState(8)
    cases = [rng.randint(0, 512, n).tolist() for n in (1, 2, 3, 99, 100, 101, 1000)]
    cases += [rng.randint(200, 204, 777).tolist(), [300] * 50, [0] * 7 + [511] * 3, [5] * 99 + [400], [5] * 100 + [400]]      # ties
    for values in cases:
        bins = np.bincount(values, minlength=512).tolist()
        for alpha in (0, 0.5, 1, 1.0, Fraction(1, 3), 5, 25, 49.999):
            want = brute_force_bin(values, alpha)
            assert ref.top_bin(bins, alpha) == want == nuclei._top_bin(bins, alpha), (len(values), alpha)
        assert ref.top_bin(bins, 0) == max(values)                               # alpha = 0: the maximum
    assert ref.top_bin([0, 0, 9, 0], 1) == 2 == nuclei._top_bin([0, 0, 9, 0], 1)  # all pixels in one bin
    assert ref.top_bin(np.bincount([5] * 99 + [400], minlength=512), 1) == 5      # 99 of 100 reach 99 %
    assert ref.top_bin(np.bincount([5] * 99 + [400] * 2, minlength=512), 1) == 400      # 99 of 101 do not


# ------------------------------------------------------------------ the matrix
@pytest.mark.parametrize('pair', [0, 1])
@pytest.mark.parametrize('shape', macenko_ref.TILE_SHAPES)
def test_dropping_the_residual_is_least_squares(shape, pair):
    """The residual row of estimate_stains is orthogonal to the other two, so the first two columns of inv(S) are the least-squares
    solution on the two stains alone."""
    S = macenko_ref.rendered_case(shape, pair)[1]
    assert abs(S[2] @ S[0]) < 1e-12 and abs(S[2] @ S[1]) < 1e-12
    od = macenko_ref.float_od(macenko_ref.rendered_tile(shape, pair), 0)
    C = np.linalg.lstsq(S[:2].T, od.T, rcond=None)[0]
    assert np.abs(np.linalg.inv(S)[:, :2].T @ od.T - C).max() < 1e-12 * max(1.0, np.abs(C).max()) * 100
    assert np.abs(np.linalg.inv(S)[:, :2] - np.linalg.pinv(S[:2])).max() < 1e-12


def test_recolor_matrix_is_the_restated_composition():
    for pair in (0, 1):
        S = macenko_ref.rendered_case((96, 80), pair)[1]
        for maxima, kw in (((Fraction(310, 128), Fraction(313, 128)), {}), ((1.5, 0.9), dict(target_max=(1.0, 2.0))),
                           ((2.0, 1.0), dict(target_stains=ref.DEFAULT_STAINS)), ((2.0, 1.0), dict(target_stains=ref.DEFAULT_STAINS[:2]))):
            a = nuclei.recolor_matrix(S, maxima, **kw)
            assert a.dtype == np.int32 and a.shape == (3, 3)
            assert np.array_equal(a, ref.recolor_matrix(S, maxima, **kw))
    assert nuclei.TARGET_STAINS == ref.TARGET_STAINS == macenko_ref.STAIN_PAIRS[0] and nuclei.TARGET_MAX == ref.TARGET_MAX == (1.9705, 1.0308)
    # a tile's own stains at their own strength map onto themselves: A = inv(S)[:, :2] S[:2] projects onto the stain plane
    S = macenko_ref.rendered_case((96, 80), 0)[1]
    A = ref.recolor_matrix_float(S, (1.0, 1.0), S, (1.0, 1.0))
    assert np.abs(S[:2] @ A - S[:2]).max() < 1e-12 and np.abs(S[2] @ A).max() < 1e-12


def test_int32_bounds_at_the_extremes():
    """The largest sums the two refusals admit, with their rounding terms, stay inside int32, and every factor fits the 24-bit
    multiplier the kernels use."""
    for slack, half in ((2 ** 15, 2 ** 14), (2 ** 11, 2 ** 11)):                  # concentration_histogram, od_recolor
        reach = (2 ** 31 - slack - 1) // ref.OD_MAX                               # the largest admitted sum_c |m[c][s]|
        assert reach * ref.OD_MAX < 2 ** 31 - slack <= (reach + 1) * ref.OD_MAX
        assert reach * ref.OD_MAX + half <= 2 ** 31 - 1 and -reach * ref.OD_MAX + half >= -2 ** 31
        assert reach < 2 ** 23 and ref.OD_MAX < 2 ** 23
        black = np.zeros((1, 1, 3), np.uint8)
        for sign in (1, -1):
            col = [sign * reach, 0, 0]
            mat = [[col[0], 0, 0], [0, 1, 0], [0, 0, 1]]
            if slack == 2 ** 15:
                hist = ref.concentration_histogram(black, 1, ref.od_lut(), 0, mat)
                assert hist[511 if sign > 0 else 0] == 1
                kernels.HipKernels._check_od_matrix('concentration_histogram', mat, slack)
                with pytest.raises(ValueError):
                    kernels.HipKernels._check_od_matrix('concentration_histogram', [[col[0] + sign, 0, 0], [0, 1, 0], [0, 0, 1]], slack)
            else:
                out = ref.od_recolor(black, 1, ref.od_lut(), mat, ref.exp_lut())
                assert out[0, 0, 0] == (0 if sign > 0 else 255)
                kernels.HipKernels._check_od_matrix('od_recolor', mat, slack)
                with pytest.raises(ValueError):
                    kernels.HipKernels._check_od_matrix('od_recolor', [[col[0] + sign, 0, 0], [0, 1, 0], [0, 0, 1]], slack)


# ------------------------------------------------------------------ the integer rules against float64
def matrices():
    S = macenko_ref.rendered_case((96, 80), 1)[1]
    inv = np.linalg.inv(S)
    T = ref.unit_rows(ref.TARGET_STAINS)
    return {'identity': np.eye(3), 'normalise': ref.recolor_matrix_float(S, (2.4, 2.5)), 'haematoxylin alone': np.outer(inv[:, 0], T[0]),
            'eosin alone': np.outer(inv[:, 1], T[1]), 'darker': 3.0 * np.eye(3), 'negative': -0.5 * np.eye(3),
            'mixing': np.array([[0.9, -0.4, 0.2], [-0.3, 1.2, 0.1], [0.25, 0.5, -0.7]])}


@pytest.mark.parametrize('name', sorted(matrices()))
@pytest.mark.parametrize('order', [0, 1])
def test_recolor_rule_against_the_float_formula(name, order):
    """od_recolor with a = rint(4096 A) against 255 exp(-(ln(255 / max(v, 1)) A)_d) cut at 255: the bound of ref.recolor_bound,
    evaluated per pixel and channel."""
    A = matrices()[name]
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    pix = np.concatenate([grey, random_pixels(20000, 12), np.array(macenko_ref.rendered_tile((48, 64), 1, order)).reshape(1, -1, 3)], axis=1)
    a = np.rint(4096.0 * A).astype(np.int64)
    out = ref.od_recolor(pix, order, ref.od_lut(), a, ref.exp_lut())
    rgb = (out[..., ::-1] if order == 0 else out).reshape(-1, 3).astype(np.float64)
    gap = np.abs(rgb - np.minimum(ref.float_recolor(pix, order, A), 255.0))
    bound = ref.recolor_bound(pix, order, A)
    worst = int(np.argmax(gap - bound))
    print('%s, order %d: largest gap %.3f levels, bound there %.3f, smallest slack %.3f' % (
        name, order, gap.max(), bound.reshape(-1)[int(np.argmax(gap))], (bound - gap).min()))
    assert (gap <= bound).all(), (gap.reshape(-1)[worst], bound.reshape(-1)[worst])


@pytest.mark.parametrize('pair', [0, 1])
@pytest.mark.parametrize('shape', macenko_ref.TILE_SHAPES)
def test_integer_rule_against_the_float_normaliser(shape, pair):
    """normalize_stains' rule against Macenko's normalisation in float64 with the same stain vectors, on the six rendered tiles: the
    bound of ref.normalize_bound -- half a concentration bin, the rank against numpy's interpolated percentile, the recolour bound --
    evaluated per pixel and channel."""
    tile, S, out, info = ref.normalized_case(shape, pair)
    bound, F, terms = ref.normalize_bound(tile, S)
    rgb = out[..., ::-1].reshape(-1, 3).astype(np.float64)
    gap = np.abs(rgb - np.minimum(F, 255.0))
    for s in range(2):                                                           # the maxima themselves
        assert abs(float(info['maxima'][s]) - terms[s]['P']) <= terms[s]['mu']
    print('%s pair %d: bins %s, n %d, largest gap %.3f levels, bound there %.3f, largest bound %.3f, smallest slack %.3f, mu %s' % (
        shape, pair, info['bins'], info['n'], gap.max(), bound.reshape(-1)[int(np.argmax(gap))], bound.max(), (bound - gap).min(),
        ['%.4f' % t['mu'] for t in terms]))
    assert (gap <= bound).all()
    assert 0 < info['bins'][0] < 511 and 0 < info['bins'][1] < 511 and info['n'] > 1000
    assert out.shape == tile.shape and out.dtype == np.uint8


def test_stains_recovered_from_a_normalised_tile():
    """A tile rendered with stain pair 1, normalised by the integer rule (U) and by the float64 normaliser (V): the vectors that
    estimate_stains' rule recovers from U against TARGET_STAINS, held to what the float64 estimate recovers from V plus the derived
    bounds between the two -- the integer estimate against the float64 one on U (macenko_ref.derived_bound) and the float64 estimate
    on U against that on V (ref.estimate_shift_bound).  On this tile: 0.064 and 0.117 degrees for the integer rules, 0.075 and 0.037
    for the float64 ones, bounds 0.97 + 13.2 degrees -- the second is dominated by the Davis-Kahan tilt of two nearly planar clouds
    (2 tau = 7.8, kappa sin tau = 4.2, gamma = 1.2); the vectors themselves are 0.02 degrees apart."""
    tile, S, U, _ = ref.normalized_case((200, 160), 1)
    V = ref.float_normalized_tile(tile, S)
    assert np.abs(U.astype(np.int64) - V).max() <= np.floor(ref.normalize_bound(tile, S)[0] + 0.5).max()
    T = ref.unit_rows(ref.TARGET_STAINS)
    got, achieved = macenko_ref.estimate(U)[0], macenko_ref.float_macenko(V)[0]
    rules, rule_terms = macenko_ref.derived_bound(U)
    shift, shift_terms = ref.estimate_shift_bound(U, V)
    for s in range(2):
        mine, theirs = macenko_ref.angle_deg(got[s], T[s]), macenko_ref.angle_deg(achieved[s], T[s])
        print('stain %d: integer rules %.3f degrees from the target, float64 rules %.3f, bounds %.3f + %.3f' % (s, mine, theirs, rules, shift))
        assert mine <= theirs + rules + shift
    print({k: round(math.degrees(v), 3) for k, v in shift_terms.items() if k != 'flipped'}, 'flipped', shift_terms['flipped'])
