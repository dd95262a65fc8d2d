"""CPU: pins tests/window_ref.py, the numpy restatement that tests/test_window_gpu.py compares csrc/window.hip with -- by loops over
every window, by ``fractions.Fraction`` / Python-integer evaluation of v > m + k s + c, by closed forms and by the example that
motivates the local rule."""
import math
from fractions import Fraction

import numpy as np
import pytest

import window_ref as wr


def brute_sums(image, r, within=None):
    H, W = image.shape
    n, S, Q = (np.zeros((H, W), np.int64) for _ in range(3))
    for y in range(H):
        for x in range(W):
            for yy in range(max(y - r, 0), min(y + r, H - 1) + 1):
                for xx in range(max(x - r, 0), min(x + r, W - 1) + 1):
                    if within is None or within[yy, xx] != 0:
                        v = int(image[yy, xx])
                        n[y, x] += 1
                        S[y, x] += v
                        Q[y, x] += v * v
    return n, S, Q


@pytest.mark.parametrize('shape', [(1, 1), (1, 9), (7, 1), (5, 9), (12, 17)])
@pytest.mark.parametrize('r', [0, 1, 3, 40])
def test_sums_equal_loops_over_every_window(shape, r):
    rng = np.random.default_rng(shape[0] * 100 + shape[1] + r)
    image = rng.integers(0, 256, shape, dtype=np.uint8)
    within = rng.integers(-1, 2, shape).astype(np.int32)                # -1, 0, 1: only "is zero" is read
    for w in (None, within, np.zeros(shape, bool)):
        for got, want in zip(wr.window_sums(image, r, w), brute_sums(image, r, w)):
            assert got.dtype == np.int64 and (got == want).all()


def exact_rule(v, n, S, Q, k64, c, floor):
    """v > m + k s + c, v > floor, n >= 1 with m = S / n, s = sqrt(Q / n - m^2), k = k64 / 64 -- no square root taken: the sign of
    a - k s for rationals a and k and s^2 = var is decided from a, k and a^2 against k^2 var."""
    if n < 1 or v <= floor:
        return False
    m = Fraction(S, n)
    var = Fraction(Q, n) - m * m
    assert var >= 0
    a, k = v - m - c, Fraction(k64, 64)                                 # foreground iff a > k s
    if k >= 0:
        return a > 0 and a * a > k * k * var
    return a > 0 or (a == 0 and var > 0) or (a < 0 and a * a < k * k * var)


def test_rule_equals_fraction_evaluation_on_random_small_inputs():
    rng = np.random.default_rng(7)
    seen = set()
    for trial in range(60):
        H, W = int(rng.integers(1, 7)), int(rng.integers(1, 8))
        levels = rng.choice([2, 3, 256])                                # few levels: ties and constant windows do occur
        image = (rng.integers(0, levels, (H, W)) * (255 // (levels - 1))).astype(np.uint8)
        within = None if trial % 3 == 0 else rng.integers(0, 2, (H, W)).astype(np.uint8)
        r = int(rng.integers(0, 4))
        k64 = int(rng.choice([-128, -64, -13, -1, 0, 1, 13, 64, 128]))
        c = int(rng.choice([-255, -3, -1, 0, 1, 3, 255]))
        floor = int(rng.choice([-1, 0, 100, 255]))
        n, S, Q = wr.window_sums(image, r, within)
        got = wr.local_threshold(image, r, k64, c, floor, within)
        for y in range(H):
            for x in range(W):
                want = exact_rule(int(image[y, x]), int(n[y, x]), int(S[y, x]), int(Q[y, x]), k64, c, floor)
                assert bool(got[y, x]) == want, (trial, y, x)
                seen.add(want)
    assert seen == {True, False}


def test_rule_agrees_with_floating_point_away_from_ties():
    rng = np.random.default_rng(11)
    image = rng.integers(0, 256, (9, 11), dtype=np.uint8)
    n, S, Q = wr.window_sums(image, 2)
    m = S / n
    s = np.sqrt(np.maximum(Q / n - m * m, 0))
    for k64, c in ((13, 0), (-13, 5), (0, -3), (128, -40)):
        margin = image - (m + k64 / 64 * s + c)
        clear = np.abs(margin) > 1e-6
        assert clear.sum() > 90
        assert (wr.local_threshold(image, 2, k64, c, -1)[clear] == (margin > 0)[clear]).all()


def test_exact_tie_is_background():
    image = np.array([[0, 0, 0, 0, 200]], np.uint8)
    n, S, Q = wr.window_sums(image, 4)
    assert n[0, 4] == 5 and S[0, 4] == 200 and Q[0, 4] == 40000       # m = 40, s = 80: m + 2 s = 200 = v
    assert not wr.local_threshold(image, 4, 128, 0, -1)[0, 4]
    assert wr.local_threshold(image, 4, 127, 0, -1)[0, 4]
    assert not wr.local_threshold(image, 4, 128, 0, -1).any()


def test_constant_images_and_empty_selections():
    image = np.full((6, 7), 93, np.uint8)
    assert not wr.local_threshold(image, 2, 13, 0, -1).any()            # D = 0, c = 0: v = m is not above m
    assert not wr.local_threshold(image, 2, -13, 0, -1).any()
    assert wr.local_threshold(image, 2, 13, -1, -1).all() and wr.local_threshold(image, 2, -128, -1, -1).all()
    assert not wr.local_threshold(image, 2, 13, -1, 93).any() and wr.local_threshold(image, 2, 13, -1, 92).all()      # the floor
    n, S, Q = wr.window_sums(image, 2, np.zeros((6, 7), np.uint8))
    assert not n.any() and not S.any() and not Q.any()
    assert not wr.local_threshold(image, 2, -128, -255, -1, np.zeros((6, 7), np.uint8)).any()      # n = 0: background


def test_closed_forms_at_the_largest_window():
    image = np.full((255, 255), 255, np.uint8)
    n, S, Q = wr.window_sums(image, 127)
    assert n[127, 127] == (2 * 127 + 1) ** 2 == 65025 and S[127, 127] == 255 * 65025
    assert Q[127, 127] == 4228250625 and 2 ** 31 < Q[127, 127] < 2 ** 32
    assert n[0, 0] == 128 * 128 and n[0, 254] == 128 * 128 and n[127, 0] == 255 * 128
    assert (Q == 255 * 255 * n).all() and (S == 255 * n).all()


def test_int64_bounds_at_the_extreme_window():
    """32 512 zeros and 32 513 values of 255: the largest variance a window can have, with the pixel and the offset at their ends."""
    n, ones = 65025, 32513
    S, Q = 255 * ones, 255 * 255 * ones
    D = n * Q - S * S
    assert D == 255 * 255 * ones * (n - ones) <= n * n * 255 * 255 // 4 and D <= 6.874e13
    assert 128 * 128 * D <= 1.13e18 < 2 ** 63
    worst_L = max(abs(64 * (n * v - s - c * n)) for v in (0, 255) for s in (0, 255 * n) for c in (-255, 255))
    assert worst_L == 64 * 2 * 255 * n < 2 ** 31 and worst_L ** 2 < 2 ** 62
    assert math.log2(worst_L) < 31.0
    # the restatement, which computes in int64, agrees with Python integers there
    for v in (0, 255):
        for c in (-255, 0, 255):
            for k64 in (-128, 128):
                got = bool(wr.decide(v, n, S, Q, k64, c, -1))
                assert got == exact_rule(v, n, S, Q, k64, c, -1)


def test_ramp_example_global_threshold_fails_local_rule_is_perfect():
    plane, disc = wr.ramp_discs()
    assert plane.shape == (256, 256) and plane[0, 0] == 20 and plane[0, 255] == 140 and disc.max() == 64
    t = wr.otsu(plane)
    assert t == 85
    fg = plane > t
    lost = [d for d in range(1, 65) if not fg[disc == d].any()]
    assert len(lost) == 8                                               # the discs of the darkest column
    assert int((fg & (disc == 0)).sum()) == 25960
    local = wr.local_threshold(plane, 20, 0, 15, -1)
    assert (local == (disc > 0)).all()
