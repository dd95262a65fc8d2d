"""CPU: tests/rank_ref.py, the numpy restatement the GPU tests of the rank filters compare against, pinned from outside: against a
sort-based double loop, against scipy.ndimage on whole footprints, against tests/morph_ref.py at the extreme quantiles, against the
literal cases of the contract, against closed forms and float64 for the entropy, and its table of entropy terms against the
library's."""
import ctypes
import decimal
import math

import numpy as np
import pytest
from scipy import ndimage

import cgc_net_amd  # noqa: F401
from cgc_net_amd import _abi, kernels

import morph_ref
import rank_ref as ref

KINDS = ref.KINDS
QS = (0, 1, 1999, 2000, 2500, 4999, 5000, 7500, 9999, 10000)


def random_image(H, W, seed=0, levels=256):
    return np.random.RandomState(seed + 13 * H + W).randint(0, levels, (H, W)).astype(np.uint8)


def random_within(H, W, seed=0, p=0.6):
    return np.random.RandomState(1000 + seed + 7 * H + W).rand(H, W) < p


def windows(image, kind, r, within=None):
    """The definition, pixel by pixel: yields (y, x, the sorted counted values of the clipped footprint)."""
    H, W = image.shape
    offs = ref.offsets(kind, r)
    for y in range(H):
        for x in range(W):
            v = [int(image[y + dy, x + dx]) for dy, dx in offs
                 if 0 <= y + dy < H and 0 <= x + dx < W and (within is None or within[y + dy, x + dx] != 0)]
            yield y, x, sorted(v)


def test_footprint_widths_are_morph_refs():
    assert ref.MAX_RADIUS == morph_ref.MAX_RADIUS and ref.KINDS == morph_ref.KINDS
    for kind in KINDS:
        for r in (0, 1, 2, 3, 5, 7, 15, 31, 63):
            assert [ref.width(kind, r, dy) for dy in range(-r, r + 1)] == [morph_ref.width(kind, r, dy) for dy in range(-r, r + 1)]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('masked', (False, True))
def test_against_a_sort_based_double_loop(kind, masked):
    for (H, W), r, levels in (((1, 1), 0, 256), ((1, 1), 2, 256), ((1, 7), 1, 256), ((6, 1), 3, 256), ((7, 9), 2, 4), ((8, 6), 3, 256),
                              ((5, 5), 7, 3)):
        image = random_image(H, W, r, levels)
        within = random_within(H, W, r).astype(np.int16) * 256 if masked else None
        cum = ref.cumulative(image, kind, r, within)
        got = {q: ref.quantile_of(cum, q) for q in QS}
        rng = ref.rank_filter_u8(image, kind, r, 'range', 2500, 7500, within)
        E, n, m = ref.entropy_of(cum)
        h16 = ref.h16_of(cum)
        for y, x, v in windows(image, kind, r, within):
            assert n[y, x] == len(v)
            for q in QS:
                want = v[min(len(v) - 1, len(v) * q // 10000)] if v else 0
                assert got[q][y, x] == want, (H, W, r, q, y, x)
            if v:
                assert rng[y, x] == v[min(len(v) - 1, len(v) * 7500 // 10000)] - v[min(len(v) - 1, len(v) * 2500 // 10000)]
                counts = np.bincount(v)
                assert m[y, x] == (counts > 0).sum()
                assert E[y, x] == ref.TERMS[len(v)] - ref.TERMS[counts].sum()
                assert h16[y, x] == E[y, x] // len(v)
            else:
                assert rng[y, x] == 0 and h16[y, x] == 0 and E[y, x] == 0


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('r', (1, 2, 3, 5))
def test_against_scipy_on_whole_footprints(kind, r):
    image = random_image(23, 29, r)
    fp = ref.footprint(kind, r)
    cum = ref.cumulative(image, kind, r)
    inner = (slice(r, 23 - r), slice(r, 29 - r))
    assert np.array_equal(cum[255][inner], np.full((23 - 2 * r, 29 - 2 * r), fp.sum()))
    assert np.array_equal(ref.quantile_of(cum, 5000)[inner], ndimage.median_filter(image, footprint=fp)[inner])
    for percent in (0, 25, 50, 75, 100):                               # n * percent / 100 is exact in binary
        assert np.array_equal(ref.quantile_of(cum, percent * 100)[inner], ndimage.percentile_filter(image, percent, footprint=fp)[inner])


@pytest.mark.parametrize('kind', KINDS)
def test_the_extreme_quantiles_are_morph_refs_extrema(kind):
    for (H, W), r in (((9, 14), 0), ((9, 14), 2), ((12, 7), 5), ((3, 40), 31)):
        image = random_image(H, W, r)
        for within in (None, random_within(H, W, r, 0.3)):
            lo, hi = morph_ref.extrema(image, kind, r, within)
            cum = ref.cumulative(image, kind, r, within)
            some = cum[255] > 0
            assert np.array_equal(ref.quantile_of(cum, 0)[some], lo[some]) and np.array_equal(ref.quantile_of(cum, 10000)[some], hi[some])
            assert not ref.quantile_of(cum, 0)[~some].any() and not ref.quantile_of(cum, 10000)[~some].any()
            assert np.array_equal(ref.quantile_range(image, r, 0, 10000, kind, within), morph_ref.morph_gradient(image, r, kind, within))


def test_the_literal_cases_of_the_contract():
    two = np.array([[10, 20]], np.uint8)
    for kind in KINDS:
        assert ref.rank_filter(two, 1, 5000, kind).tolist() == [[20, 20]]
        assert ref.rank_filter(two, 1, 4999, kind).tolist() == [[10, 10]]
        assert ref.median(two, 1, kind).tolist() == [[20, 20]]
    # the interior of a square of r = 2: n = 25, the values 0..24 in some order
    image = np.random.RandomState(5).permutation(25).reshape(5, 5).astype(np.uint8)
    assert ref.rank_filter(image, 2, 2000, 'square')[2, 2] == 5 and ref.rank_filter(image, 2, 1999, 'square')[2, 2] == 4
    assert ref.rank_filter(image, 2, 0, 'square')[2, 2] == 0 and ref.rank_filter(image, 2, 10000, 'square')[2, 2] == 24
    assert ref.rank_filter(image, 2, 9999, 'square')[2, 2] == 24 and ref.rank_filter(image, 2, 1, 'square')[2, 2] == 0
    assert ref.rank_index(np.array([25, 25, 0, 1, 16129]), 2000).tolist() == [5, 5, -1, 0, 3225]
    # a bool image: the majority, a tie gives True, nothing counted gives False
    mask = np.array([[True, False, False, True]])
    assert ref.median(mask, 1, 'square').tolist() == [[True, False, False, True]]     # {T,F}, {T,F,F}, {F,F,T}, {F,T}
    assert ref.median(mask, 1, 'square', within=np.zeros((1, 4), np.uint8)).tolist() == [[False] * 4]
    assert ref.median(mask, 1).dtype == bool and ref.median(two, 1).dtype == np.uint8


def test_empty_images_and_empty_selections():
    for shape in ((0, 5), (5, 0), (0, 0)):
        image = np.zeros(shape, np.uint8)
        assert ref.rank_filter(image, 2, 5000).shape == shape and ref.quantile_range(image, 2, 0, 10000).shape == shape
        assert ref.local_entropy_raw(image, 2).shape == shape and ref.local_entropy_raw(image, 2).dtype == np.int32
    image = random_image(6, 7)
    none = np.zeros((6, 7), np.int64)
    assert not ref.rank_filter(image, 2, 10000, within=none).any() and not ref.quantile_range(image, 2, 0, 10000, within=none).any()
    assert not ref.local_entropy_raw(image, 2, within=none).any()


# ------------------------------------------------------------------ entropy
def test_entropy_closed_forms():
    const = np.full((9, 9), 77, np.uint8)
    for kind in KINDS:
        assert not ref.local_entropy_raw(const, 3, kind).any()
    # two values half and half: exactly one bit.  A 1 x 4 window of a 1 x 4 image holds everything at r = 3
    half = np.array([[5, 9, 5, 9]], np.uint8)
    assert ref.local_entropy_raw(half, 3, 'square').tolist() == [[65536] * 4]
    assert ref.local_entropy_raw(np.array([[3, 200]], np.uint8), 1).tolist() == [[65536, 65536]]
    # a (1, 3) split: H = 2 - (3 / 4) log2 3
    split = np.array([[1, 2, 2, 2]], np.uint8)
    got = ref.local_entropy_raw(split, 3, 'square')
    want = (ref.TERMS[4] - ref.TERMS[3]) // 4
    assert got.tolist() == [[want] * 4] and ref.TERMS[4] == 8 * 65536
    assert abs(want / 65536 - (2 - 0.75 * math.log2(3))) <= 2 ** -15
    # all n values differ: log2 n
    ramp = np.arange(16, dtype=np.uint8).reshape(1, 16)
    assert ref.local_entropy_raw(ramp, 15, 'square').tolist() == [[4 * 65536] * 16]


@pytest.mark.parametrize('kind', KINDS)
def test_entropy_bounds_against_float64(kind):
    for (H, W), r, levels in (((20, 23), 3, 256), ((20, 23), 3, 5), ((17, 40), 15, 256), ((17, 40), 15, 3), ((9, 9), 1, 2), ((6, 6), 0, 256)):
        image = random_image(H, W, r, levels)
        for within in (None, random_within(H, W, r)):
            cum = ref.cumulative(image, kind, r, within)
            E, n, m = ref.entropy_of(cum)
            h16 = ref.h16_of(cum)
            counts = np.diff(cum, axis=0, prepend=0).astype(np.float64)
            with np.errstate(divide='ignore', invalid='ignore'):
                p = counts / n[None]
                H64 = -np.where(counts > 0, p * np.log2(p), 0.0).sum(axis=0)
            H64 = np.where(n > 0, H64, 0.0)
            assert (E >= 0).all() and np.array_equal(E == 0, m <= 1)
            assert (np.abs(E - 65536.0 * n * H64) <= (m + 1) / 2 + 1e-5).all()           # 1e-5: float64's own error, < 2^16 * 961 * 10 * 2^-50
            assert (np.abs(h16 / 65536.0 - H64) <= 2.0 ** -15).all()
            assert h16.dtype == np.int32 and h16.max() < 2 ** 24 and (h16[n == 0] == 0).all()


def test_the_table_of_entropy_terms():
    T = ref.TERMS
    assert len(T) == 962 == ref.ENTROPY_TERMS == kernels.RANK_ENTROPY_TERMS == (2 * ref.ENTROPY_MAX_RADIUS + 1) ** 2 + 1
    assert T[0] == T[1] == 0 and T[2] == 2 * 65536 and T[4] == 8 * 65536 and T[512] == 512 * 9 * 65536 and T.max() == T[961] < 2 ** 31
    # superadditive with a gap of two bits at least: E >= 0, and E == 0 only for one bin
    small = np.arange(1, 200)
    assert (T[small[:, None] + small[None]] - T[small][:, None] - T[small][None] >= 2 * 65536 - 2).all()
    # the library's table, entry by entry, against 50 digits and more
    import __graft_entry__ as ge
    ge.build()
    lib = ctypes.CDLL(kernels.lib_path())
    _abi.declare(lib)
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        ln2 = decimal.Decimal(2).ln()
        for c in range(962):
            exact = decimal.Decimal(c) * (decimal.Decimal(c).ln() / ln2) * 65536 if c > 1 else decimal.Decimal(0)
            got = lib.cgc_rank_entropy_term(c)
            assert got == T[c] and abs(decimal.Decimal(got) - exact) < decimal.Decimal('0.4993'), c      # nearest, and no near tie
    for c in (-1, 962, 1000, -2 ** 31, 2 ** 31 - 1):
        assert lib.cgc_rank_entropy_term(c) == -1
