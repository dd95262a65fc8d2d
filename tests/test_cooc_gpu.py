"""GPU: the region co-occurrence (csrc/region.hip; cgc_net_amd.nuclei.region_cooccurrence, cooccurrence_properties, texture_features)
against tests/cooc_ref.py, bit for bit, at the smallest shapes at which each mechanism can fail: partners beyond the tile seam, in
another band, wave or tile, negative column offsets, partners that a clamped address would alias, label boundaries, more labels in a
tile than its table holds, colliding labels, a bin at its capacity, ``within`` at the anchor and at the partner."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, nuclei

import cooc_ref as ref
from image_cases import DEV, DTYPES, gpu, tissue

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRS = nuclei.COOC_DIRECTIONS
LONG = ((1, -1), (3, -16), (16, 16), (-16, 5), (0, 16))


@functools.lru_cache(maxsize=None)
def geometry():
    k = kernels.get()
    return k.region_tile, k.region_slots


def check(labels, values, offsets=DIRS, levels=16, lut=None, symmetric=True, max_label=None, within=None):
    """The tables against the restatement; labels, values, within: numpy arrays.  Returns the tables as int64 numpy."""
    top = int(labels.max()) if max_label is None and labels.size else (max_label or 0)
    got = nuclei.region_cooccurrence(gpu(labels), gpu(values), offsets, levels, lut, symmetric, max_label,
                                     None if within is None else gpu(within))
    assert got.dtype == torch.int32 and tuple(got.shape) == (top + 1, len(offsets), levels, levels) and got.is_cuda
    want = ref.tables(labels, values, offsets, levels, lut, symmetric, top, within)
    got = got.cpu().numpy().astype(np.int64)
    assert np.array_equal(got, want)
    return got


def random_case(H, W, top, seed, block=1):
    """Labels 0..top in blocks of ``block`` x ``block`` pixels, random uint8 values."""
    rng = np.random.RandomState(seed)
    small = rng.randint(0, top + 1, (-(-H // block), -(-W // block))).astype(np.int32)
    labels = small if block == 1 else np.kron(small, np.ones((block, block), np.int32))[:H, :W]
    return np.ascontiguousarray(labels), rng.randint(0, 256, (H, W)).astype(np.uint8)


def pairs(H, W, dy, dx):
    return max(0, H - abs(dy)) * max(0, W - abs(dx))


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize('shape', [(0, 5), (5, 0), (1, 1), (1, 7), (7, 1)])
def test_degenerate_shapes(shape):
    labels, values = random_case(shape[0], shape[1], 3, 1)
    for symmetric in (True, False):
        check(labels, values, symmetric=symmetric, max_label=3)
    got = check(labels, values)                                         # the range read from the labels; an empty image has row 0 only
    assert got.shape[0] == (int(labels.max()) + 1 if labels.size else 1)
    check(np.zeros(shape, np.int32), values, symmetric=False, max_label=0)
    assert check(labels, values, max_label=3, within=np.zeros(shape, bool)).sum() == 0


def test_max_label_far_above_the_largest():
    t, S = geometry()
    labels, values = random_case(t + 3, 9, 5, 2)
    got = check(labels, values, levels=8, max_label=5000)               # rows 6 .. 5000 are empty
    assert got[6:].sum() == 0 and got[:6].sum() > 0


# ------------------------------------------------------------------ tile seams
def test_tile_seams_random():
    t, S = geometry()
    labels, values = random_case(t + 3, 2 * t + 5, 4, 3)
    got = check(labels, values, offsets=DIRS + ((-1, 0), (0, -1)), symmetric=False)
    assert (got.sum(axis=(0, 2, 3)) > 0).all()


def test_one_label_every_pair_is_counted_once():
    t, S = geometry()
    n = 2 * t + 1
    labels = np.zeros((n, n), np.int32)
    values = np.random.RandomState(4).randint(0, 256, (n, n)).astype(np.uint8)
    offsets = DIRS + ((-1, 0), (0, -1), (-1, -1), (-1, 1))
    got = check(labels, values, offsets=offsets, symmetric=False)
    assert got.sum(axis=(0, 2, 3)).tolist() == [pairs(n, n, dy, dx) for dy, dx in offsets]      # from arithmetic, not the restatement
    got = check(labels, values, offsets=offsets, symmetric=True)
    assert got.sum(axis=(0, 2, 3)).tolist() == [2 * pairs(n, n, dy, dx) for dy, dx in offsets]


# ------------------------------------------------------------------ negative and long offsets
def test_long_and_negative_offsets():
    t, S = geometry()
    labels, values = random_case(t + 20, t + 20, 2, 5, block=8)
    got = check(labels, values, offsets=LONG, symmetric=False)
    assert (got.sum(axis=(0, 2, 3)) > 0).all()                          # every offset finds pairs inside the 8 x 8 blocks or across them
    check(labels, values, offsets=LONG, levels=5, symmetric=True, within=np.random.RandomState(6).rand(t + 20, t + 20) < 0.8)
    one = check(np.zeros_like(labels), values, offsets=LONG, symmetric=False)
    assert one.sum(axis=(0, 2, 3)).tolist() == [pairs(t + 20, t + 20, dy, dx) for dy, dx in LONG]


def test_offsets_that_pass_the_image():
    labels, values = random_case(5, 5, 1, 7)
    got = check(np.zeros_like(labels), values, offsets=LONG)
    assert got.sum(axis=(0, 2, 3)).tolist() == [2 * 16, 0, 0, 0, 0]     # only (1, -1) fits 5 x 5
    check(labels, values, offsets=LONG, symmetric=False)
    check(labels, values, offsets=((4, 4), (-4, -4), (5, 0), (0, -5), (4, -4)), symmetric=False)


# ------------------------------------------------------------------ clamped partners are never counted
@pytest.mark.parametrize('shape', ['small', 'seam'])
def test_a_clamped_partner_is_not_a_pair(shape):
    """A constant image of one label whose last row and column hold another value: a partner read through a clamped address would be
    the anchor itself or its neighbour on the edge, and would add to the diagonal bin of the edge value."""
    t, S = geometry()
    H, W = (5, 7) if shape == 'small' else (t + 5, t + 9)
    labels = np.zeros((H, W), np.int32)
    values = np.full((H, W), 10, np.uint8)
    values[-1, :] = values[:, -1] = 200
    offsets = DIRS + ((-1, 0), (0, -1), (3, -4), (-4, 3))
    got = check(labels, values, offsets=offsets, symmetric=False)
    lo, hi = 10 * 16 >> 8, 200 * 16 >> 8
    assert got[0, 0, lo, lo] == (H - 1) * (W - 2) and got[0, 0, lo, hi] == H - 1 and got[0, 0, hi, hi] == W - 1      # (0, 1)
    assert got[0, 2, lo, lo] == (H - 2) * (W - 1) and got[0, 2, lo, hi] == W - 1 and got[0, 2, hi, hi] == H - 1      # (1, 0)
    assert got[0, 1, hi, hi] == 0 and got[0, 1, lo, hi] == H + W - 3      # (1, 1): the edge is only ever a partner, the corner too
    assert got[0, 4, hi, hi] == H - 1 and got[0, 5, hi, hi] == W - 1      # (-1, 0), (0, -1): along the edge itself
    assert got.sum(axis=(0, 2, 3)).tolist() == [pairs(H, W, dy, dx) for dy, dx in offsets]
    check(labels, values, offsets=LONG, symmetric=True)


# ------------------------------------------------------------------ label boundaries
def test_checkerboard_and_stripes():
    t, S = geometry()
    H, W = t + 3, t + 5
    yy, xx = np.mgrid[0:H, 0:W]
    values = np.random.RandomState(8).randint(0, 256, (H, W)).astype(np.uint8)
    got = check(((yy + xx) % 2 + 1).astype(np.int32), values, symmetric=False)
    assert got.sum(axis=(0, 2, 3)).tolist() == [0, (H - 1) * (W - 1), 0, (H - 1) * (W - 1)] and got[0].sum() == 0
    got = check(xx.astype(np.int32), values, levels=4, symmetric=False)   # vertical stripes of width 1
    assert got.sum(axis=(0, 2, 3)).tolist() == [0, 0, (H - 1) * W, 0]


def test_every_pixel_its_own_label():
    t, S = geometry()
    n = t + 6
    labels = np.random.RandomState(9).permutation(n * n).astype(np.int32).reshape(n, n)
    values = np.random.RandomState(10).randint(0, 256, (n, n)).astype(np.uint8)
    assert check(labels, values, levels=4).sum() == 0


# ------------------------------------------------------------------ more labels than the table holds
@pytest.mark.parametrize('extra', [0, 1])
def test_exactly_as_many_labels_as_slots_and_one_more(extra):
    t, S = geometry()
    rng = np.random.RandomState(11 + extra)
    small = rng.randint(0, S + extra, (t // 2, t // 2)).astype(np.int32)
    small.reshape(-1)[:S + extra] = np.arange(S + extra)                # every label is there
    labels = np.kron(small, np.ones((2, 2), np.int32))                  # one tile, blocks of 2 x 2: pairs exist
    values = rng.randint(0, 256, (t, t)).astype(np.uint8)
    got = check(labels, values)
    assert got.shape[0] == S + extra and (got.sum(axis=(2, 3)) > 0).all()
    check(labels, values, symmetric=False, levels=7)


def test_the_direct_route_with_within_on_partial_tiles():
    t, S = geometry()
    n = t + 6                                                           # even; four tiles, three of them partial
    perm = np.random.RandomState(13).permutation(n * n // 2).astype(np.int32)
    labels = perm[np.arange(n * n) // 2].reshape(n, n)                  # a label is two pixels side by side: far more than S per tile
    values = np.random.RandomState(14).randint(0, 256, (n, n)).astype(np.uint8)
    within = np.ones((n, n), np.int32)
    within[:, ::3] = 0                                                  # every third column: it splits some of the pairs
    offsets = ((0, 1), (0, -1), (1, 0))
    for symmetric in (True, False):
        got = check(labels, values, offsets=offsets, symmetric=symmetric, within=within)
        assert got[:, 0].sum() == got[:, 1].sum() > 0 and got[:, 2].sum() == 0


def test_labels_that_collide_in_the_hash():
    t, S = geometry()
    source = open(os.path.join(ROOT, 'cgc-net_amd', 'csrc', 'region.hip')).read()
    mult = int(re.search(r'\(unsigned\)L \* (0x[0-9A-Fa-f]+)u\) >> \(32 - REGION_SLOT_BITS\)', source).group(1), 16)
    bits = S.bit_length() - 1
    slot = lambda L: ((L * mult) & 0xffffffff) >> (32 - bits)           # noqa: E731
    ids = np.array([L for L in range(1, 4000) if slot(L) == slot(1)][:40], np.int32)
    assert len(ids) == 40 and len(set(slot(int(L)) for L in ids)) == 1  # forty labels, one home slot: most find no slot in 8 probes
    rng = np.random.RandomState(13)
    H, W = t + 10, t + 2
    labels = np.kron(ids[rng.randint(0, 40, (H // 2, W // 2))], np.ones((2, 2), np.int32))
    labels[::7] = ids[1]                                                # and long runs of one of them
    values = rng.randint(0, 256, (H, W)).astype(np.uint8)
    check(labels, values, levels=4)
    check(labels, values, levels=4, symmetric=False, within=rng.rand(H, W) < 0.5)


# ------------------------------------------------------------------ bin capacity
def test_one_label_one_value_over_nine_tiles():
    t, S = geometry()
    n = 3 * t
    labels = np.full((n, n), 2, np.int32)
    values = np.full((n, n), 77, np.uint8)
    got = check(labels, values)                                         # the diagonal bin of the interior tile takes 2 x 4096
    lv = 77 * 16 >> 8
    assert got[2, :, lv, lv].tolist() == [2 * pairs(n, n, dy, dx) for dy, dx in DIRS] and got.sum() == got[2, :, lv, lv].sum()


# ------------------------------------------------------------------ within
def test_within_at_the_anchor_and_at_the_partner():
    t, S = geometry()
    H, W = 2, t + 1                                                     # the last pair of a row crosses the tile seam
    labels = np.zeros((H, W), np.int32)
    values = np.random.RandomState(14).randint(0, 256, (H, W)).astype(np.uint8)
    total = lambda w: int(check(labels, values, offsets=((0, 1),), symmetric=False, within=w).sum())      # noqa: E731
    w = np.ones((H, W), np.uint8)
    assert total(w) == 2 * t
    w[0, 0] = 0                                                         # only ever an anchor
    assert total(w) == 2 * t - 1
    w[0, 0], w[0, t] = 1, 0                                             # only ever a partner, beyond the seam
    assert total(w) == 2 * t - 1
    w[0, t], w[1, t - 1] = 1, 0                                         # the partner of one pair, the anchor of the next
    assert total(w) == 2 * t - 2
    # the same for a vertical offset that leaves the thread's band and the tile
    labels, values = np.zeros((t + 1, 2), np.int32), values.T.copy()
    for y in (0, 15, 16, t - 1, t):
        w = np.ones((t + 1, 2), bool)
        w[y, 1] = False
        got = check(labels, values, offsets=((1, 0), (-1, 0)), symmetric=False, within=w)
        assert got.sum(axis=(0, 2, 3)).tolist() == [2 * t - (1 if y in (0, t) else 2)] * 2


@pytest.mark.parametrize('dtype', DTYPES)
def test_within_of_every_dtype_with_strides(dtype):
    t, S = geometry()
    labels, values, _ = tissue()
    labels, values = labels[:t + 7, :t + 11], values[:t + 7, :t + 11]
    rng = np.random.RandomState(15)
    within = rng.rand(*labels.shape) < 0.7
    wide = torch.zeros(labels.shape[0], 2 * labels.shape[1], dtype=dtype, device=DEV)
    info = None if dtype == torch.bool else torch.iinfo(dtype)
    fill = gpu(within) if dtype == torch.bool else gpu(np.where(within, rng.choice([1, 2, info.max, info.min or 5], labels.shape), 0)).to(dtype)
    wide[:, ::2] = fill
    Wn = wide[:, ::2]
    assert not Wn.is_contiguous() and torch.equal(Wn != 0, gpu(within))
    got = nuclei.region_cooccurrence(gpu(labels), gpu(values), within=Wn)
    assert np.array_equal(got.cpu().numpy(), ref.tables(labels, values, DIRS, 16, None, True, int(labels.max()), within))


@pytest.mark.parametrize('ldtype', [torch.int64, torch.uint8])
def test_label_planes_of_other_dtypes_and_strides(ldtype):
    t, S = geometry()
    labels, values = random_case(t + 2, t + 9, 100, 16, block=3)
    L, V = gpu(labels.T.copy()).to(ldtype).T, gpu(values.T.copy()).T
    assert not L.is_contiguous() and not V.is_contiguous()
    got = nuclei.region_cooccurrence(L, V, max_label=100)
    assert np.array_equal(got.cpu().numpy(), ref.tables(labels, values, DIRS, 16, None, True, 100, None))
    if ldtype == torch.int64:
        bad = L.clone()
        bad[1, 1] = 2 ** 32 + 1                                         # would be label 1 after a narrowing cast
        with pytest.raises(ValueError, match='outside'):
            nuclei.region_cooccurrence(bad, V, max_label=100)


# ------------------------------------------------------------------ levels and tables
@pytest.mark.parametrize('levels', [2, 3, 7, 16])
def test_levels(levels):
    t, S = geometry()
    labels, values = random_case(t + 5, t + 1, 3, 17, block=4)
    got = check(labels, values, levels=levels)
    assert (got.sum(axis=(0, 1)) > 0).all()                             # every pair of levels occurs
    fold = (np.random.RandomState(18).permutation(256) % levels)
    for lut in (fold.tolist(), tuple(fold.tolist()), fold, fold.astype(np.uint8), torch.from_numpy(fold)):
        check(labels, values, levels=levels, lut=lut, symmetric=False)


def test_level_lut_with_bounds_and_bool_values():
    t, S = geometry()
    labels, values = random_case(t + 5, t + 1, 3, 19, block=4)
    lut = nuclei.level_lut(8, 20, 159)
    got = check(labels, values, levels=8, lut=lut)
    assert np.array_equal(got, ref.tables(labels, values, DIRS, 8, ref.level_lut(8, 20, 159), True, 3, None))
    flags = values > 100
    got = nuclei.region_cooccurrence(gpu(labels), gpu(flags), levels=2, lut=[0] + [1] * 255, symmetric=False)
    assert np.array_equal(got.cpu().numpy(), ref.tables(labels, flags.astype(np.uint8), DIRS, 2, [0] + [1] * 255, False, 3, None))


def test_symmetric_is_plain_plus_its_transpose_and_reversed_offsets_transpose():
    labels, values, within = tissue()
    L, V, Wn = gpu(labels), gpu(values), gpu(within)
    offsets = DIRS + ((2, -3), (0, 16))
    plain = nuclei.region_cooccurrence(L, V, offsets, symmetric=False, within=Wn)
    sym = nuclei.region_cooccurrence(L, V, offsets, symmetric=True, within=Wn)
    assert torch.equal(sym, plain + plain.transpose(2, 3))
    back = nuclei.region_cooccurrence(L, V, [(-dy, -dx) for dy, dx in offsets], symmetric=False, within=Wn)
    assert torch.equal(back, plain.transpose(2, 3))


# ------------------------------------------------------------------ refusals that need the device
def test_labels_outside_the_range_raise_and_are_counted_once():
    t, S = geometry()
    labels, values = random_case(t + 3, t + 3, 5, 20, block=2)
    L, V = gpu(labels), gpu(values)
    n = int((labels == 5).sum())
    assert n > 0
    with pytest.raises(ValueError, match='region_cooccurrence: %d pixels carry a label outside \\[0, 4\\]' % n):
        nuclei.region_cooccurrence(L, V, max_label=4)                   # four offsets: the count is not four times the pixels
    bad = L.clone()
    bad[t + 1, t + 2] = -3
    with pytest.raises(ValueError, match=' 1 pixels .* outside'):
        nuclei.region_cooccurrence(bad, V, max_label=5, within=torch.zeros_like(L))      # ... whatever `within` says there
    with pytest.raises(ValueError, match='negative'):
        nuclei.region_cooccurrence(bad, V)
    # the library counts them once per call, and the rest is still exact
    k = kernels.get()
    for offsets in (DIRS, DIRS + LONG[1:], ((0, 1),)):
        tables, meta = k.region_cooccurrence(L, V, 4, ref.level_lut(16), 16, offsets, True)
        assert int(meta) == n == ref.refused(labels, 4)
        want = ref.tables(labels, values, offsets, 16, None, True, 4, None)
        assert np.array_equal(tables.view(5, len(offsets), 16, 16).cpu().numpy(), want)
    assert k.region_cooc_max_offset == nuclei.COOC_MAX_OFFSET == 16 and k.region_cooc_max_offsets == nuclei.COOC_MAX_OFFSETS == 8


# ------------------------------------------------------------------ tissue
def test_tissue_twice_bit_identical():
    labels, values, within = tissue()
    L, V, Wn = gpu(labels), gpu(values), gpu(within)
    a = nuclei.region_cooccurrence(L, V, within=Wn)
    b = nuclei.region_cooccurrence(L, V, within=Wn)
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), ref.tables(labels, values, DIRS, 16, None, True, int(labels.max()), within))
    c = nuclei.region_cooccurrence(L, V, offsets=nuclei.cooc_directions(3), levels=8, symmetric=False, within=L != 0)
    assert int(c[0].sum()) == 0 and int(c.sum()) > 0                    # the background is left out by `within`
    assert np.array_equal(c.cpu().numpy(), ref.tables(labels, values, nuclei.cooc_directions(3), 8, None, False, int(labels.max()), labels != 0))


# ------------------------------------------------------------------ properties
REL, ABS, CORR_ABS = 2.0 ** -23, 2.0 ** -40, 2.0 ** -22


def test_properties_within_the_rounding_of_float32():
    """Every property but correlation is a sum of at most 256 non-negative float64 terms (relative error of the sum at most about 256
    * 2^-53 = 2^-45, and the same again for the reference) and one rounding to float32, 2^-24 |x|: the bound is 2^-23 |x| plus 2^-40
    absolute for values next to zero.  Entropy's terms -P log2 P are non-negative too.  Correlation lies in [-1, 1]: one float32
    rounding is at most 2^-25 there, and the float64 error of the centred sums, 256 terms of at most 15^2, divided by sigma_i sigma_j,
    is 256 * 15^2 * 2^-52 / (sigma_i sigma_j) -- the test computes the smallest sigma_i sigma_j of the regions it compares and asserts
    that this stays below the bound 2^-22."""
    labels, values, within = tissue()
    tables = nuclei.region_cooccurrence(gpu(labels), gpu(values), within=gpu(within))
    got = nuclei.cooccurrence_properties(tables)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(tables.shape[:2]) + (7,) and got.is_cuda
    got = got.cpu().numpy().astype(np.float64)
    ints = tables.cpu().numpy().astype(np.int64)
    want = ref.properties(ints)
    corr = ref.PROPERTIES.index('correlation')
    for c, name in enumerate(ref.PROPERTIES):
        if c != corr:
            assert (np.abs(got[:, :, c] - want[:, :, c]) <= REL * np.abs(want[:, :, c]) + ABS).all(), name
    # correlation: the regions whose integer marginals have at least two levels
    two = ((ints.sum(axis=3) != 0).sum(axis=2) >= 2) & ((ints.sum(axis=2) != 0).sum(axis=2) >= 2)
    assert two.sum() >= 100
    n = ints.sum(axis=(2, 3)).astype(np.float64)
    p = ints / np.where(n > 0, n, 1)[:, :, None, None]
    lv = np.arange(16, dtype=np.float64)
    pi, pj = p.sum(axis=3), p.sum(axis=2)
    var_i = (pi * lv ** 2).sum(axis=2) - (pi * lv).sum(axis=2) ** 2
    var_j = (pj * lv ** 2).sum(axis=2) - (pj * lv).sum(axis=2) ** 2
    smallest = float(np.sqrt(var_i[two] * var_j[two]).min())
    assert 256 * 15 ** 2 * 2.0 ** -52 / smallest + 2.0 ** -25 < CORR_ABS, smallest
    assert (np.abs(got[:, :, corr] - want[:, :, corr])[two] <= CORR_ABS).all()
    assert (np.abs(got[:, :, corr]) <= 1 + CORR_ABS).all()
    # the rest: one level only gives exactly 1, no pair gives exactly 0
    assert (got[:, :, corr][~two & (n > 0)] == 1).all() and (got[n == 0] == 0).all()
    some = nuclei.cooccurrence_properties(tables, ('entropy', 'ASM'))
    assert torch.equal(some, nuclei.cooccurrence_properties(tables)[:, :, [6, 3]])


def test_properties_of_one_level_and_of_no_pair_are_exact():
    labels = np.zeros((6, 9), np.int32)
    labels[:3, :4] = 1                                                  # one value throughout: one level in both marginals
    labels[4:, 5:] = 3                                                  # two rows of one value each: (0, 1) has one level, (1, 0) has
    values = np.random.RandomState(22).randint(0, 256, (6, 9)).astype(np.uint8)      # one level per marginal; label 2 has no pixel
    values[:3, :4] = 90
    values[4, 5:], values[5, 5:] = 20, 250
    tables = nuclei.region_cooccurrence(gpu(labels), gpu(values), ((0, 1), (1, 0)), symmetric=False, max_label=4)
    got = nuclei.cooccurrence_properties(tables).cpu().numpy()
    assert got[1].tolist() == [[0, 0, 1, 1, 1, 1, 0]] * 2
    assert got[2].tolist() == [[0] * 7] * 2 and got[4].tolist() == [[0] * 7] * 2
    assert got[3, 0, 5] == 1 and got[3, 1, 5] == 1                      # levels 1 and 15 in step: 49 / sqrt(49 * 49); sigma_i = 0: 1 by rule
    assert got[3, 1].tolist() == [14 ** 2, 14, np.float32(1 / 197), 1, 1, 1, 0]      # levels 1 above 15
    assert np.array_equal(got[1:], ref.properties(tables.cpu().numpy()).astype(np.float32)[1:])      # exact values only


# ------------------------------------------------------------------ texture_features
@functools.lru_cache(maxsize=None)
def stained_tissue():
    labels, gray, _ = tissue()
    L, G = gpu(labels), gpu(gray)
    tile = torch.stack([G, 255 - G // 2, 128 + G // 4], dim=2).contiguous()
    top = int(labels.max())
    _, _, kept = nuclei.nucleus_features(L, G, max_label=top)
    return L, tile, kept, top


def rebuilt(L, tile, kept, top, planes, levels, lo, hi, distance):
    columns = []
    for plane in nuclei.separate_stains(tile, planes=planes):
        tables = nuclei.region_cooccurrence(L, plane, nuclei.cooc_directions(distance), levels, nuclei.level_lut(levels, lo, hi), True, top,
                                            within=L != 0)
        props = nuclei.cooccurrence_properties(tables, ('contrast', 'dissimilarity', 'homogeneity', 'energy', 'correlation', 'entropy'))
        for c in range(6):
            d = [props[:, k, c] for k in range(4)]
            most, least = torch.stack(d).max(0)[0], torch.stack(d).min(0)[0]
            columns += [((d[0] + d[1]) + (d[2] + d[3])) * 0.25, most - least]
    return torch.stack(columns, dim=1)[kept.long()]


def test_texture_features_are_the_columns_rebuilt_from_the_parts():
    L, tile, kept, top = stained_tissue()
    assert kept.numel() > 20
    feats = nuclei.texture_features(L, tile, kept, hi=159, max_label=top)
    assert feats.dtype == torch.float32 and tuple(feats.shape) == (kept.numel(), 12) == (kept.numel(), len(nuclei.TEXTURE_FEATURE_NAMES))
    assert torch.equal(feats, rebuilt(L, tile, kept, top, (0,), 16, 0, 159, 1))
    assert torch.equal(feats, nuclei.texture_features(L, tile, kept, hi=159))      # the range read from the labels; bit-identical
    assert bool(torch.isfinite(feats).all()) and float(feats.std(0).min()) > 0    # the columns say something
    two = nuclei.texture_features(L, tile, kept, planes=(0, 1), levels=8, lo=10, distance=2, max_label=top)
    assert tuple(two.shape) == (kept.numel(), 24) and torch.equal(two, rebuilt(L, tile, kept, top, (0, 1), 8, 10, 255, 2))
    pick = torch.flip(kept, [0])[::3]                                   # row k describes kept_labels[k]
    assert torch.equal(nuclei.texture_features(L, tile, pick.to(torch.int64), hi=159, max_label=top), torch.flip(feats, [0])[::3])
    names = nuclei.TEXTURE_FEATURE_NAMES
    assert names[0] == 'hematoxylin_contrast_mean' and names[9] == 'hematoxylin_correlation_range' and len(set(names)) == 12


def test_texture_features_refuses_kept_labels_out_of_range():
    L, tile, kept, top = stained_tissue()
    for bad in ([1, top + 1], [-1, 2], [2 ** 31 - 1]):
        with pytest.raises(ValueError, match='kept_labels'):
            nuclei.texture_features(L, tile, torch.tensor(bad, dtype=torch.int32, device=DEV), max_label=top)
    with pytest.raises(ValueError, match='outside'):
        nuclei.texture_features(L, tile, torch.tensor([1], dtype=torch.int32, device=DEV), max_label=top - 1)
    assert tuple(nuclei.texture_features(L, tile, torch.zeros(0, dtype=torch.int32, device=DEV), max_label=top).shape) == (0, 12)
