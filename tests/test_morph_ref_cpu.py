"""CPU: tests/morph_ref.py, the numpy restatement the GPU tests of flat morphology compare against, pinned from outside: against
scipy.ndimage with an explicit footprint, against a plain double loop, against footprints written out by hand and against closed
forms."""
import numpy as np
import pytest
from scipy import ndimage

import morph_ref as ref

KINDS = ref.KINDS


def random_image(H, W, seed=0):
    return np.random.RandomState(seed + 13 * H + W).randint(0, 256, (H, W)).astype(np.uint8)


# ------------------------------------------------------------------ footprints
def test_footprints_written_out_by_hand():
    disk1 = [[0, 1, 0],
             [1, 1, 1],
             [0, 1, 0]]
    disk2 = [[0, 0, 1, 0, 0],
             [0, 1, 1, 1, 0],
             [1, 1, 1, 1, 1],
             [0, 1, 1, 1, 0],
             [0, 0, 1, 0, 0]]
    disk3 = [[0, 0, 0, 1, 0, 0, 0],                                     # skimage's disk(3)
             [0, 1, 1, 1, 1, 1, 0],
             [0, 1, 1, 1, 1, 1, 0],
             [1, 1, 1, 1, 1, 1, 1],
             [0, 1, 1, 1, 1, 1, 0],
             [0, 1, 1, 1, 1, 1, 0],
             [0, 0, 0, 1, 0, 0, 0]]
    diamond2 = disk2                                                    # |dx| + |dy| <= 2 and dx^2 + dy^2 <= 4 are the same set
    assert np.array_equal(ref.footprint('disk', 1), disk1)
    assert np.array_equal(ref.footprint('disk', 2), disk2)
    assert np.array_equal(ref.footprint('disk', 3), disk3)
    assert np.array_equal(ref.footprint('diamond', 2), diamond2)
    assert np.array_equal(ref.footprint('diamond', 1), disk1)
    assert np.array_equal(ref.footprint('square', 2), np.ones((5, 5)))
    for kind in KINDS:
        assert np.array_equal(ref.footprint(kind, 0), [[1]])


def test_footprints_by_their_definitions():
    for r in (0, 1, 2, 3, 4, 5, 7, 12, 31, 63):
        yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
        assert np.array_equal(ref.footprint('disk', r), (xx * xx + yy * yy <= r * r).astype(np.uint8)), r
        assert np.array_equal(ref.footprint('diamond', r), (abs(xx) + abs(yy) <= r).astype(np.uint8)), r
        assert ref.footprint('square', r).all()
        for kind in KINDS:
            f = ref.footprint(kind, r)
            assert np.array_equal(f, f[::-1]) and np.array_equal(f, f[:, ::-1]) and np.array_equal(f, f.T)
            assert len(ref.offsets(kind, r)) == f.sum()
    assert ref.width('disk', 5, 3) == 4 and ref.width('disk', 5, 4) == 3 and ref.width('disk', 5, 5) == 0      # 3-4-5: exact
    assert ref.width('disk', 63, 0) == 63 and ref.width('disk', 63, 63) == 0 and ref.width('disk', 63, 62) == 11


# ------------------------------------------------------------------ scipy
@pytest.mark.parametrize('kind', KINDS)
def test_erode_and_dilate_against_scipy(kind):
    for (H, W), r in (((1, 1), 2), ((5, 9), 1), ((5, 9), 7), ((23, 31), 3), ((40, 37), 6), ((12, 70), 20)):
        a = random_image(H, W)
        f = ref.footprint(kind, r)
        assert np.array_equal(ref.erode(a, r, kind), ndimage.grey_erosion(a, footprint=f, mode='constant', cval=255)), (H, W, r)
        assert np.array_equal(ref.dilate(a, r, kind), ndimage.grey_dilation(a, footprint=f, mode='constant', cval=0)), (H, W, r)


@pytest.mark.parametrize('kind', KINDS)
def test_compositions_against_scipy_on_the_interior(kind):
    """scipy pads erosion and dilation with the same constant, the contract clips: the two agree where no footprint of the
    composition reaches the border (r from it for the gradient, 2 r for the two-step operations)."""
    for (H, W), r in (((30, 41), 1), ((30, 41), 3), ((45, 38), 5)):
        a = random_image(H, W, 5)
        f = ref.footprint(kind, r)
        wide = a.astype(np.int32)
        kw = dict(footprint=f, mode='constant', cval=0)
        inner = (slice(r, H - r), slice(r, W - r))
        assert np.array_equal(ref.morph_gradient(a, r, kind)[inner], ndimage.morphological_gradient(wide, **kw)[inner])
        inner = (slice(2 * r, H - 2 * r), slice(2 * r, W - 2 * r))
        assert np.array_equal(ref.white_tophat(a, r, kind)[inner], ndimage.white_tophat(wide, **kw)[inner])
        assert np.array_equal(ref.black_tophat(a, r, kind)[inner], ndimage.black_tophat(wide, **kw)[inner])
        assert np.array_equal(ref.opening(a, r, kind)[inner], ndimage.grey_opening(wide, **kw)[inner])
        assert np.array_equal(ref.closing(a, r, kind)[inner], ndimage.grey_closing(wide, **kw)[inner])
        # the white top-hat's border rule does coincide when scipy is told each step's own neutral value
        opened = ndimage.grey_dilation(ndimage.grey_erosion(a, footprint=f, mode='constant', cval=255), footprint=f, mode='constant', cval=0)
        assert np.array_equal(ref.white_tophat(a, r, kind), a - opened) and (opened <= a).all()
        closed = ndimage.grey_erosion(ndimage.grey_dilation(a, footprint=f, mode='constant', cval=0), footprint=f, mode='constant', cval=255)
        assert np.array_equal(ref.black_tophat(a, r, kind), closed - a) and (closed >= a).all()


# ------------------------------------------------------------------ a double loop
def loops(a, kind, r, within, op, other=None, epilogue=None):
    H, W = a.shape
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            vals = [int(a[y + dy, x + dx]) for dy, dx in ref.offsets(kind, r)
                    if 0 <= y + dy < H and 0 <= x + dx < W and (within is None or within[y + dy, x + dx] != 0)]
            if op == 'erode':
                v = min(vals) if vals else 255
            elif op == 'dilate':
                v = max(vals) if vals else 0
            else:
                v = max(vals) - min(vals) if vals else 0
            if epilogue == 'other_minus':
                v = max(0, int(other[y, x]) - v)
            elif epilogue == 'minus_other':
                v = max(0, v - int(other[y, x]))
            out[y, x] = v
    return out


@pytest.mark.parametrize('kind', KINDS)
def test_against_a_double_loop(kind):
    rng = np.random.RandomState(3)
    for (H, W), r in (((1, 1), 0), ((1, 1), 3), ((1, 9), 2), ((9, 1), 2), ((7, 11), 1), ((7, 11), 3), ((6, 5), 9), ((13, 12), 4)):
        a = random_image(H, W, 1)
        other = random_image(H, W, 2)
        for within in (None, rng.rand(H, W) < 0.5, np.zeros((H, W), np.int32), (rng.rand(H, W) < 0.7) * np.int64(2 ** 40)):
            for op in ('erode', 'dilate', 'gradient'):
                assert np.array_equal(ref.flat_morphology(a, kind, r, op, within), loops(a, kind, r, within, op)), (H, W, r, op)
                for ep in ('other_minus', 'minus_other'):
                    assert np.array_equal(ref.flat_morphology(a, kind, r, op, within, other, ep),
                                          loops(a, kind, r, within, op, other, ep)), (H, W, r, op, ep)


def test_nothing_counted_gives_the_neutral_values():
    a = random_image(6, 7)
    none = np.zeros((6, 7), bool)
    for kind in KINDS:
        assert (ref.erode(a, 2, kind, none) == 255).all() and (ref.dilate(a, 2, kind, none) == 0).all()
        assert (ref.morph_gradient(a, 2, kind, none) == 0).all()
        assert (ref.erode(a > 100, 2, kind, none)).all() and not ref.dilate(a > 100, 2, kind, none).any()


# ------------------------------------------------------------------ closed forms
@pytest.mark.parametrize('kind', KINDS)
def test_a_single_pixel_becomes_the_footprint(kind):
    for r in (0, 1, 3, 6):
        f = ref.footprint(kind, r)
        a = np.zeros((2 * r + 5, 2 * r + 7), np.uint8)
        a[r + 2, r + 3] = 200
        want = np.zeros_like(a)
        want[2:2 * r + 3, 3:2 * r + 4] = 200 * f
        assert np.array_equal(ref.dilate(a, r, kind), want)
        assert np.array_equal(ref.erode(255 - a, r, kind), 255 - want)
        assert np.array_equal(ref.morph_gradient(a, r, kind), want if r else 0 * want)     # r = 0: max = min
        assert np.array_equal(ref.dilate(a != 0, r, kind), want != 0) and ref.dilate(a != 0, r, kind).dtype == bool
    # at a corner the footprint is clipped, not wrapped or reflected
    a = np.zeros((6, 6), np.uint8)
    a[0, 0] = 9
    want = np.zeros((6, 6), np.uint8)
    want[:3, :3] = 9 * ref.footprint(kind, 2)[2:, 2:]
    assert np.array_equal(ref.dilate(a, 2, kind), want)


def test_a_square_larger_than_the_image_gives_the_global_extremum():
    for H, W in ((1, 1), (5, 9), (12, 7)):
        a = random_image(H, W, 7)
        r = max(H, W)
        assert (ref.erode(a, r, 'square') == a.min()).all() and (ref.dilate(a, r, 'square') == a.max()).all()
        assert (ref.morph_gradient(a, r, 'square') == int(a.max()) - int(a.min())).all()


def test_order_and_duality():
    a = random_image(20, 27, 9)
    w = np.random.RandomState(4).rand(20, 27) < 0.8
    for kind in KINDS:
        for r in (1, 2, 4):
            assert np.array_equal(ref.dilate(a, r, kind), 255 - ref.erode(255 - a, r, kind))
            assert np.array_equal(ref.dilate(a, r, kind, w), 255 - ref.erode(255 - a, r, kind, w))
            o, c = ref.opening(a, r, kind), ref.closing(a, r, kind)
            assert (o <= a).all() and (a <= c).all()
            assert np.array_equal(ref.opening(o, r, kind), o) and np.array_equal(ref.closing(c, r, kind), c)
            assert np.array_equal(ref.white_tophat(a, r, kind), a - o) and np.array_equal(ref.black_tophat(a, r, kind), c - a)
            assert np.array_equal(ref.morph_gradient(a, r, kind).astype(int),
                                  ref.dilate(a, r, kind).astype(int) - ref.erode(a, r, kind).astype(int))
