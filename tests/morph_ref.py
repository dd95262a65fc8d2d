"""numpy restatement of kernels.KernelSpec.flat_morphology (csrc/morph.hip) and of the public functions on it, straight from the
definition: the offset list of the footprint, the image padded with the neutral value, the min / max over shifted views.  Pinned by
tests/test_morph_ref_cpu.py (scipy.ndimage, a double loop, literal footprints, closed forms)."""
import numpy as np

MAX_RADIUS = 63
KINDS = ('square', 'disk', 'diamond')


def width(kind, r, dy):
    """The half width w(dy) of footprint row dy, in integers."""
    assert kind in KINDS and abs(dy) <= r
    if kind == 'square':
        return r
    if kind == 'diamond':
        return r - abs(dy)
    w = 0
    while (w + 1) ** 2 + dy * dy <= r * r:
        w += 1
    return w


def offsets(kind, r):
    """Every (dy, dx) of the footprint."""
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-width(kind, r, dy), width(kind, r, dy) + 1)]


def footprint(kind, r):
    """The footprint as a (2 r + 1)^2 array of 0 / 1."""
    f = np.zeros((2 * r + 1, 2 * r + 1), np.uint8)
    for dy, dx in offsets(kind, r):
        f[dy + r, dx + r] = 1
    return f


def extrema(image, kind, r, within=None):
    """(lo, hi) as int64 arrays: the minimum and the maximum over the counted pixels of every clipped footprint, 255 and 0 where none
    is counted."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 2 and 0 <= r <= MAX_RADIUS
    H, W = image.shape
    counted = np.ones((H, W), bool) if within is None else np.asarray(within) != 0
    lo_src = np.full((H + 2 * r, W + 2 * r), 255, np.uint8)
    hi_src = np.zeros((H + 2 * r, W + 2 * r), np.uint8)
    lo_src[r:r + H, r:r + W] = np.where(counted, image, 255)
    hi_src[r:r + H, r:r + W] = np.where(counted, image, 0)
    lo, hi = np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8)
    for dy, dx in offsets(kind, r):
        lo = np.minimum(lo, lo_src[r + dy:r + dy + H, r + dx:r + dx + W])
        hi = np.maximum(hi, hi_src[r + dy:r + dy + H, r + dx:r + dx + W])
    lo, hi = lo.astype(np.int64), hi.astype(np.int64)
    return lo, hi


def flat_morphology(image, kind, r, op, within=None, other=None, epilogue=None):
    """The contract's result as uint8."""
    lo, hi = extrema(image, kind, r, within)
    res = {'erode': lo, 'dilate': hi, 'gradient': np.maximum(hi - lo, 0)}[op]       # nothing counted: 0 - 255 -> 0
    assert (other is None) == (epilogue is None)
    if epilogue == 'other_minus':
        res = np.maximum(np.asarray(other).astype(np.int64) - res, 0)
    elif epilogue == 'minus_other':
        res = np.maximum(res - np.asarray(other).astype(np.int64), 0)
    else:
        assert epilogue is None
    return res.astype(np.uint8)


def _u8(image):
    image = np.asarray(image)
    return image.astype(np.uint8) if image.dtype == bool else image


def _as(image, out):
    return out != 0 if np.asarray(image).dtype == bool else out


def erode(image, r, kind='disk', within=None):
    return _as(image, flat_morphology(_u8(image), kind, r, 'erode', within))


def dilate(image, r, kind='disk', within=None):
    return _as(image, flat_morphology(_u8(image), kind, r, 'dilate', within))


def opening(image, r, kind='disk', within=None):
    x = _u8(image)
    return _as(image, flat_morphology(flat_morphology(x, kind, r, 'erode', within), kind, r, 'dilate', within))


def closing(image, r, kind='disk', within=None):
    x = _u8(image)
    return _as(image, flat_morphology(flat_morphology(x, kind, r, 'dilate', within), kind, r, 'erode', within))


def white_tophat(image, r, kind='disk', within=None):
    x = _u8(image)
    return flat_morphology(flat_morphology(x, kind, r, 'erode', within), kind, r, 'dilate', within, x, 'other_minus')


def black_tophat(image, r, kind='disk', within=None):
    x = _u8(image)
    return flat_morphology(flat_morphology(x, kind, r, 'dilate', within), kind, r, 'erode', within, x, 'minus_other')


def morph_gradient(image, r, kind='disk', within=None):
    return flat_morphology(_u8(image), kind, r, 'gradient', within)
