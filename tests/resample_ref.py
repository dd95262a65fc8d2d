"""A restatement of the resampling contract (kernels.KernelSpec.resample_u8 / resample_labels, items 2 to 7) in Python integers and
numpy int64, for the tests.  It shares no code with the package.  Everything is separable: per-axis tables, then two passes, so a
32767-wide row is instant.  A plain module: no pytest hooks, no fixtures."""
import numpy as np


def linear_axis(n, m):
    """Item 2: per output index (i0, i1, f), f over 2 m."""
    d = np.arange(m, dtype=np.int64)
    num = np.clip((2 * d + 1) * n - m, 0, 2 * m * (n - 1))
    i0 = num // (2 * m)
    return i0, np.minimum(i0 + 1, n - 1), num - i0 * 2 * m


def linear(img, size):
    """Item 3 on [H, W]: one rounding, half up."""
    H, W = img.shape
    H2, W2 = size
    p = img.astype(np.int64)
    y0, y1, fy = linear_axis(H, H2)
    x0, x1, fx = linear_axis(W, W2)
    rows = p[:, x0] * (2 * W2 - fx) + p[:, x1] * fx                              # [H, W2]
    S = rows[y0] * (2 * H2 - fy)[:, None] + rows[y1] * fy[:, None]
    D = 4 * H2 * W2
    return ((2 * S + D) // (2 * D)).astype(np.uint8)


def box_integral(p, n, m, axis):
    """Item 4 along one axis: out[d] = sum_i p[i] o_i = F((d + 1) n) - F(d n), where F(t) is the integral of the step function p
    over [0, t) in units of 1 / m of a pixel: F(t) = m * (p[0] + .. + p[i - 1]) + (t - i m) p[i], i = floor(t / m)."""
    p = np.moveaxis(p.astype(np.int64), axis, 0)
    shape = (1,) + p.shape[1:]
    prefix = np.concatenate([np.zeros(shape, np.int64), np.cumsum(p, axis=0)])      # [n + 1, ...]
    padded = np.concatenate([p, np.zeros(shape, np.int64)])                        # p[n] = 0
    t = np.arange(m + 1, dtype=np.int64) * n
    i = t // m
    part = (t - i * m).reshape((-1,) + (1,) * (p.ndim - 1))
    F = m * prefix[i] + part * padded[i]
    return np.moveaxis(F[1:] - F[:-1], 0, axis)


def area(img, size):
    """Item 4 on [H, W]."""
    H, W = img.shape
    H2, W2 = size
    assert H2 <= H and W2 <= W
    S = box_integral(box_integral(img, W, W2, 1), H, H2, 0)
    D = H * W
    return ((2 * S + D) // (2 * D)).astype(np.uint8)


def resize(img, size, mode):
    """Items 3 to 5: a plane or an interleaved tile."""
    f = {'linear': linear, 'area': area}[mode]
    if img.ndim == 2:
        return f(img, size)
    return np.stack([f(img[:, :, c], size) for c in range(img.shape[2])], axis=2)


def nearest_axis(n, m):
    d = np.arange(m, dtype=np.int64)
    return (2 * d + 1) * n // (2 * m)


def nearest(lab, size):
    """Item 6."""
    return lab[nearest_axis(lab.shape[0], size[0])][:, nearest_axis(lab.shape[1], size[1])]


def box_weights(d, n, m):
    """Item 4: the pixels i of output index d's box and their weights o_i."""
    lo, hi = d * n // m, ((d + 1) * n - 1) // m
    i = np.arange(lo, hi + 1, dtype=np.int64)
    o = np.minimum((d + 1) * n, (i + 1) * m) - np.maximum(d * n, i * m)
    assert (o > 0).all() and o.sum() == n
    return i, o


def majority(lab, size):
    """Item 7: the value of the largest total weight, ties to the smallest value (bool as 0 / 1)."""
    H, W = lab.shape
    H2, W2 = size
    assert H2 <= H <= 8 * H2 and W2 <= W <= 8 * W2
    src = lab.astype(np.uint8) if lab.dtype == np.bool_ else lab
    out = np.empty((H2, W2), src.dtype)
    cols = [box_weights(x, W, W2) for x in range(W2)]
    for y in range(H2):
        iy, oy = box_weights(y, H, H2)
        for x in range(W2):
            ix, ox = cols[x]
            assert len(iy) <= 9 and len(ix) <= 9
            values, inverse = np.unique(src[np.ix_(iy, ix)], return_inverse=True)      # ascending, signed for signed dtypes
            weight = np.zeros(len(values), np.int64)
            np.add.at(weight, inverse.ravel(), np.outer(oy, ox).ravel())
            out[y, x] = values[int(np.argmax(weight))]                                 # the first of equal maxima: the smallest value
    return out.astype(lab.dtype)


def resize_labels(lab, size, mode):
    return {'nearest': nearest, 'majority': majority}[mode](lab, size)


def scaled_side(n, f):
    """max(1, floor(n f + 1/2)) for a Fraction f."""
    from fractions import Fraction
    v = n * Fraction(f) + Fraction(1, 2)
    return max(1, v.numerator // v.denominator)
