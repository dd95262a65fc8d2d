"""numpy restatement of kernels.KernelSpec.rank_filter (csrc/rank.hip) and of the public functions on it, straight from the
definition: for every level t the indicator image "counted and value <= t", its row prefix sums, and those summed over the rows of the
footprint -- the cumulative counts #{v <= t} of every window at all 256 levels at once.  Quantiles, the range and the bin counts of
the entropy are read off those counts.  The table of entropy terms is computed here with ``decimal``.  Nothing of the package is
used; the footprint widths are restated as in tests/morph_ref.py.  Pinned by tests/test_rank_ref_cpu.py (a sort-based double loop,
scipy.ndimage, morph_ref, literal cases, closed forms, float64 entropy)."""
import decimal

import numpy as np

MAX_RADIUS = 63
ENTROPY_MAX_RADIUS = 15
ENTROPY_TERMS = 962
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


def _terms():
    """T[c] = round(c * log2(c) * 2^16), c = 0..961, in 60-digit decimal arithmetic (no value lies near a half)."""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        ln2 = decimal.Decimal(2).ln()
        out = [0, 0]
        for c in range(2, ENTROPY_TERMS):
            x = decimal.Decimal(c) * (decimal.Decimal(c).ln() / ln2) * 65536
            out.append(int(x.to_integral_value(rounding=decimal.ROUND_HALF_EVEN)))
    return np.array(out, np.int64)


TERMS = _terms()


def cumulative(image, kind, r, within=None):
    """int64 [256, H, W]: entry [t, y, x] is the number of counted pixels of the clipped footprint at (y, x) whose value is <= t.
    Entry [255] is n."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 2 and 0 <= r <= MAX_RADIUS
    H, W = image.shape
    counted = np.ones((H, W), bool) if within is None else np.asarray(within) != 0
    assert counted.shape == (H, W)
    below = (image[None] <= np.arange(256, dtype=np.int64)[:, None, None]) & counted[None]
    # row prefix sums, padded so that every read below is a slice: column r + j holds P[j] = #{x < j}, the columns left of it 0 and
    # the columns right of r + W the row's total; rows outside the image hold nothing
    prefix = np.zeros((256, H + 2 * r, W + 1 + 2 * r), np.int32)
    if W:
        inner = np.cumsum(below, axis=2, dtype=np.int32)
        prefix[:, r:r + H, r + 1:r + 1 + W] = inner
        prefix[:, r:r + H, r + 1 + W:] = inner[:, :, -1:]
    cum = np.zeros((256, H, W), np.int64)
    for dy in range(-r, r + 1):
        w = width(kind, r, dy)                                          # columns x - w .. x + w: P[min(x + w + 1, W)] - P[max(x - w, 0)]
        rows = prefix[:, r + dy:r + dy + H, :]
        cum += rows[:, :, r + w + 1:r + w + 1 + W] - rows[:, :, r - w:r - w + W]
    return cum


def rank_index(n, q10k):
    """k = min(n - 1, floor(n * q10k / 10000)); -1 where n = 0."""
    assert isinstance(q10k, int) and 0 <= q10k <= 10000
    return np.minimum(n - 1, n * q10k // 10000)


def quantile_of(cum, q10k):
    """v[k] from the cumulative counts: the smallest t with cum[t] > k = the number of levels with cum[t] <= k; 0 where n = 0."""
    k = rank_index(cum[255], q10k)
    return (cum <= k[None]).sum(axis=0).astype(np.int64) if cum.shape[1] * cum.shape[2] else np.zeros(cum.shape[1:], np.int64)


def entropy_of(cum):
    """(E, n, occupied bins) of every window as int64: E = T[n] - sum over the non-empty bins of T[count]."""
    counts = np.diff(cum, axis=0, prepend=0)
    n = cum[255]
    assert counts.min(initial=0) >= 0 and n.max(initial=0) < ENTROPY_TERMS
    return TERMS[n] - TERMS[counts].sum(axis=0), n, (counts > 0).sum(axis=0)


def h16_of(cum):
    E, n, _ = entropy_of(cum)
    return np.where(n > 0, E // np.maximum(n, 1), 0).astype(np.int32)


def rank_filter_u8(image, kind, r, op, q_lo=0, q_hi=0, within=None):
    """The contract's result: uint8 for 'quantile' and 'range', int32 for 'entropy'."""
    assert 0 <= q_lo <= q_hi <= 10000
    cum = cumulative(image, kind, r, within)
    if op == 'quantile':
        return quantile_of(cum, q_hi).astype(np.uint8)
    if op == 'range':
        return (quantile_of(cum, q_hi) - quantile_of(cum, q_lo)).astype(np.uint8)
    assert op == 'entropy' and r <= ENTROPY_MAX_RADIUS
    return h16_of(cum)


def _u8(image):
    image = np.asarray(image)
    return image.astype(np.uint8) if image.dtype == bool else image


def _as(image, out):
    return out != 0 if np.asarray(image).dtype == bool else out


def rank_filter(image, r, q10k, kind='disk', within=None):
    return _as(image, rank_filter_u8(_u8(image), kind, r, 'quantile', 0, q10k, within))


def median(image, r, kind='disk', within=None):
    return rank_filter(image, r, 5000, kind, within)


def quantile_range(image, r, lo10k, hi10k, kind='disk', within=None):
    return rank_filter_u8(_u8(image), kind, r, 'range', lo10k, hi10k, within)


def local_entropy_raw(image, r=3, kind='disk', within=None):
    return rank_filter_u8(_u8(image), kind, r, 'entropy', within=within)
