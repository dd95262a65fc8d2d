"""numpy restatement of kernels.KernelSpec.window_sums / local_threshold (csrc/window.hip): the sums of every clipped window by int64
cumulative sums, and the rule in the sign cases of the contract.  Pinned by tests/test_window_ref_cpu.py (brute-force loops,
``fractions.Fraction`` evaluation of v > m + k s + c, closed forms)."""
import numpy as np

MAX_RADIUS = 127


def _box(a, r):
    """Sum of the int64 array a over rows y - r .. y + r and columns x - r .. x + r, clipped to the array."""
    H, W = a.shape
    t = np.zeros((H + 1, W + 1), np.int64)
    t[1:, 1:] = a.cumsum(0).cumsum(1)
    y, x = np.arange(H), np.arange(W)
    y0, y1 = np.maximum(y - r, 0)[:, None], np.minimum(y + r, H - 1)[:, None] + 1
    x0, x1 = np.maximum(x - r, 0)[None, :], np.minimum(x + r, W - 1)[None, :] + 1
    return t[y1, x1] - t[y0, x1] - t[y1, x0] + t[y0, x0]


def window_sums(image, radius, within=None):
    """(n, S, Q) as int64 arrays: the number, the sum and the sum of squares of the counted pixels of every window."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 2 and 0 <= radius <= MAX_RADIUS
    sel = np.ones(image.shape, np.int64) if within is None else (np.asarray(within) != 0).astype(np.int64)
    v = image.astype(np.int64) * sel
    return _box(sel, radius), _box(v, radius), _box(v * v, radius)


def decide(v, n, S, Q, k64, offset, floor):
    """The rule on int64 arrays: v > S / n + (k64 / 64) sqrt(Q / n - (S / n)^2) + offset, v > floor, n >= 1."""
    assert -128 <= k64 <= 128 and -255 <= offset <= 255 and -1 <= floor <= 255
    v, n, S, Q = (np.asarray(a, np.int64) for a in (v, n, S, Q))
    L = 64 * (n * v - S - offset * n)
    D = n * Q - S * S
    L2, k2D = L * L, (k64 * k64) * D
    if k64 >= 0:
        fg = (L > 0) & (L2 > k2D)
    else:
        fg = (L > 0) | ((L == 0) & (D > 0)) | ((L < 0) & (L2 < k2D))
    return fg & (v > floor) & (n >= 1)


def local_threshold(image, radius, k64, offset, floor, within=None):
    """bool [H, W]; floor = -1: no floor."""
    n, S, Q = window_sums(image, radius, within)
    return decide(np.asarray(image).astype(np.int64), n, S, Q, k64, offset, floor)


def otsu(image):
    """Otsu's threshold as nuclei._otsu states it, in Python integers."""
    h = np.bincount(np.asarray(image).reshape(-1), minlength=256).tolist()
    N, S = sum(h), sum(v * c for v, c in enumerate(h))
    best, bn, bd, w0, s0 = None, 0, 1, 0, 0
    for t in range(255):
        w0 += h[t]
        s0 += t * h[t]
        if 0 < w0 < N:
            num, den = (w0 * S - N * s0) ** 2, w0 * (N - w0)
            if best is None or num * bd > bn * den:
                best, bn, bd = t, num, den
    return best if best is not None else (max(v for v, c in enumerate(h) if c) if N else 0)


def ramp_discs(size=256, grid=8, disc_radius=6, lo=20, hi=140, contrast=50):
    """The example of a varying background: columns ramp from lo to hi, a grid x grid lattice of discs sits `contrast` above it.
    Returns (plane uint8 [size, size], disc int32 [size, size]: 0 background, 1 .. grid^2 the discs)."""
    x = np.arange(size)
    plane = np.broadcast_to(lo + ((hi - lo) * x) // (size - 1), (size, size)).astype(np.int64).copy()
    disc = np.zeros((size, size), np.int32)
    step = size // grid
    yy, xx = np.mgrid[:size, :size]
    for i in range(grid):
        for j in range(grid):
            cy, cx = step // 2 + i * step, step // 2 + j * step
            disc[(yy - cy) ** 2 + (xx - cx) ** 2 <= disc_radius ** 2] = 1 + i * grid + j
    plane[disc > 0] += contrast
    assert plane.max() <= 255
    return plane.astype(np.uint8), disc
