"""Reference for the stain front end (csrc/stain.hip, csrc/smooth.hip; cgc_net_amd.nuclei.separate_stains, histogram, otsu_threshold,
smooth, stain_foreground): the contracts of kernels.KernelSpec.stain_separate / histogram_u8 / binomial_smooth restated in numpy int64
and Python integers, with no knowledge of how the kernels work.  A plain module: no pytest hooks, no fixtures."""
import functools
import math
from fractions import Fraction

import numpy as np

OD_MAX = 5674
DEFAULT_STAINS = ((0.65, 0.70, 0.29), (0.07, 0.99, 0.11), (0.27, 0.57, 0.78))      # haematoxylin, eosin, residual (R, G, B)


def od_lut():
    """floor(1024 ln(255 / max(v, 1)) + 0.5) for v = 0..255, as int64."""
    return np.array([math.floor(1024.0 * math.log(255.0 / max(v, 1)) + 0.5) for v in range(256)], np.int64)


def stain_matrix(stains=DEFAULT_STAINS):
    """rint(4096 inv(S)) as int64 [3, 3] (row = channel R, G, B; column = stain), S = the row-normalised stain vectors."""
    S = np.array(stains, np.float64)
    S = S / np.sqrt((S * S).sum(axis=1))[:, None]
    return np.rint(4096.0 * np.linalg.inv(S)).astype(np.int64)


def separate(pix, M, order=0, planes=(0, 1, 2)):
    """pix uint8 [..., 3] (order 0: B, G, R; 1: R, G, B), M int [3, 3] -> uint8 [len(planes), ...]."""
    pix = np.asarray(pix)
    rgb = pix[..., ::-1] if order == 0 else pix
    od = od_lut()[rgb.astype(np.int64)]                       # [..., 3]
    C = od @ np.asarray(M, np.int64)                          # [..., 3]: C_s = sum_c od_c M[c][s]
    assert np.abs(C).max(initial=0) < 2 ** 31 - 2 ** 15
    level = np.clip((C + 2 ** 15) >> 16, 0, 255).astype(np.uint8)
    return np.stack([level[..., s] for s in planes]) if len(planes) else np.zeros((0,) + pix.shape[:-1], np.uint8)


def separate_float(pix, stains=DEFAULT_STAINS, order=0):
    """The float64 formula: clip(64 ln(255 / max(v, 1)) @ inv(S), 0, 255) -> float64 [3, ...]."""
    pix = np.asarray(pix)
    rgb = (pix[..., ::-1] if order == 0 else pix).astype(np.float64)
    S = np.array(stains, np.float64)
    S = S / np.sqrt((S * S).sum(axis=1))[:, None]
    C = 64.0 * np.log(255.0 / np.maximum(rgb, 1.0)) @ np.linalg.inv(S)
    return np.moveaxis(np.clip(C, 0.0, 255.0), -1, 0)


def histogram(img, within=None):
    img = np.asarray(img)
    sel = img.reshape(-1) if within is None else img.reshape(-1)[np.asarray(within).reshape(-1) != 0]
    return np.bincount(sel.astype(np.int64), minlength=256).astype(np.int64)


def otsu(hist):
    """The t in 0..254 with 0 < w0 < N that maximises (w0 S - N s0)^2 / (w0 (N - w0)) as an exact Fraction; the smallest of equal
    ones; the one value of a one-valued selection; 0 for an empty one."""
    h = [int(c) for c in hist]
    N = sum(h)
    if N == 0:
        return 0
    S = sum(v * c for v, c in enumerate(h))
    scores = []
    for t in range(255):
        w0 = sum(h[:t + 1])
        s0 = sum(v * h[v] for v in range(t + 1))
        if 0 < w0 < N:
            scores.append((Fraction((w0 * S - N * s0) ** 2, w0 * (N - w0)), -t))
    if not scores:
        return [v for v, c in enumerate(h) if c][0]
    return -max(scores)[1]


def binomial_smooth(img, radius):
    """Both passes in int64 with replicated borders, then the single rounding."""
    img = np.asarray(img)
    r = int(radius)
    w = [math.comb(2 * r, k) for k in range(2 * r + 1)]
    H, W = img.shape
    if H * W == 0:
        return img.copy()
    a = img.astype(np.int64)
    ys = np.clip(np.arange(H)[:, None] + np.arange(-r, r + 1)[None, :], 0, H - 1)      # [H, 2r + 1]
    xs = np.clip(np.arange(W)[:, None] + np.arange(-r, r + 1)[None, :], 0, W - 1)
    wv = np.array(w, np.int64)
    a = (a[:, xs] * wv).sum(axis=2)                           # rows: [H, W, 2r + 1] -> [H, W]
    a = (a[ys, :] * wv[None, :, None]).sum(axis=1)            # columns: [H, 2r + 1, W] -> [H, W]
    if r > 0:
        a = (a + (1 << (4 * r - 1))) >> (4 * r)
    return a.astype(np.uint8)


def stain_foreground(pix, stain=0, radius=2, stains=DEFAULT_STAINS, order=0, within=None):
    plane = binomial_smooth(separate(pix, stain_matrix(stains), order, (stain,))[0], radius)
    t = otsu(histogram(plane, within))
    return plane > t, t, plane


def render_tile(labels, order=0, c_nucleus=1.5, c_background=0.2, c_eosin=0.6):
    """A noise-free H&E tile of an instance mask: uint8 [H, W, 3] = rint(255 exp(-(cH h + cE e))) with h, e the unit OD vectors of
    haematoxylin and eosin, cH = c_nucleus on labelled pixels and c_background elsewhere, cE constant."""
    S = np.array(DEFAULT_STAINS, np.float64)
    S = S / np.sqrt((S * S).sum(axis=1))[:, None]
    cH = np.where(np.asarray(labels) > 0, c_nucleus, c_background)[..., None]
    rgb = np.rint(255.0 * np.exp(-(cH * S[0] + c_eosin * S[1]))).astype(np.uint8)
    return np.ascontiguousarray(rgb[..., ::-1] if order == 0 else rgb)


@functools.lru_cache(maxsize=None)
def tile_case():
    """(labels int32 [192, 160], tile uint8 [192, 160, 3] BGR, within bool [192, 160]) -- computed once, never modified."""
    from cgc_net_amd import nuclei
    labels, _ = nuclei.synthetic_tissue(192, 160, 30, seed=3)
    tile = render_tile(labels)
    within = np.zeros(labels.shape, bool)
    within[10:170, 5:150] = True
    for a in (labels, tile, within):
        a.setflags(write=False)
    return labels, tile, within
