"""The oracle of cgc_net_amd.nuclei.reconstruct / h_maxima / regional_maxima / fill_holes / split_touching(markers='h_maxima'): numpy +
scipy, written from the definition for the tests and sharing no code with the kernel (tests/test_reconstruct_ref_cpu.py pins it to
scipy's binary propagation and hole filling, to a brute-force max-min path closure and to an independent plateau labelling).

Reconstruction by dilation iterates R = min(mask, grey_dilation(R)) from min(marker, mask) until nothing changes, in int64 so that no
int32 value is special; by erosion it is ~dilation(~marker, ~mask)."""
import math

import numpy as np
from scipy import ndimage

import edt_ref
import geodesic_ref
import label_ref

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
FOOTPRINTS = {1: ndimage.generate_binary_structure(2, 1), 2: ndimage.generate_binary_structure(2, 2)}


def as_int(a):
    a = np.asarray(a)
    return a.astype(np.int64)           # bool -> 0 / 1


def reconstruct(marker, mask, method='dilation', connectivity=1):
    """int64 [H, W]: the reconstruction of the contract of nuclei.reconstruct (the caller casts to the marker's dtype)."""
    assert method in ('dilation', 'erosion') and connectivity in (1, 2)
    marker, mask = as_int(marker), as_int(mask)
    assert marker.shape == mask.shape and marker.ndim == 2
    if method == 'erosion':
        return ~reconstruct(~marker, ~mask, 'dilation', connectivity)
    r = np.minimum(marker, mask)
    if r.size == 0:
        return r
    while True:
        grown = np.minimum(mask, ndimage.grey_dilation(r, footprint=FOOTPRINTS[connectivity], mode='nearest'))
        if np.array_equal(grown, r):
            return r
        r = grown


def brute_closure(marker, mask, connectivity=1):
    """The max-min path closure by its definition, for tiny images: R[p] = max over q and paths q -> p of min(R0[q], min of mask on the
    path), as a Floyd-Warshall closure of the bottleneck capacity min(mask[u], mask[v]) of every neighbour step."""
    marker, mask = as_int(marker), as_int(mask)
    H, W = mask.shape
    n = H * W
    low = -2 ** 40
    cap = np.full((n, n), low, np.int64)
    m = mask.ravel()
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 2 else [])
    for y in range(H):
        for x in range(W):
            p = y * W + x
            cap[p, p] = m[p]
            for dy, dx in steps:
                ny, nx = y + dy, x + dx
                if 0 <= ny < H and 0 <= nx < W:
                    cap[p, ny * W + nx] = min(m[p], m[ny * W + nx])
    for k in range(n):
        cap = np.maximum(cap, np.minimum(cap[:, k:k + 1], cap[k:k + 1, :]))
    r0 = np.minimum(marker, mask).ravel()
    return np.max(np.minimum(r0[:, None], cap), axis=0).reshape(H, W)


def h_maxima(image, h, connectivity=1):
    """bool [H, W]: (image - reconstruct(image - h saturated at INT32_MIN, image)) >= h."""
    image = as_int(image)
    assert 1 <= h <= INT32_MAX
    marker = np.maximum(image - h, INT32_MIN)
    return image - reconstruct(marker, image, 'dilation', connectivity) >= h


def regional_maxima(image, connectivity=1):
    return h_maxima(image, 1, connectivity)


def plateau_maxima(image, connectivity=1):
    """Independent of reconstruction: label the plateaus level by level; one qualifies if none of its pixels has a higher neighbour."""
    image = as_int(image)
    out = np.zeros(image.shape, bool)
    if image.size == 0:
        return out
    higher = ndimage.maximum_filter(image, footprint=FOOTPRINTS[connectivity], mode='nearest') > image
    for level in np.unique(image):
        lab, n = ndimage.label(image == level, structure=FOOTPRINTS[connectivity])
        if n:
            bad = np.unique(lab[higher & (lab > 0)])
            out |= (lab > 0) & ~np.isin(lab, bad)
    return out


def holes_of(image, connectivity=1):
    """bool [H, W]: the ``connectivity``-components of {image == 0} that do not touch the image border."""
    bg = np.asarray(image) == 0
    if bg.size == 0:
        return bg
    border = np.zeros_like(bg)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    outside = reconstruct(bg & border, bg, 'dilation', connectivity) != 0
    return bg & ~outside


def fill_holes(image, connectivity=1):
    image = np.asarray(image)
    holes = holes_of(image, connectivity)
    if image.dtype == np.bool_:
        return image | holes
    if image.size == 0:
        return image.copy()
    return geodesic_ref.expand_labels_geodesic(image, None, within=holes, connectivity=connectivity)


def eighths(dist2):
    """int32 [H, W]: T = isqrt(64 dist2), the distance in eighths of a pixel, by Python's integer square root."""
    d = np.asarray(dist2)
    return np.array([math.isqrt(64 * int(v)) for v in d.ravel()], np.int64).reshape(d.shape).astype(np.int32)


def h8_of(h):
    """The largest integer with h8 / 8 <= h."""
    k = int(math.floor(h * 8)) + 2
    while k / 8 > h:
        k -= 1
    return k


def split_touching_h_maxima(mask, h, connectivity=1, min_size=0):
    """split_touching(mask, None, connectivity, min_size, growth='geodesic', markers='h_maxima', h=h) on the oracles."""
    fg = np.asarray(mask) != 0
    d2 = edt_ref.dist2_scipy(~fg)
    seeds = h_maxima(eighths(d2), h8_of(h), connectivity) & fg
    cores, k, _ = label_ref.label(seeds, connectivity)
    grown = geodesic_ref.expand_labels_geodesic(cores, None, within=fg, connectivity=connectivity)
    rest, _, _ = label_ref.label(fg & (grown == 0), connectivity)
    combined = np.where(rest > 0, rest + k, grown)
    lab, n, _ = label_ref.label(combined, connectivity, min_size)
    return lab, n
