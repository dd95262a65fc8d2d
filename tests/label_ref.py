"""The oracle of cgc_net_amd.nuclei.label_instances: numpy + scipy, written for the tests (tests/test_label_ref_cpu.py pins it to a
brute-force flood fill).  A binary image goes to scipy.ndimage.label directly; an integer image is labelled value by value and the
union renumbered by first raster index; min_size is applied with numpy.bincount before the renumbering."""
import numpy as np
from scipy import ndimage

STRUCTURES = {1: ndimage.generate_binary_structure(2, 1), 2: ndimage.generate_binary_structure(2, 2)}


def renumber_by_first_pixel(lab):
    """Positive labels of ``lab`` -> 1..n in the raster order of each label's first pixel; 0 stays 0."""
    flat = lab.ravel()
    vals, first = np.unique(flat, return_index=True)
    keep = vals > 0
    vals, first = vals[keep], first[keep]
    order = np.argsort(first, kind='stable')
    table = np.zeros(int(flat.max()) + 1 if flat.size else 1, np.int64)
    table[vals[order]] = np.arange(1, vals.size + 1)
    return table[np.maximum(lab, 0)].astype(np.int32), int(vals.size)


def label(image, connectivity=1, min_size=0):
    """(labels int32 [H, W], n, sizes int32 [n]) of the contract of label_instances."""
    image = np.asarray(image)
    assert image.ndim == 2 and connectivity in (1, 2) and min_size >= 0
    if image.size == 0:
        return np.zeros(image.shape, np.int32), 0, np.zeros(0, np.int32)
    st = STRUCTURES[connectivity]
    values = np.unique(image)
    values = values[values != 0]
    if image.dtype == np.bool_ or values.size <= 1:
        lab, n = ndimage.label(image != 0, structure=st)
        lab = lab.astype(np.int64)
    else:
        lab, n = np.zeros(image.shape, np.int64), 0
        for v in values:
            part, k = ndimage.label(image == v, structure=st)
            lab[part > 0] = part[part > 0] + n
            n += k
    if min_size > 0:
        counts = np.bincount(lab.ravel(), minlength=n + 1)
        small = counts < min_size
        small[0] = False
        lab[small[lab]] = 0
    lab, n = renumber_by_first_pixel(lab)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:].astype(np.int32)
    return lab, n, sizes


def flood_fill(image, connectivity=1):
    """Brute force, for small images: scan in raster order, flood every unlabelled foreground pixel over equal-valued neighbours."""
    image = np.asarray(image)
    H, W = image.shape
    nbrs = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 2 else [])
    lab = np.zeros((H, W), np.int32)
    n = 0
    for y in range(H):
        for x in range(W):
            if image[y, x] == 0 or lab[y, x]:
                continue
            n += 1
            lab[y, x] = n
            stack = [(y, x)]
            while stack:
                cy, cx = stack.pop()
                for dy, dx in nbrs:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < H and 0 <= nx < W and not lab[ny, nx] and image[ny, nx] == image[y, x]:
                        lab[ny, nx] = n
                        stack.append((ny, nx))
    return lab, n
