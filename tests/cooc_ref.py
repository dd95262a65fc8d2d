"""A numpy restatement of the region co-occurrence tables (kernels.KernelSpec.region_cooccurrence) and of the Haralick properties
read off them (nuclei.cooccurrence_properties), written from the definition: shifted slices of the label, level and within planes and
``np.add.at`` in int64.  It shares no code with the package; tests/test_cooc_ref_cpu.py pins it against loops and hand-written cases.
A plain module: no pytest hooks, no fixtures."""
import numpy as np

MAX_OFFSET = 16
MAX_OFFSETS = 8
MAX_LEVELS = 16
DIRECTIONS = ((0, 1), (1, 1), (1, 0), (1, -1))
PROPERTIES = ('contrast', 'dissimilarity', 'homogeneity', 'ASM', 'energy', 'correlation', 'entropy')


def level_lut(levels, lo=0, hi=255):
    """256 levels: 0 up to lo, levels - 1 from hi on, floor((v - lo) levels / (hi - lo + 1)) between."""
    out = []
    for v in range(256):
        if v <= lo:
            out.append(0)
        elif v >= hi:
            out.append(levels - 1)
        else:
            out.append(((v - lo) * levels) // (hi - lo + 1))
    return out


def _anchor_and_partner(plane, dy, dx):
    """The two views of ``plane`` that hold p and p + (dy, dx) for every p at which both lie inside; empty if there is none."""
    H, W = plane.shape
    if abs(dy) >= H or abs(dx) >= W:
        return plane[:0, :0], plane[:0, :0]
    ya, yb = (0, H - dy) if dy >= 0 else (-dy, H)
    xa, xb = (0, W - dx) if dx >= 0 else (-dx, W)
    return plane[ya:yb, xa:xb], plane[ya + dy:yb + dy, xa + dx:xb + dx]


def tables(labels, values, offsets, levels, lut=None, symmetric=True, max_label=None, within=None):
    """int64 [max_label + 1, len(offsets), levels, levels]."""
    labels = np.asarray(labels).astype(np.int64)
    lut = np.asarray(level_lut(levels) if lut is None else lut, dtype=np.int64)
    assert lut.shape == (256,) and lut.min() >= 0 and lut.max() < levels
    level = lut[np.asarray(values).astype(np.uint8)]
    if max_label is None:
        max_label = int(labels.max()) if labels.size else 0
    ok = (labels >= 0) & (labels <= max_label)
    if within is not None:
        ok &= np.asarray(within) != 0
    out = np.zeros((max_label + 1, len(offsets), levels, levels), np.int64)
    for k, (dy, dx) in enumerate(offsets):
        lp, lq = _anchor_and_partner(labels, dy, dx)
        op, oq = _anchor_and_partner(ok, dy, dx)
        vp, vq = _anchor_and_partner(level, dy, dx)
        pair = op & oq & (lp == lq)
        np.add.at(out, (lp[pair], k, vp[pair], vq[pair]), 1)
        if symmetric:
            np.add.at(out, (lp[pair], k, vq[pair], vp[pair]), 1)
    return out


def refused(labels, max_label):
    labels = np.asarray(labels).astype(np.int64)
    return int(((labels < 0) | (labels > max_label)).sum())


def properties(tables):
    """float64 [R, K, 7] in the order of PROPERTIES, from integer tables [R, K, levels, levels]."""
    c = np.asarray(tables).astype(np.float64)
    R, K, lv, _ = c.shape
    n = c.sum(axis=(2, 3))
    p = c / np.where(n > 0, n, 1.0)[:, :, None, None]
    i, j = np.meshgrid(np.arange(lv, dtype=np.float64), np.arange(lv, dtype=np.float64), indexing='ij')
    out = np.zeros((R, K, len(PROPERTIES)))
    out[:, :, 0] = (p * (i - j) ** 2).sum(axis=(2, 3))
    out[:, :, 1] = (p * np.abs(i - j)).sum(axis=(2, 3))
    out[:, :, 2] = (p / (1.0 + (i - j) ** 2)).sum(axis=(2, 3))
    out[:, :, 3] = (p * p).sum(axis=(2, 3))
    out[:, :, 4] = np.sqrt(out[:, :, 3])
    mu_i = (p * i).sum(axis=(2, 3))[:, :, None, None]
    mu_j = (p * j).sum(axis=(2, 3))[:, :, None, None]
    var_i = (p * (i - mu_i) ** 2).sum(axis=(2, 3))
    var_j = (p * (j - mu_j) ** 2).sum(axis=(2, 3))
    cov = (p * (i - mu_i) * (j - mu_j)).sum(axis=(2, 3))
    ints = np.asarray(tables).astype(np.int64)
    single = ((ints.sum(axis=3) != 0).sum(axis=2) <= 1) | ((ints.sum(axis=2) != 0).sum(axis=2) <= 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        out[:, :, 5] = np.where(single, 1.0, cov / np.sqrt(np.where(single, 1.0, var_i) * np.where(single, 1.0, var_j)))
        out[:, :, 6] = -np.where(p > 0, p * np.log2(np.where(p > 0, p, 1.0)), 0.0).sum(axis=(2, 3))
    out[n == 0] = 0.0
    return out
