"""A numpy restatement of the region geometry (csrc/region.hip; kernels.KernelSpec.region_geometry) and of the properties
cgc_net_amd.nuclei.region_shape reads off it, written from the definition: np.bincount and np.add.at in int64 for the pixel tables,
np.minimum.at / np.maximum.at for the extents, four shifted views of an image padded by one position that belongs to nobody for the
bit quads.  A plain module: no pytest hooks, no fixtures.  tests/test_shape_ref_cpu.py pins it against per-pixel loops,
scipy.ndimage, scipy.spatial and cases written out by hand."""
import math

import numpy as np

DIRECTIONS = ((1, 0), (2, 1), (1, 1), (1, 2), (0, 1), (-1, 2), (-1, 1), (-2, 1))      # (a, b) of a x + b y
QUADS = ('n1', 'n2', 'nd', 'n3')
NONE = -1
SHAPE_FLOATS = ('area', 'centroid_y', 'centroid_x', 'var_y', 'var_x', 'cov', 'major_axis', 'minor_axis', 'eccentricity', 'orientation',
                'bbox_fill', 'perimeter', 'circularity', 'equivalent_diameter', 'feret_max', 'feret_min', 'polygon_area', 'convexity16')
SHAPE_INTS = ('bbox', 'perimeter_crack', 'euler4', 'euler8', 'border')
FEATURES = ('area', 'major_axis', 'minor_axis', 'eccentricity', 'orientation', 'perimeter', 'circularity', 'convexity16', 'feret_max',
            'feret_min', 'bbox_fill', 'holes', 'touches_border')


def belongs(labels, max_label, within=None):
    """int64 [H, W]: the row a pixel belongs to, or NONE (a label outside [0, max_label], or ``within`` zero there)."""
    lab = np.asarray(labels).astype(np.int64)
    ok = (lab >= 0) & (lab <= max_label)
    if within is not None:
        ok &= np.asarray(within) != 0
    return np.where(ok, lab, NONE)


def refused(labels, max_label):
    lab = np.asarray(labels).astype(np.int64)
    return int(((lab < 0) | (lab > max_label)).sum())


def geometry(labels, max_label, within=None):
    """dict(count int32 [R], sy sx syy sxy sxx int64 [R], extents int32 [R, 8, 2], quads int32 [R, 4], border int32 [R])."""
    e = belongs(labels, max_label, within)
    H, W = e.shape
    R = max_label + 1
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    on = e != NONE
    l, y, x = e[on], yy[on], xx[on]
    out = dict(count=np.bincount(l, minlength=R).astype(np.int32))
    for name, v in (('sy', y), ('sx', x), ('syy', y * y), ('sxy', x * y), ('sxx', x * x)):
        out[name] = np.zeros(R, np.int64)
        np.add.at(out[name], l, v)
    big = np.iinfo(np.int64).max
    lo, hi = np.full((R, 8), big), np.full((R, 8), -big)
    for k, (a, b) in enumerate(DIRECTIONS):
        np.minimum.at(lo[:, k], l, a * x + b * y)
        np.maximum.at(hi[:, k], l, a * x + b * y)
    some = out['count'] > 0
    out['extents'] = np.where(some[:, None, None], np.stack([lo, hi], axis=2), 0).astype(np.int32)
    out['border'] = np.bincount(l[(y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)], minlength=R).astype(np.int32)
    # quads: top-left corners (-1 .. H-1) x (-1 .. W-1) of the padded image
    p = np.full((H + 2, W + 2), NONE, np.int64)
    p[1:H + 1, 1:W + 1] = e
    tl, tr, bl, br = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]
    quads = np.zeros((R, 4), np.int64)
    if H * W:
        corners = (tl, tr, bl, br)
        for i, c in enumerate(corners):                              # the row at corner i, unless an earlier corner has it already
            first = c != NONE
            for j in range(i):
                first &= corners[j] != c
            m = [(d == c) for d in corners]
            n = sum(mm.astype(np.int64) for mm in m)
            diagonal = (m[0] & m[3] & ~m[1] & ~m[2]) | (m[1] & m[2] & ~m[0] & ~m[3])
            cls = np.where(n == 1, 0, np.where(n == 3, 3, np.where(diagonal, 2, 1)))
            sel = first & (n < 4)
            np.add.at(quads, (c[sel], cls[sel]), 1)
    out['quads'] = quads.astype(np.int32)
    return out


def n4(g):
    """The quads that lie in the row entirely: (4 count - n1 - 2 n2 - 2 nd - 3 n3) / 4, which must divide."""
    q = g['quads'].astype(np.int64)
    rest = 4 * g['count'].astype(np.int64) - q[:, 0] - 2 * q[:, 1] - 2 * q[:, 2] - 3 * q[:, 3]
    assert (rest % 4 == 0).all() and (rest >= 0).all()
    return rest // 4


def shape(g, real=np.float64):
    """dict of region_shape's tables, evaluated in ``real`` (np.float64: what the device computes; np.longdouble: a yardstick) and left
    in it -- the caller rounds.  Integer tables are int64.  The formulas are those of the function's docstring, in its order."""
    f = real
    ni = g['count'].astype(np.int64)
    some = ni > 0
    n = np.where(some, ni, 1).astype(f)
    ext = g['extents'].astype(np.int64)
    x0, x1, y0, y1 = ext[:, 0, 0], ext[:, 0, 1], ext[:, 4, 0], ext[:, 4, 1]
    sy, sx, syy, sxy, sxx = (g[k].astype(np.int64) for k in ('sy', 'sx', 'syy', 'sxy', 'sxx'))
    su, sv = sx - ni * x0, sy - ni * y0
    suu = sxx - 2 * x0 * sx + ni * x0 * x0
    svv = syy - 2 * y0 * sy + ni * y0 * y0
    suv = sxy - x0 * sy - y0 * sx + ni * x0 * y0
    su, sv, suu, svv, suv = (t.astype(f) for t in (su, sv, suu, svv, suv))
    nn = n * n
    A, B, C = n * suu - su * su, n * svv - sv * sv, n * suv - su * sv
    D = np.sqrt((A - B) * (A - B) + f(4) * (C * C))
    top = A + B + D
    l1, l2 = top / (f(2) * nn), np.maximum(A + B - D, f(0)) / (f(2) * nn)
    ecc = np.where(top > 0, np.sqrt(np.minimum(f(2) * D / np.where(top > 0, top, f(1)), f(1))), f(0))
    q = g['quads'].astype(np.int64)
    n1, n2, nd, n3 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    diag = n1 + n3 + 2 * nd
    perimeter = n2.astype(f) + diag.astype(f) / np.sqrt(f(2))
    area = ni.astype(f)
    box = ((y1 + 1 - y0) * (x1 + 1 - x0)).astype(f)
    ab = np.array(DIRECTIONS, np.int64)
    a, b = ab[:, 0], ab[:, 1]
    half = (np.abs(a) + np.abs(b)).astype(f) * f(0.5)
    corner = a[None] * x0[:, None] + b[None] * y0[:, None]
    lo, hi = (ext[:, :, 0] - corner).astype(f), (ext[:, :, 1] - corner).astype(f)
    widths = (hi - lo + f(2) * half) / np.sqrt((a * a + b * b).astype(f))
    h = np.concatenate([hi + half, half - lo], axis=1)
    a16, b16 = np.concatenate([a, -a]).astype(f), np.concatenate([b, -b]).astype(f)
    a_n, b_n, h_n = np.roll(a16, -1), np.roll(b16, -1), np.roll(h, -1, 1)
    px, py = h * b_n - b16 * h_n, a16 * h_n - h * a_n
    polygon = f(0.5) * (px * np.roll(py, -1, 1) - np.roll(px, -1, 1) * py).sum(1)
    pi = f(math.pi)                                                   # the device multiplies by the float64 constant

    def z(t):
        return np.where(some if t.ndim == 1 else some[:, None], t, 0)

    assert ((n1 - n3 + 2 * nd) % 4 == 0).all() and ((n1 - n3 - 2 * nd) % 4 == 0).all()
    return dict(
        area=z(area), centroid_y=z(y0.astype(f) + sv / n), centroid_x=z(x0.astype(f) + su / n), var_y=z(B / nn), var_x=z(A / nn), cov=z(C / nn),
        major_axis=z(f(4) * np.sqrt(l1)), minor_axis=z(f(4) * np.sqrt(l2)), eccentricity=z(ecc), orientation=z(np.arctan2(f(2) * C, A - B) * f(0.5)),
        bbox=z(np.stack([y0, x0, y1 + 1, x1 + 1], axis=1)), bbox_fill=z(area / box), perimeter_crack=z(n1 + n2 + n3 + 2 * nd),
        perimeter=z(perimeter), circularity=z(f(4) * pi * area / np.where(some, perimeter * perimeter, f(1))),
        euler4=z((n1 - n3 + 2 * nd) // 4), euler8=z((n1 - n3 - 2 * nd) // 4), equivalent_diameter=z(np.sqrt(f(4) * area / pi)),
        feret_max=z(widths.max(1)), feret_min=z(widths.min(1)), polygon_area=z(polygon),
        convexity16=z(area / np.where(some, polygon, f(1))), border=z(g['border'].astype(np.int64)), widths=z(widths),
        exact=bool((np.abs(np.stack([n * suu, su * su, n * svv, sv * sv, n * suv, su * sv])) < 2.0 ** 53).all()))


def features(s):
    """[R, 13] in the dtype of ``s``: shape_features' columns of every row."""
    some = s['area'] > 0
    cols = [s[k] for k in FEATURES[:11]] + [np.where(some, 1 - s['euler8'], 0), (s['border'] > 0)]
    return np.stack([np.asarray(c, s['perimeter'].dtype) for c in cols], axis=1)


def clear_border(labels):
    """labels with every region that has a pixel on the image frame set to 0."""
    lab = np.asarray(labels)
    if lab.size == 0:
        return lab.copy()
    frame = np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]])
    return np.where(np.isin(lab, np.unique(frame)), 0, lab).astype(lab.dtype)
