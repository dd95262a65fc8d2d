"""Independent float64 numpy / scipy restatement of the nucleus-feature stage (dataflow/construct_feature_graph.py:50-123 +
common/nuc_feature.py), items 1-12 of cgc_net_amd.kernels.KernelSpec.nucleus_features.

It shares no code with the HIP path (csrc/nuclei.hip): scipy.ndimage.label for the components and the outside background, an
explicit Suzuki border follower, a monotone-chain hull, numpy.linalg.lstsq for the two ellipse fits, the entropy from per-pixel value
counts.  It is the oracle the GPU tests compare against (test infrastructure, not part of the package)."""
import numpy as np
from scipy import ndimage

DISK3 = [(dy, dx) for dy in range(-3, 4) for dx in range(-3, 4) if dy * dy + dx * dx <= 9]
assert len(DISK3) == 29
# OpenCV chain codes: 0 = +x, then counter-clockwise as seen on the screen (rows grow downwards)
CODE_DX = (1, 1, 0, -1, -1, -1, 0, 1)
CODE_DY = (0, -1, -1, -1, 0, 1, 1, 1)
RCOND = 1e-6


def bgr_to_gray(bgr):
    """Item 12: cv2.cvtColor(BGR2GRAY) on uint8 data."""
    bgr = np.asarray(bgr)
    b, g, r = (bgr[..., i].astype(np.int64) for i in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def remove_small_objects(mask, min_size=10):
    """Item 1: skimage 0.15 on an integer label image -- bincount over the whole image, no relabelling."""
    mask = np.asarray(mask)
    if mask.size and mask.min() < 0:
        raise ValueError('negative labels')
    out = mask.copy()
    sizes = np.bincount(mask.ravel())
    out[(sizes < min_size)[mask]] = 0
    return out


def entropy_at(gray, rows, cols, chunk=20000):
    """Item 5 at the given pixels: -sum p log2 p of the in-image values under disk(3).  Written per element: every value occurrence
    contributes -log2(count / pop) / pop."""
    H, W = gray.shape
    out = np.zeros(rows.size)
    for s in range(0, rows.size, chunk):
        r, c = rows[s:s + chunk], cols[s:s + chunk]
        vals = np.full((r.size, 29), -1, np.int64)
        for k, (dy, dx) in enumerate(DISK3):
            y, x = r + dy, c + dx
            ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
            vals[ok, k] = gray[y[ok], x[ok]]
        valid = vals >= 0
        pop = valid.sum(1).astype(np.float64)
        cnt = ((vals[:, :, None] == vals[:, None, :]) & valid[:, None, :]).sum(2)
        p = np.where(valid, cnt / pop[:, None], 1.0)
        out[s:s + r.size] = -(np.log2(p) / pop[:, None]).sum(1)
    return out


def choose_contour(fg):
    """Item 7: start pixel (row, col) of the top-level 8-connected component whose raster-first pixel comes last."""
    ch, cw = fg.shape
    comp, _ = ndimage.label(fg, structure=np.ones((3, 3), int))
    bl, _ = ndimage.label(np.pad(~fg, 1, constant_values=True))        # 4-connected background, the crop padded by one pixel
    outside = bl == bl[0, 0]
    ids, first = np.unique(comp.ravel(), return_index=True)
    best = -1
    for k, f in zip(ids, first):
        y, x = divmod(int(f), cw)
        if k != 0 and outside[y + 1, x]:                                 # padded position of (y, x - 1)
            best = max(best, int(f))
    return divmod(best, cw)


def trace_border(fg, y0, x0):
    """Item 8: Suzuki border following (8-connected) of an outer border from its raster-first pixel, CHAIN_APPROX_SIMPLE.
    Returns the kept vertices as (x, y)."""
    ch, cw = fg.shape

    def on(y, x):
        return 0 <= y < ch and 0 <= x < cw and bool(fg[y, x])

    s = 4
    while True:
        s = (s - 1) & 7
        if on(y0 + CODE_DY[s], x0 + CODE_DX[s]) or s == 4:
            break
    if s == 4:
        return [(x0, y0)]
    y1, x1 = y0 + CODE_DY[s], x0 + CODE_DX[s]
    y3, x3, prev = y0, x0, s ^ 4
    pts = []
    while True:
        y4, x4 = y3, x3
        while s < 15:
            s += 1
            y4, x4 = y3 + CODE_DY[s & 7], x3 + CODE_DX[s & 7]
            if on(y4, x4):
                break
        s &= 7
        if s != prev:
            pts.append((x3, y3))
            prev = s
        if (y4, x4) == (y0, x0) and (y3, x3) == (y1, x1):
            return pts
        y3, x3 = y4, x4
        s = (s + 4) & 7


def _shoelace2(pts):
    a = 0
    px, py = pts[-1]
    for x, y in pts:
        a += px * y - py * x
        px, py = x, y
    return a


def hull_area(pts):
    """Convex hull (Andrew's monotone chain) area of integer points; 0 for fewer than 3 distinct or collinear points."""
    p = sorted(set(pts))
    if len(p) < 3:
        return 0.0

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    lower, upper = [], []
    for q in p:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], q) <= 0:
            lower.pop()
        lower.append(q)
    for q in reversed(p):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], q) <= 0:
            upper.pop()
        upper.append(q)
    h = lower[:-1] + upper[:-1]
    return abs(_shoelace2(h)) * 0.5 if len(h) >= 3 else 0.0


def fit_ellipse(pts, ratios=None):
    """Item 10 (OpenCV 4.1 fitEllipseNoDirect restated): (width, height, angle) of the box, float32.  Points centred on their mean and
    scaled into [-1, 1]; lstsq with singular values below RCOND of the largest dropped.  ``ratios`` (a list) receives the conditioning
    of the three solves: per solve the singular values over the largest, s / s[0] -- a test uses it to keep its inputs clear of RCOND."""
    def lstsq(A, b):
        x, _, _, s = np.linalg.lstsq(A, b, rcond=RCOND)
        if ratios is not None:
            ratios.append(s / s[0] if s[0] > 0 else np.zeros_like(s))
        return x

    P = np.asarray(pts, np.float64)
    u, v = P[:, 0] - P[:, 0].mean(), P[:, 1] - P[:, 1].mean()
    amax = max(np.abs(u).max(), np.abs(v).max())
    sc = 1.0 / amax if amax > 0 else 1.0
    u, v = u * sc, v * sc
    g = lstsq(np.stack([-u * u, -v * v, -u * v, u, v], 1), np.ones(u.size))
    c = lstsq(np.array([[2 * g[0], g[2]], [g[2], 2 * g[1]]]), g[3:5])
    uu, vv = u - c[0], v - c[1]
    h = lstsq(np.stack([uu * uu, vv * vv, uu * vv], 1), np.ones(u.size)) * sc * sc
    th = -0.5 * np.arctan2(h[2], h[1] - h[0])
    t = h[2] / np.sin(-2.0 * th) if abs(h[2]) > 1e-8 else h[1] - h[0]
    ra, rb = abs(h[0] + h[1] - t), abs(h[0] + h[1] + t)
    ra = np.sqrt(2.0 / ra) if ra > 1e-8 else ra
    rb = np.sqrt(2.0 / rb) if rb > 1e-8 else rb
    w, hh, ang = np.float32(ra * 2), np.float32(rb * 2), np.float32(0)
    if w > hh:
        w, hh = hh, w
        ang = np.float32(90 + th * 180 / np.pi)
    return w, hh, ang


def shape_features(pts, ratios=None):
    """Item 9: (area, hull_area, solidity, perimeter, eccentricity, major, minor, orientation).  ``ratios``: see fit_ellipse."""
    V = len(pts)
    area = abs(_shoelace2(pts)) * 0.5 if V >= 3 else 0.0
    ha = hull_area(pts) if V >= 3 else 0.0
    if ha == 0:
        ha = 1.0
    perim = 0.0
    if V >= 2:
        px, py = pts[-1]
        for x, y in pts:
            perim += float(np.sqrt(np.float32((x - px) ** 2 + (y - py) ** 2)))
            px, py = x, y
    if V > 4:
        w, h, ang = fit_ellipse(pts, ratios)
        major, minor = max(w, h), min(w, h)
    else:
        major, minor, ang = np.float32(1), np.float32(1), np.float32(0)
    ecc = np.sqrt(1.0 - (float(minor) / float(major)) ** 2) if major != 0 else 0.0
    return area, ha, area / ha, perim, ecc, major, minor, ang


def intensity_features(fg, g):
    """Item 4."""
    fgv = g[fg].astype(np.float64)
    bgv = g[~fg].astype(np.float64)
    mean_fg = fgv.sum() / (fgv.size + 1e-8)
    diff = abs(mean_fg - bgv.sum() / (bgv.size + 1e-8))
    var = np.var(fgv)
    d = fgv - fgv.mean()
    m2, m3 = np.mean(d ** 2), np.mean(d ** 3)
    skew = 0.0 if m2 == 0 else m3 / m2 ** 1.5
    return mean_fg, diff, var, skew


def glcm_features(fg, g):
    """Item 6: (dissimilarity, homogeneity, energy, ASM)."""
    img = g.astype(np.int64) * fg
    a, b = img[:, :-1].ravel(), img[:, 1:].ravel()
    sel = (a > 0) & (b > 0)
    a, b = a[sel], b[sel]
    T = float(a.size) if a.size else 1.0
    P = np.bincount(a * 256 + b, minlength=65536).astype(np.float64) / T
    d = np.abs(a - b).astype(np.float64)
    asm = float((P * P).sum())
    return d.sum() / T, (1.0 / (1.0 + d * d)).sum() / T, np.sqrt(asm), asm


def nucleus_features(labels, gray, min_size=10, ratios=None):
    """Returns (features f32 [n, 16], centroids f32 [n, 2], kept_labels int32 [n], info int64 [n, 3] = contour start row, start col,
    vertex count).  ``ratios`` (a dict) receives per kept label that had an ellipse fit the three arrays fit_ellipse reports."""
    labels = np.asarray(labels)
    gray = np.asarray(gray)
    if labels.shape != gray.shape:
        raise ValueError('labels and gray differ in size')
    mask = remove_small_objects(labels.astype(np.int64), min_size)
    fg_all = mask > 0
    rr, cc = np.nonzero(fg_all)
    labs = mask[rr, cc]
    kept = np.unique(labs)
    cnt = np.bincount(labs)
    sr = np.bincount(labs, weights=rr.astype(np.float64))
    sc = np.bincount(labs, weights=cc.astype(np.float64))
    objs = ndimage.find_objects(mask)
    ent = np.zeros(gray.shape)
    ent[rr, cc] = entropy_at(gray, rr, cc)
    feats = np.zeros((kept.size, 16), np.float32)
    cens = np.zeros((kept.size, 2), np.float32)
    info = np.zeros((kept.size, 3), np.int64)
    for k, L in enumerate(kept):
        rs, cs = objs[L - 1]
        win = (slice(rs.start, rs.stop + 1), slice(cs.start, cs.stop + 1))     # bbox[0] : bbox[2] + 1 (quirk 3)
        fg, g, e = fg_all[win], gray[win], ent[win]
        mean_fg, diff, var, skew = intensity_features(fg, g)
        dis, hom, energy, asm = glcm_features(fg, g)
        y0, x0 = choose_contour(fg)
        pts = trace_border(fg, y0, x0)
        fit = None if ratios is None else []
        area, _, solidity, perim, ecc, major, minor, ang = shape_features(pts, fit)
        if fit:
            ratios[int(L)] = fit
        feats[k] = [mean_fg, diff, var, skew, e[fg].mean(), dis, hom, energy, asm, ecc, area, major, minor, perim, solidity, ang]
        cens[k] = [sr[L] / cnt[L], sc[L] / cnt[L]]
        info[k] = [y0, x0, len(pts)]
    return feats, cens, kept.astype(np.int32), info
