"""Hand-made scenes for the nucleus-feature stage (csrc/nuclei.hip) and the comparison with the float64 restatement
tests/nuclei_ref.py that the GPU tests share.  A plain module: no pytest hooks, no fixtures.

``SCENES[name]()`` returns (labels int32 [H, W], gray uint8 [H, W], min_size, names) -- numpy only, deterministic, at most 320 x 512.
``names`` maps a label value to what the shape is.  Where nuclei.synthetic_tissue covers the workload (rotated ellipses of 4-14 pixel
radius), these cover the branches: contours of 1, 2 and 4 vertices, pixels that lie on a contour several times, crops on both sides of
the LDS limit and one without a background pixel, more large crops than the global path has workspace slots, components whose minimum
must travel a long way against the raster order, the zero rules of the moments and the GLCM, the label pass with 64 labels in a wave,
kept labels on the compaction's ballot and chunk edges, and ``min_size`` at equality.
"""
import numpy as np
import torch

from cgc_net_amd import nuclei

import nuclei_ref as ref

DEV = torch.device('cuda:0')
C = {k: i for i, k in enumerate(nuclei.FEATURE_NAMES)}
LDS_PIXELS = 2048                        # cgc_nuclei_lds_max_pixels(): crops of at most this many pixels run in LDS
BIG_SLOTS = 32                           # NUC_BIG_SLOTS: workgroups (= workspace slots) of the global path


def _ulp_close(a, b, n=1):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    tol = n * np.spacing(np.maximum(np.abs(a), np.abs(b)))
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= tol


def _gpu(labels, gray, **kw):
    f, c, k, info = nuclei.nucleus_features(torch.from_numpy(labels).to(DEV), torch.from_numpy(gray).to(DEV), return_info=True, **kw)
    torch.cuda.synchronize()
    return f.cpu().numpy(), c.cpu().numpy(), k.cpu().numpy(), info.cpu().numpy()


def check_against_reference(labels, gray, min_size=10):
    f, c, k, info = _gpu(labels, gray, min_size=min_size)
    rf, rc, rk, rinfo = ref.nucleus_features(labels, gray, min_size=min_size)
    assert f.shape == rf.shape and np.array_equal(k, rk)
    assert np.array_equal(info[:, :3], rinfo), np.nonzero((info[:, :3] != rinfo).any(1))[0][:10]
    assert _ulp_close(c, rc).all()
    for name in ('area', 'perimeter', 'solidity', 'mean_im_out', 'diff', 'var_im'):
        ok = _ulp_close(f[:, C[name]], rf[:, C[name]])
        assert ok.all(), (name, np.nonzero(~ok)[0][:5], f[~ok, C[name]][:5], rf[~ok, C[name]][:5])
    for name in ('glcm_dissimilarity', 'glcm_homogeneity', 'glcm_energy', 'glcm_ASM'):
        np.testing.assert_allclose(f[:, C[name]], rf[:, C[name]], rtol=1e-6, atol=0, err_msg=name)
    np.testing.assert_allclose(f[:, C['skew_im']], rf[:, C['skew_im']], rtol=0, atol=1e-6)
    np.testing.assert_allclose(f[:, C['mean_ent']], rf[:, C['mean_ent']], rtol=1e-5, atol=0)
    for name in ('majoraxis_length', 'minoraxis_length', 'eccentricity'):
        np.testing.assert_allclose(f[:, C[name]], rf[:, C[name]], rtol=1e-4, atol=1e-6, err_msg=name)
    maj, mnr = rf[:, C['majoraxis_length']].astype(np.float64), rf[:, C['minoraxis_length']].astype(np.float64)
    sel = (maj - mnr) / np.maximum(maj, 1e-30) > 1e-3
    d = np.abs(f[sel, C['orientation']].astype(np.float64) - rf[sel, C['orientation']]) % 180
    assert (np.minimum(d, 180 - d) <= 1e-3).all()
    assert np.isfinite(f).all()
    return f, c, k, info


# ---- scene helpers
def crop_box(labels, L):
    """(r0, r1, c0, c1): the crop of label L, rows [r0, r1) x columns [c0, c1) -- its bounding box plus one row and one column,
    clipped at the image edge (KernelSpec.nucleus_features, item 3)."""
    rr, cc = np.nonzero(labels == L)
    H, W = labels.shape
    return int(rr.min()), min(int(rr.max()) + 2, H), int(cc.min()), min(int(cc.max()) + 2, W)


def crop_pixels(labels, L):
    r0, r1, c0, c1 = crop_box(labels, L)
    return (r1 - r0) * (c1 - c0)


def by_name(names):
    """name -> label of a scene's ``names``."""
    inv = {v: k for k, v in names.items()}
    assert len(inv) == len(names)
    return inv


def _ellipse(h, w, cy, cx, a, b, phi, hole=0.0):
    yy, xx = np.mgrid[0:h, 0:w]
    dy, dx = yy - cy, xx - cx
    u = dx * np.cos(phi) + dy * np.sin(phi)
    v = -dx * np.sin(phi) + dy * np.cos(phi)
    q = (u / a) ** 2 + (v / b) ** 2
    return (q <= 1.0) & (q > hole * hole)


def _spiral(n):
    """A square spiral, one pixel wide with one-pixel gaps, from (0, 0) clockwise inwards, in an n x n box."""
    m = np.zeros((n, n), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    while True:
        moved = 0
        while True:
            ny, nx = y + dy, x + dx
            if not (0 <= ny < n and 0 <= nx < n) or m[ny, nx]:
                break
            ay, ax = ny + dy, nx + dx
            if 0 <= ay < n and 0 <= ax < n and m[ay, ax]:
                break
            y, x = ny, nx
            m[y, x] = True
            moved += 1
        if moved < 2:
            return m
        dy, dx = dx, -dy


class _Canvas(object):
    """Paints one shape per label and refuses a shape that reaches into the crop of another one (or the other way round)."""

    def __init__(self, H, W, seed):
        self.labels = np.zeros((H, W), np.int32)
        self.gray = np.random.RandomState(seed).randint(0, 256, size=(H, W)).astype(np.uint8)
        self.crops = np.zeros((H, W), np.int32)      # label whose crop covers the pixel
        self.names = {}
        self.free = set()                            # labels allowed to share crops with each other (the ring pair)

    def put(self, name, top, left, mask, shared=False):
        L = len(self.names) + 1
        mask = np.asarray(mask, bool)
        rr, cc = np.nonzero(mask)
        rr, cc = rr + top, cc + left
        H, W = self.labels.shape
        assert rr.min() >= 0 and cc.min() >= 0 and rr.max() < H and cc.max() < W, name
        r0, r1, c0, c1 = int(rr.min()), min(int(rr.max()) + 2, H), int(cc.min()), min(int(cc.max()) + 2, W)
        others = set(np.unique(self.labels[r0:r1, c0:c1])) | set(np.unique(self.crops[rr, cc])) | set(np.unique(self.labels[rr, cc]))
        others -= {0} | (self.free if shared else set())
        assert not others, (name, sorted(others))
        self.labels[rr, cc] = L
        self.crops[r0:r1, c0:c1] = L
        self.names[L] = name
        if shared:
            self.free.add(L)
        return L


def shapes():
    """One shape per label on random gray, min_size 1.  Every shape except the ring pair keeps clear of the others' crops."""
    cv = _Canvas(160, 320, seed=11)
    one = np.ones
    # the LDS limit: 32 x 64 = 2048 pixels runs in LDS, one more column takes the global workspace
    cv.put('rect_lds_2048', 2, 2, one((31, 63)))
    cv.put('rect_global_2080', 2, 70, one((31, 64)))
    cv.put('rect_corner_2048', 128, 256, one((32, 64)))                  # crop clipped by the image corner: no background pixel
    # 1, 2 and 4 contour vertices
    cv.put('pixel', 40, 5, one((1, 1)))
    cv.put('hline', 40, 10, one((1, 12)))
    cv.put('vline', 40, 26, one((12, 1)))
    cv.put('diagonal', 40, 30, np.eye(12))
    cv.put('block2', 40, 46, one((2, 2)))
    cv.put('rect_5x9', 40, 52, one((5, 9)))
    plus = np.zeros((11, 11), bool)
    plus[4:7, :] = plus[:, 4:7] = True
    cv.put('plus', 40, 66, plus)
    # pixels that lie on the contour more than once
    bell = np.zeros((7, 18), bool)
    bell[:, :7] = bell[:, 11:] = bell[3, :] = True
    cv.put('dumbbell', 40, 82, bell)
    ell = np.zeros((12, 10), bool)
    ell[:, 0] = ell[11, :] = True
    cv.put('L', 40, 105, ell)
    stair = np.zeros((6, 12), bool)
    for k in range(6):
        stair[k, 2 * k:2 * k + 2] = True
    cv.put('staircase', 40, 120, stair)
    blocks = np.zeros((12, 12), bool)
    for k in range(6):
        blocks[2 * k:2 * k + 2, 2 * k:2 * k + 2] = True                  # 2 x 2 blocks that touch at their corners
    cv.put('staircase_blocks', 40, 180, blocks)
    cv.put('thin_ellipse', 40, 138, _ellipse(24, 36, 11.3, 17.6, 16.0, 1.6, 0.5))
    # the zero rules of the moments and the GLCM: patches of one gray level that reach 3 pixels (the entropy disk) past the crop
    cv.put('block_const', 84, 10, one((8, 8)))
    cv.gray[81:96, 7:22] = 77
    cv.put('block_zero', 84, 40, one((8, 8)))
    cv.gray[81:96, 37:52] = 0
    # a ring with a nucleus in its hole: the later-starting inner component is not top-level
    cv.put('ring', 84, 70, _ellipse(24, 28, 11.4, 13.7, 11.0, 8.0, 0.3, hole=0.6), shared=True)
    cv.put('ring_inner', 84, 70, _ellipse(24, 28, 11.4, 13.7, 3.3, 2.4, 0.3), shared=True)
    return cv.labels, cv.gray, 1, cv.names


def many_big():
    """40 rotated ellipses, one per 64 x 64 cell, every crop above the LDS limit: more than the 32 workspace slots of the global path,
    so slots 0..7 are used twice.  The large crops are listed in ascending label order and crop j runs in slot j % 32: the first row
    (j < 8) holds large ellipses, the last (j >= 32) small ones, those between alternate -- a slot's second nucleus is smaller than
    its first, and stale data would lie beyond it."""
    H, W = 320, 512
    rng = np.random.RandomState(12)
    labels = np.zeros((H, W), np.int32)
    names = {}
    for j in range(40):
        r, c = divmod(j, 8)
        large = j < 8 or (j < 32 and j % 2 == 0)
        a, b = (29.0, 27.0) if large else (24.0, 23.0)
        m = _ellipse(64, 64, 31.5 + rng.uniform(-0.4, 0.4), 31.5 + rng.uniform(-0.4, 0.4), a, b, rng.uniform(0, np.pi))
        labels[64 * r:64 * r + 64, 64 * c:64 * c + 64][m] = j + 1
        names[j + 1] = 'large' if large else 'small'
    gray = rng.randint(0, 256, size=(H, W)).astype(np.uint8)
    return labels, gray, 10, names


def spirals():
    """Two one-pixel-wide square spirals, each one 8-connected component whose minimum has to travel its whole length, half of it
    against the raster order: 63 x 63 (crop 64 x 64: global workspace) and, mirrored, 44 x 44 (crop 45 x 45 = 2025: LDS)."""
    labels = np.zeros((70, 120), np.int32)
    labels[2:65, 2:65][_spiral(63)] = 1
    labels[2:46, 70:114][_spiral(44)[:, ::-1]] = 2
    gray = np.random.RandomState(13).randint(0, 256, size=labels.shape).astype(np.uint8)
    return labels, gray, 10, {1: 'spiral_global', 2: 'spiral_lds'}


def stripes():
    """label = column + 1 on a 40 x 67 image: 64 distinct labels in every wave of the label pass, and waves that straddle rows."""
    H, W = 40, 67
    labels = np.tile(np.arange(1, W + 1, dtype=np.int32), (H, 1))
    gray = np.random.RandomState(14).randint(0, 256, size=(H, W)).astype(np.uint8)
    return labels, gray, 10, {c + 1: 'column_%d' % c for c in range(W)}


LABEL_EDGE_KEPT = (63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 5000)    # 12 pixels each
LABEL_EDGE_DROPPED = {65: 66, 1025: 1026, 2049: 2050}                         # 9 pixels each, right of the kept block named


def label_edges():
    """3 x 4 blocks whose label values sit on the compaction's ballot (64 | 65) and chunk (1024 | 1025, 2048 | 2049) edges, and three
    3 x 3 blocks that min_size 10 drops, each with its first column inside the crop of the kept block on its left."""
    labels = np.zeros((12, 12 * len(LABEL_EDGE_KEPT) + 4), np.int32)
    names = {}
    for i, L in enumerate(LABEL_EDGE_KEPT):
        labels[4:7, 2 + 12 * i:6 + 12 * i] = L
        names[L] = 'kept_%d' % L
        if L in LABEL_EDGE_DROPPED:
            labels[4:7, 6 + 12 * i:9 + 12 * i] = LABEL_EDGE_DROPPED[L]
            names[LABEL_EDGE_DROPPED[L]] = 'dropped_%d' % LABEL_EDGE_DROPPED[L]
    gray = np.random.RandomState(15).randint(0, 256, size=labels.shape).astype(np.uint8)
    return labels, gray, 10, names


SCENES = {'shapes': shapes, 'many_big': many_big, 'spirals': spirals, 'stripes': stripes, 'label_edges': label_edges}
