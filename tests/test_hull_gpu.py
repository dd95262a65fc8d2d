"""GPU: the exact convex hull per region (csrc/region.hip; cgc_net_amd.nuclei.region_hull, hull_shape, hull_features) against
tests/hull_ref.py.  Every integer table and the vertex list must equal the restatement EXACTLY, at the smallest shapes at which each
mechanism can fail: tile seams (t = the tile side, read from the library), runs that end on a tile's last column, labels of several
pieces, more labels in a tile than anything could fold, ``within``, and both routes of stage 2 (T = cgc_region_hull_tall_rows()).

The one float table is ``perimeter``: both sides sum, in hull order from vertex 0, the correctly rounded square roots of the same
integers (below 2^53, so the conversions are exact).  A sequential sum of ``count`` such terms, all positive, carries a relative error
of at most (count + 1) 2^-53 on either side -- one rounding per root, one per addition, first order -- so the two sides differ by at most
(count + 1) 2^-52 of the value.  That is the bound; it does not depend on the kernel's results.

hull_shape's float32 columns: both sides evaluate the same few float64 operations (/, sqrt: correctly rounded; atan2: a library
function, a few units of float64) on identical integers and round once to float32: the bound is one unit of float32, |got - want| <=
2^-23 |want|, as for region_shape (tests/test_shape_gpu.py)."""
import functools
import math

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, nuclei

import hull_ref as ref
from image_cases import gpu

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def sizes():
    k = kernels.get()
    return k.region_tile, k.region_hull_tall_rows


def same(got, want):
    """A RegionHull (with vertices) against the restatement's dict."""
    for name in ref.TABLES + ('vertices', 'ptr'):
        g = getattr(got, name)
        w = want[name]
        assert g.dtype == {np.dtype('int32'): torch.int32, np.dtype('int64'): torch.int64, np.dtype('float64'): torch.float64}[w.dtype], name
        assert tuple(g.shape) == w.shape, (name, tuple(g.shape), w.shape)
        g = g.cpu().numpy()
        if name == 'perimeter':
            bound = (want['count'] + 1) * 2.0 ** -52 * w
            err = np.abs(g - w)
            print('perimeter: worst error / bound %.3g' % float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all()
        else:
            assert np.array_equal(g, w), (name, np.argwhere(g != w)[:4])


def check(labels, max_label=None, within=None, dtype=None):
    """Every table and the vertices against the restatement; labels, within: numpy arrays.  Returns (RegionHull, the restatement)."""
    labels = np.asarray(labels, np.int32)
    top = int(labels.max()) if max_label is None and labels.size else (max_label or 0)
    lab = gpu(labels) if dtype is None else gpu(labels).to(dtype)
    got = nuclei.region_hull(lab, max_label=max_label, within=None if within is None else gpu(within), return_vertices=True)
    assert isinstance(got, nuclei.RegionHull)
    want = ref.tables(labels, top, within)
    same(got, want)
    return got, want


def canvas(H, W, mask, at=(0, 0), label=1):
    out = np.zeros((H, W), np.int32)
    h, w = mask.shape
    out[at[0]:at[0] + h, at[1]:at[1] + w][mask] = label
    return out


def disc(r):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return yy * yy + xx * xx <= r * r


# ------------------------------------------------------------------ single shapes
def test_one_pixel():
    got, _ = check(canvas(5, 6, np.ones((1, 1), bool), (2, 3)))
    assert got.count[1] == 4 and got.area2[1] == 2 and got.diameter2[1] == 2 and got.width_cross[1] == 1
    assert got.vertices[got.ptr[1]:got.ptr[2]].tolist() == [[2, 3], [3, 3], [3, 4], [2, 4]]
    assert got.diameter_ends[1].tolist() == [[2, 3], [3, 4]] and got.width_edge[1].tolist() == [1, 0]
    assert got.perimeter[1] == 4.0


SHAPES = {
    'row': np.ones((1, 9), bool),
    'column': np.ones((9, 1), bool),
    'rectangle': np.ones((3, 5), bool),
    'staircase': np.eye(7, dtype=bool),
    'anti_staircase': np.eye(7, dtype=bool)[::-1],
    'disc7': disc(7),
    'L': np.array([[1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [1, 1, 1, 1]], bool),
    'C': np.array([[1, 1, 1, 1], [1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [1, 1, 1, 1]], bool),
    'ring': disc(6) & ~np.pad(disc(3), 3),
}


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_single_shapes(name):
    m = SHAPES[name]
    got, want = check(canvas(m.shape[0] + 3, m.shape[1] + 4, m, (1, 2)))
    n = int(m.sum())
    assert want['area2'][1] >= 2 * n
    if name in ('row', 'column', 'rectangle'):
        assert want['area2'][1] == 2 * n and want['count'][1] == 4                  # solidity 1
    if name in ('L', 'C'):
        assert want['area2'][1] > 2 * n
    if name == 'staircase':
        assert want['count'][1] == 6                                                # the collinear corners are dropped
    if name == 'ring':
        full = ref.tables(canvas(13, 13, disc(6)), 1)
        assert np.array_equal(want['vertices'][want['ptr'][1]:want['ptr'][2]] - [1, 2], full['vertices'][full['ptr'][1]:])      # the hole does not matter


# ------------------------------------------------------------------ several regions
def test_two_pieces_with_empty_rows_between():
    lab = np.zeros((20, 12), np.int32)
    lab[2:4, 3:6] = 2
    lab[11:15, 7:9] = 2
    lab[6, 1] = 1
    got, want = check(lab)
    assert want['count'][2] >= 4 and want['area2'][2] > 2 * 14


def test_half_discs_that_touch():
    d = disc(9)
    lab = np.zeros((25, 25), np.int32)
    lab[3:22, 3:22][d] = 1
    lab[12:22, 3:22][d[9:]] = 2                                                     # the lower half is another label
    got, want = check(lab)
    assert got.vertices[got.ptr[1]:got.ptr[2], 0].max() == 12 and got.vertices[got.ptr[2]:got.ptr[3], 0].min() == 12


def test_missing_labels_are_rows_of_zeros():
    lab = np.zeros((6, 6), np.int32)
    lab[1:3, 1:3] = 3
    got, _ = check(lab, max_label=5)
    for L in (1, 2, 4, 5):
        assert got.count[L] == 0 and got.area2[L] == 0 and got.diameter2[L] == 0 and got.width_cross[L] == 0 and got.perimeter[L] == 0
        assert not got.diameter_ends[L].any() and not got.width_edge[L].any() and got.ptr[L] == got.ptr[L + 1]


# ------------------------------------------------------------------ image sizes and tile seams
@pytest.mark.parametrize('shape', [(1, 1), (1, 130), (130, 1), (65, 67)])
def test_image_sizes(shape):
    rng = np.random.RandomState(shape[0] * 131 + shape[1])
    check(rng.randint(0, 3, shape).astype(np.int32))
    check(np.ones(shape, np.int32))


def test_empty_images():
    for shape in ((0, 0), (0, 5), (5, 0)):
        got = nuclei.region_hull(torch.zeros(shape, dtype=torch.int32, device='cuda'), max_label=2, return_vertices=True)
        assert got.count.tolist() == [0, 0, 0] and tuple(got.vertices.shape) == (0, 2) and got.ptr.tolist() == [0, 0, 0, 0]
        assert not got.area2.any() and not got.perimeter.any()


def test_tile_seams():
    t, _ = sizes()
    rng = np.random.RandomState(5)
    blob = rng.rand(9, 11) < 0.6
    for at in ((10, t - 5), (t - 4, 10), (t - 4, t - 5), (2 * t - 4, t - 5)):        # vertical seam, horizontal seam, corners of four tiles
        check(canvas(2 * t + 9, 2 * t + 3, blob, at))
    lab = np.zeros((t + 2, 2 * t), np.int32)
    lab[3, t - 7:t] = 1                                                             # a run that ends exactly on a tile's last column
    lab[4, t - 1] = 1
    lab[5, t:t + 3] = 1                                                             # ... and one that begins on the next tile's first
    lab[7, 0:2 * t] = 2                                                             # a run across the whole image
    check(lab)


def test_every_pixel_its_own_label():
    lab = np.arange(70 * 70, dtype=np.int32).reshape(70, 70)
    got = nuclei.region_hull(gpu(lab), return_vertices=True)
    yy, xx = np.mgrid[0:70, 0:70]
    y, x = yy.ravel(), xx.ravel()
    assert (got.count == 4).all() and (got.area2 == 2).all() and (got.diameter2 == 2).all() and (got.width_cross == 1).all()
    assert (got.perimeter == 4.0).all()
    want = np.stack([np.stack([y, x], 1), np.stack([y + 1, x], 1), np.stack([y + 1, x + 1], 1), np.stack([y, x + 1], 1)], 1)
    assert np.array_equal(got.vertices.cpu().numpy().reshape(-1, 4, 2), want)
    assert np.array_equal(got.diameter_ends.cpu().numpy(), want[:, [0, 2]])
    assert (got.width_edge.cpu().numpy() == [1, 0]).all()
    part = nuclei.region_hull(gpu(lab[:2, :66]), max_label=70 * 70 - 1, return_vertices=True)
    same(part, ref.tables(lab[:2, :66], 70 * 70 - 1))


# ------------------------------------------------------------------ options
def test_within_removes_the_extreme_pixels():
    m = disc(7)
    lab = canvas(20, 21, m, (2, 3))
    within = np.ones(lab.shape, bool)
    within[2] = within[16] = False
    within[:, 3] = within[:, 17] = False
    got, want = check(lab, within=within)
    plain = ref.tables(lab, 1)
    assert want['area2'][1] < plain['area2'][1] and want['diameter2'][1] < plain['diameter2'][1]
    check(lab, within=within.astype(np.int32) * 7)
    check(lab, within=np.zeros(lab.shape, bool))                                    # nothing is counted anywhere


@pytest.mark.parametrize('dtype', nuclei._INT_DTYPES, ids=str)
def test_label_dtypes(dtype):
    rng = np.random.RandomState(11)
    check(rng.randint(0, 4, (13, 70)).astype(np.int32), dtype=dtype)


def test_labels_above_max_label_raise():
    lab = np.zeros((8, 8), np.int32)
    lab[2:4, 2:5] = 3
    for call in (lambda: nuclei.region_hull(gpu(lab), max_label=2), lambda: nuclei.region_hull(gpu(lab), max_label=2, return_vertices=True),
                 lambda: nuclei.hull_features(gpu(lab), torch.tensor([1], device='cuda'), max_label=2)):
        with pytest.raises(ValueError, match=r'6 pixels carry a label outside \[0, 2\]'):
            call()
    with pytest.raises(ValueError, match='kept_labels lie outside'):
        nuclei.hull_features(gpu(lab), torch.tensor([1, 4], device='cuda'), max_label=3)


# ------------------------------------------------------------------ the tall route
@functools.lru_cache(maxsize=None)
def tall_image():
    """One label with random holes, T + 70 rows high, and a second region of T rows -- just below the threshold -- beside it."""
    _, T = sizes()
    rng = np.random.RandomState(17)
    H = T + 70
    yy, xx = np.mgrid[0:H, 0:40]
    lab = np.zeros((H, 40), np.int32)
    tall = ((xx - 12 - 6 * np.sin(yy / 37.0)) ** 2 / 100.0 + (yy - H / 2.0) ** 2 / (H / 2.0) ** 2 <= 1.0) & (rng.rand(H, 40) < 0.6)
    tall[0, 12] = tall[H - 1, 13] = True
    lab[tall] = 1
    short = (np.abs(xx - 32 - 3 * np.cos(yy / 11.0)) <= 3) & (yy >= 5) & (yy < 5 + T) & (rng.rand(H, 40) < 0.7)
    short[5, 31] = short[4 + T, 33] = True
    lab[short & ~tall] = 2
    return lab


def test_tall_route_is_exact():
    _, T = sizes()
    lab = tall_image()
    rows = [np.nonzero((lab == L).any(1))[0] for L in (1, 2)]
    assert rows[0][-1] - rows[0][0] + 1 == T + 70 > T and rows[1][-1] - rows[1][0] + 1 == T      # one on each side of the threshold
    check(lab)                                                                      # label 0, the background, is tall as well


def test_both_routes_agree():
    """The same image through the library's own threshold, with every region on the short route, and with every region on the tall
    one: identical tables and vertices."""
    lab = tall_image()
    k = kernels.get()
    labels = gpu(lab)
    geometry = nuclei.region_geometry(labels, max_label=2)
    ptr = k.region_hull_ptr(geometry.count, geometry.extents)
    S = int(ptr[-1].item())
    runs = [k.region_hull(labels, 2, geometry.extents, ptr, S, tall_rows=rows) for rows in (0, lab.shape[0], 1)]
    first = 2 * (ptr[:-1] + torch.arange(3, device=ptr.device))
    for tables, points in runs[1:]:
        for a, b in zip(tables, runs[0][0]):
            assert torch.equal(a, b)
        for L in range(3):
            n = int(tables[0][L])
            assert torch.equal(points[first[L]:first[L] + n], runs[0][1][first[L]:first[L] + n])
    # and with every label cut into bands of T rows, so that the library's own threshold sends every piece down the short route
    _, T = sizes()
    cut = (lab * 2 + np.mgrid[0:lab.shape[0], 0:40][0] // T).astype(np.int32)
    assert (cut.max(), lab.shape[0] // T) == (5, 1)
    check(cut)


# ------------------------------------------------------------------ a tissue
@functools.lru_cache(maxsize=None)
def tissue_case():
    labels, _ = nuclei.synthetic_tissue(256, 256, 40)
    labels = np.asarray(labels, np.int32)
    top = int(labels.max())
    return labels, top, ref.tables(labels, top)


def test_tissue_equals_the_restatement_twice():
    labels, top, want = tissue_case()
    a = nuclei.region_hull(gpu(labels), max_label=top, return_vertices=True)
    same(a, want)
    b = nuclei.region_hull(gpu(labels), max_label=top, return_vertices=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)                                                    # bit-identical, the perimeter included


def test_hull_shape_and_features():
    labels, top, want = tissue_case()
    lab = gpu(labels)
    hull = nuclei.region_hull(lab, max_label=top)
    assert hull.vertices is None and hull.ptr is None
    geometry = nuclei.region_geometry(lab, max_label=top)
    shape = nuclei.hull_shape(hull, geometry)
    count = np.bincount(labels.ravel(), minlength=top + 1)
    ws = ref.shape(want, count)
    for name in nuclei.HullShape._fields:
        g = getattr(shape, name)
        assert g.dtype == torch.float32 and tuple(g.shape) == (top + 1,), name
        w32 = ws[name].astype(np.float32).astype(np.float64)
        err = np.abs(g.cpu().numpy().astype(np.float64) - w32)
        print('%-18s worst error / bound %.3g' % (name, float((err / np.maximum(ULP * np.abs(w32), 1e-300)).max()) if err.any() else 0.0))
        assert (err <= ULP * np.abs(w32)).all(), name
    assert (shape.solidity <= 1).all() and (shape.solidity[count > 0] > 0).all()
    assert (shape.feret_angle > -math.pi / 2).all() and (shape.feret_angle <= float(np.float32(math.pi / 2))).all()
    kept = torch.tensor([5, 1, top, 0, 5], device=lab.device)
    feats = nuclei.hull_features(lab, kept, max_label=top)
    assert feats.dtype == torch.float32 and tuple(feats.shape) == (5, len(nuclei.HULL_FEATURE_NAMES))
    table = torch.stack([getattr(shape, name) for name in nuclei.HULL_FEATURE_NAMES], 1)
    assert torch.equal(feats, table[kept])
    assert torch.equal(nuclei.hull_features(lab, kept.to(torch.int32), max_label=top), feats)


def test_relations_to_the_geometry():
    """On the same image, in float64 from the integer tables: n <= hull area <= the 16-gon's; the diameter is at least the largest of
    the eight square widths and the width at most the smallest; the hull vertices' extents in the eight directions are the extents of
    the pixel centres plus the half-square terms."""
    labels, top, want = tissue_case()
    lab = gpu(labels)
    geometry = nuclei.region_geometry(lab, max_label=top)
    shape = nuclei.region_shape(geometry)
    hull = nuclei.region_hull(lab, max_label=top, return_vertices=True)
    some = (hull.count > 0).cpu().numpy()
    assert np.array_equal(some, geometry.count.cpu().numpy() > 0) and some.sum() >= 30      # the ids are sparse: rows with pixels only
    n = geometry.count.cpu().numpy().astype(np.float64)[some]
    area = hull.area2.cpu().numpy()[some] / 2.0
    ext = geometry.extents.cpu().numpy().astype(np.int64)
    ab = np.array(nuclei.GEOMETRY_DIRECTIONS, np.int64)
    norm = np.sqrt((ab ** 2).sum(1).astype(np.float64))
    widths = ((ext[:, :, 1] - ext[:, :, 0] + np.abs(ab).sum(1)) / norm)[some]                 # of the pixel squares, float64
    assert (n <= area).all()
    assert (area <= shape.polygon_area.cpu().numpy().astype(np.float64)[some] * (1 + 2.0 ** -23)).all()      # polygon_area is float32
    assert (np.sqrt(hull.diameter2.cpu().numpy().astype(np.float64))[some] * (1 + 2.0 ** -50) >= widths.max(1)).all()
    e = hull.width_edge.cpu().numpy().astype(np.float64)[some]
    width = hull.width_cross.cpu().numpy()[some] / np.sqrt((e ** 2).sum(1))
    assert (width <= widths.min(1) * (1 + 2.0 ** -50)).all()
    v, ptr = hull.vertices.cpu().numpy().astype(np.int64), hull.ptr.cpu().numpy()
    for L in np.nonzero(some)[0]:
        p = v[ptr[L]:ptr[L + 1]]
        proj = p[:, 1:2] * ab[None, :, 0] + p[:, 0:1] * ab[None, :, 1]                # a x + b y at every vertex, [k, 8]
        # a pixel centre is (x + 1/2, y + 1/2) in corner coordinates; the square adds (|a| + |b|) / 2 on either side: doubled, in integers
        assert np.array_equal(2 * proj.min(0), 2 * ext[L, :, 0] + ab.sum(1) - np.abs(ab).sum(1)), L
        assert np.array_equal(2 * proj.max(0), 2 * ext[L, :, 1] + ab.sum(1) + np.abs(ab).sum(1)), L
