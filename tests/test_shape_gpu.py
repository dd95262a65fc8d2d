"""GPU: the region geometry (csrc/region.hip; cgc_net_amd.nuclei.region_geometry, region_shape, shape_features, clear_border) against
tests/shape_ref.py.  The integer tables are compared bit for bit, at the smallest shapes at which each mechanism can fail: tile
seams, the frame of quads around the image, more labels in a tile than its table holds, labels that collide in the table's hash, sums
past 32 bits, extents of negative value.  t = the tile side and S = the table slots are read from the library.

The float columns of region_shape.  Both sides evaluate the formulas of region_shape's docstring in float64 from identical integers
and round once to float32.  On every input used here the moment products n suu, su^2, ... stay below 2^53 (asserted: ``exact``), so A,
B, C are exact integers on both sides and what follows is a handful of float64 operations (+, -, *, /, sqrt: correctly rounded by
IEEE 754 on both sides; atan2: a library function, accurate to a few units of the last place) on values of like sign, or quotients and
roots of them.  Such a value carries a relative error of at most some tens of 2^-53 on either side, which is far below half a unit
of the float32 it is rounded to; the two roundings can therefore differ only when the float64 value lies that close to a float32
rounding boundary, and then by one float32 unit.  The bound for these columns is one unit in the last place of float32, taken as
|got - want| <= 2^-23 |want| (a unit of float32 is between 2^-24 and 2^-23 of the value).  That covers eccentricity = sqrt(2 D / (A + B
+ D)) and orientation = atan2(2 C, A - B) / 2 as well: with A, B, C exact there is no cancellation left in them, and a region that is
exactly isotropic (a pixel, a square, a disc) has A - B = C = 0 exactly and gives an exact 0 (tested on its own).  A region whose
moments pass 2^53 -- tens of thousands of pixels -- would bring the cancellation back near isotropy; none is used here, so
the columns are tested away from that singularity.
The one column with a cancellation is minor_axis = 4 sqrt(l2), l2 = (A + B - D) / (2 n^2): the difference has an absolute error of at
most 8 * 2^-53 (A + B) <= 16 * 2^-53 * l1 * 2 n^2 (D from a root of a sum of two squares, two additions), so l2 is off by at most 2^-48
l1, its root by at most sqrt(2^-48 l1) = 2^-24 sqrt(l1) (the root's slope is unbounded at 0; sqrt(l2 + e) - sqrt(l2) <= sqrt(e)), and
minor_axis by 2^-24 * 4 sqrt(l1) = 2^-24 major_axis.  Its bound is 2^-23 |want| + 2^-23 major_axis (both sides carry the error)."""
import functools
import math

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, nuclei

import shape_ref as ref
from image_cases import DEV, gpu, tissue, two_discs

pytestmark = pytest.mark.gpu

TABLES = ('count', 'sy', 'sx', 'syy', 'sxy', 'sxx', 'extents', 'quads', 'border')
ULP = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def sizes():
    k = kernels.get()
    return k.region_tile, k.region_slots


def same_tables(got, want):
    for name in TABLES:
        g = getattr(got, name)
        assert g.dtype == (torch.int64 if name[0] == 's' else torch.int32), name
        assert g.shape == want[name].shape and np.array_equal(g.cpu().numpy(), want[name]), name


def check(labels, max_label=None, within=None):
    """Every table against the restatement; labels, within: numpy arrays.  Returns the RegionGeometry."""
    top = int(labels.max()) if max_label is None and labels.size else (max_label or 0)
    got = nuclei.region_geometry(gpu(labels), max_label=max_label, within=None if within is None else gpu(within))
    assert isinstance(got, nuclei.RegionGeometry)
    same_tables(got, ref.geometry(labels, top, within))
    return got


def check_shape(geometry, want_g):
    """region_shape of a RegionGeometry against the restatement of the same integers: integer tables exactly, float tables within the
    bounds of the module docstring.  Returns (shape, want)."""
    shape = nuclei.region_shape(geometry)
    want = ref.shape(want_g)
    assert want['exact']                                                # the premise of the bounds: no moment product passes 2^53
    for k in ref.SHAPE_INTS:
        got = getattr(shape, k)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want[k]), k
    assert np.array_equal(shape.area.cpu().numpy(), want['area'].astype(np.float32))
    assert np.array_equal(shape.polygon_area.cpu().numpy(), want['polygon_area'].astype(np.float32))      # half-integers: exact
    for k in ref.SHAPE_FLOATS:
        got = getattr(shape, k)
        assert got.dtype == torch.float32 and got.dim() == 1, k
        w32 = want[k].astype(np.float32).astype(np.float64)
        bound = ULP * np.abs(w32) + (ULP * want['major_axis'] if k == 'minor_axis' else 0.0)
        err = np.abs(got.cpu().numpy().astype(np.float64) - w32)
        print('%-20s worst error / bound: %.3g' % (k, float((err / np.maximum(bound, 1e-300)).max()) if err.any() else 0.0))
        assert (err <= bound).all(), k
    return shape, want


def random_labels(H, W, top, seed):
    return np.random.RandomState(seed).randint(0, top + 1, (H, W)).astype(np.int32)


def blobs(H, W, top, seed, cell=7):
    """Labels in patches of ``cell`` pixels: long runs down the columns, as an instance mask has them."""
    rng = np.random.RandomState(seed)
    coarse = rng.randint(0, top + 1, (H // cell + 1, W // cell + 1))
    return np.kron(coarse, np.ones((cell, cell), np.int64))[:H, :W].astype(np.int32)


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize('shape', [(0, 5), (5, 0), (1, 1), (1, 7), (7, 1)])
def test_degenerate_shapes(shape):
    labels = random_labels(shape[0], shape[1], 3, 1)
    check(labels, max_label=3)
    check(labels)                                                       # the range read from the labels; an empty image has row 0 only
    check(labels, max_label=3, within=np.zeros(shape, bool))
    check(labels, max_label=3, within=np.ones(shape, np.int16))


def test_max_label_far_above_the_largest_and_an_all_zero_within():
    t, S = sizes()
    labels = random_labels(t + 3, 9, 4, 3)
    g = check(labels, max_label=5000)                                   # rows 5 .. 5000 are empty
    assert all(int(getattr(g, name)[5:].abs().sum()) == 0 for name in TABLES)
    shape = nuclei.region_shape(g)
    assert all(int((getattr(shape, k)[5:] != 0).sum()) == 0 for k in shape._fields)
    g = check(labels, max_label=4, within=np.zeros(labels.shape, np.uint8))
    assert all(int(getattr(g, name).abs().sum()) == 0 for name in TABLES)
    g = check(np.zeros((t + 3, 9), np.int32), max_label=0)
    assert g.count.tolist() == [(t + 3) * 9]


# ------------------------------------------------------------------ tile seams
def test_random_image_over_tile_seams():
    t, S = sizes()
    check(random_labels(t + 3, 2 * t + 5, 5, 4))
    check(blobs(t + 3, 2 * t + 5, 5, 5))
    check(blobs(2 * t + 1, t + 2, 5, 6), within=np.random.RandomState(7).rand(2 * t + 1, t + 2) < 0.8)


@pytest.mark.parametrize('shift', [-1, 0, 1])
@pytest.mark.parametrize('axis', [0, 1])
def test_a_label_boundary_on_and_beside_a_seam(axis, shift):
    t, S = sizes()
    labels = np.ones((t + 9, t + 9), np.int32)
    if axis == 0:
        labels[t + shift:] = 2                                          # the boundary runs along a seam, or one pixel to either side
    else:
        labels[:, t + shift:] = 2
    g = check(labels)
    n = t + 9
    assert g.quads[1].tolist() == [4, 2 * (n - 1) + 2 * (t + shift - 1), 0, 0]      # a rectangle: corners and straight edges only
    assert g.count.tolist() == [0, n * (t + shift), n * (9 - shift)]


def test_checkerboard_across_a_seam_corner():
    t, S = sizes()
    n = t + 4                                                           # four tiles meet at (t, t)
    yy, xx = np.mgrid[0:n, 0:n]
    labels = (1 + (yy + xx) % 2).astype(np.int32)
    g = check(labels)
    inner = (n - 1) * (n - 1)                                           # every quad inside the image is the two diagonals
    assert g.quads[:, 2].tolist() == [0, inner, inner] and g.quads[:, 3].tolist() == [0, 0, 0]
    assert g.quads[1, 1] == 0 and g.quads[2, 1] == 0                    # no two pixels of a label share an edge
    # the frame: 4 (n - 1) quads hold two pixels, one of each label, and give each an n1; the four corner quads hold one pixel
    assert int(g.quads[1, 0] + g.quads[2, 0]) == 8 * (n - 1) + 4


# ------------------------------------------------------------------ the frame
@pytest.mark.parametrize('shape', ['t+3 x 2t+1', 't x t', '1 x t+2'])
def test_an_image_of_one_label(shape):
    t, S = sizes()
    H, W = {'t+3 x 2t+1': (t + 3, 2 * t + 1), 't x t': (t, t), '1 x t+2': (1, t + 2)}[shape]
    g = check(np.full((H, W), 3, np.int32))
    assert g.quads[3].tolist() == [4, 2 * (H - 1) + 2 * (W - 1), 0, 0]
    assert g.border[3] == (2 * H + 2 * W - 4 if H > 1 and W > 1 else H * W) and g.count[3] == H * W
    assert g.extents[3, 0].tolist() == [0, W - 1] and g.extents[3, 4].tolist() == [0, H - 1]
    assert g.sy[3] == W * H * (H - 1) // 2 and g.sxx[3] == H * (W - 1) * W * (2 * W - 1) // 6


def test_a_region_of_one_tile_exactly():
    t, S = sizes()
    labels = np.zeros((2 * t + 1, 2 * t + 1), np.int32)
    labels[t:2 * t, t:2 * t] = 3                                        # no mixed quad inside its tile; its edges belong to four tiles' quads
    labels[-1, :] = 7                                                   # only on the image's last row ...
    labels[:, -1] = 7                                                   # ... and last column
    g = check(labels)
    assert g.quads[3].tolist() == [4, 4 * (t - 1), 0, 0] and g.border[3] == 0 and g.border[7] == 4 * t + 1
    assert g.extents[3, 0].tolist() == [t, 2 * t - 1]


# ------------------------------------------------------------------ more labels than the table holds
def test_every_pixel_its_own_label():
    t, S = sizes()
    labels = np.random.RandomState(6).permutation(t * t).astype(np.int32).reshape(t, t)
    assert t * t > S
    g = check(labels)
    assert (g.count == 1).all() and (g.quads[:, 0] == 4).all() and int(g.quads[:, 1:].abs().sum()) == 0
    check(np.random.RandomState(8).permutation((t + 6) * (t + 6)).astype(np.int32).reshape(t + 6, t + 6))


def test_the_direct_route_with_within_on_partial_tiles():
    t, S = sizes()
    n = t + 6                                                           # four tiles, three of them partial; 64 labels of each fold
    labels = np.random.RandomState(6).permutation(n * n).astype(np.int32).reshape(n, n)
    within = (np.indices((n, n)).sum(0) % 2).astype(np.int16)           # a checkerboard: every pixel that belongs is a run of one
    g = check(labels, within=within)
    assert np.array_equal(g.count.cpu().numpy()[labels.reshape(-1)], within.reshape(-1))


@pytest.mark.parametrize('extra', [0, 1])
def test_exactly_as_many_labels_as_slots_and_one_more(extra):
    t, S = sizes()
    rng = np.random.RandomState(8 + extra)
    labels = rng.randint(0, S + extra, (t, t)).astype(np.int32)
    labels.reshape(-1)[:S + extra] = np.arange(S + extra)               # every label is there
    g = check(labels)
    assert (g.count > 0).all() and g.count.numel() == S + extra


def slot_hash(L, S):
    """The slot a label asks for first (csrc/region.hip, region_slot)."""
    return ((np.asarray(L, np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xffffffff)) >> np.uint64(32 - int(math.log2(S)))


def test_labels_that_collide_in_the_hash():
    t, S = sizes()
    ids = np.arange(1, 40000)
    ids = ids[slot_hash(ids, S) == slot_hash(ids[0], S)][:24].astype(np.int32)      # more than any probe sequence is long
    assert len(ids) == 24 and len(set(slot_hash(ids, S).tolist())) == 1
    rng = np.random.RandomState(10)
    labels = ids[rng.randint(0, len(ids), ((t + 9) // 3 + 1, (t + 2) // 2 + 1))]
    labels = np.kron(labels, np.ones((3, 2), np.int32))[:t + 9, :t + 2]
    labels[1, 0] = ids[-1]
    got = nuclei.region_geometry(gpu(labels))
    compact = np.searchsorted(ids, labels).astype(np.int32)
    want = ref.geometry(compact, len(ids) - 1)
    rows = gpu(ids).long()
    for name in TABLES:
        table = getattr(got, name)
        assert np.array_equal(table[rows].cpu().numpy(), want[name]), name
        assert int(table.abs().sum()) == int(np.abs(want[name]).sum()), name      # and no other row holds anything
    check(labels[:, :9], within=rng.rand(t + 9, 9) < 0.5)


def test_a_label_permutation_permutes_the_tables():
    t, S = sizes()
    labels = blobs(t + 5, t + 7, 90, 11, cell=3)                        # more labels than slots
    perm = np.random.RandomState(12).permutation(91).astype(np.int32)
    a = nuclei.region_geometry(gpu(labels), max_label=90)
    b = nuclei.region_geometry(gpu(perm[labels]), max_label=90)
    for name in TABLES:
        assert torch.equal(getattr(a, name), getattr(b, name)[gpu(perm).long()]), name
    check(perm[labels], max_label=90)


# ------------------------------------------------------------------ within
def test_within_cuts_a_region_in_two_and_one_pixel_of_a_quad():
    t, S = sizes()
    labels = np.zeros((t + 6, t + 6), np.int32)
    labels[3:t + 3, 5:15] = 1                                           # a bar over the seam
    within = np.ones(labels.shape, bool)
    within[t - 1:t + 1] = False                                         # cut in two, on both sides of the seam
    g = check(labels, within=within)
    assert g.quads[1].tolist()[0] == 8 and int(nuclei.region_shape(g).euler8[1]) == 2
    within = np.ones(labels.shape, np.int32)
    within[10, 10] = 0                                                  # a hole of one pixel: four quads lose a position
    g = check(labels, within=within)
    assert g.quads[1].tolist() == [4, 2 * (t - 1) + 2 * 9, 0, 4] and int(nuclei.region_shape(g).euler8[1]) == 0
    within[t, 5] = 0                                                    # and one on the seam, on the bar's edge
    check(labels, within=within)


# ------------------------------------------------------------------ extents
def test_single_pixels_at_the_image_corners():
    t, S = sizes()
    n = t + 1
    labels = np.zeros((n, n), np.int32)
    for L, (y, x) in enumerate(((0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1)), start=1):
        labels[y, x] = L
    g = check(labels)
    for L, (y, x) in enumerate(((0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1)), start=1):
        assert g.extents[L].tolist() == [[a * x + b * y] * 2 for a, b in nuclei.GEOMETRY_DIRECTIONS]
        assert g.quads[L].tolist() == [4, 0, 0, 0] and g.border[L] == 1
    assert g.extents[2, 7].tolist() == [-2 * t, -2 * t]                 # (-2, 1): negative values


def test_negative_extents_over_tiles():
    t, S = sizes()
    labels = np.zeros((t + 3, 2 * t + 9), np.int32)
    labels[2:6, t - 2:2 * t + 7] = 1                                    # far right, near the top: -2 x + y is negative all over it
    labels[t:t + 2, 1:4] = 2
    g = check(labels)
    assert g.extents[1, 7].tolist() == [-2 * (2 * t + 6) + 2, -2 * (t - 2) + 5]
    assert g.extents[1, 5].tolist() == [-(2 * t + 6) + 4, -(t - 2) + 10]


# ------------------------------------------------------------------ 64-bit sums
def test_sums_past_32_bits():
    W = 32767
    labels = np.full((2, W), 1, np.int32)
    g = check(labels)
    assert int(g.sxx[1]) == 2 * (W - 1) * W * (2 * W - 1) // 6 > 2 ** 32
    assert int(g.sx[1]) == W * (W - 1) and int(g.sxy[1]) == W * (W - 1) // 2 and int(g.sy[1]) == W and int(g.syy[1]) == W
    assert g.quads[1].tolist() == [4, 2 * (W - 1) + 2, 0, 0] and g.border[1] == 2 * W


# ------------------------------------------------------------------ dtypes and strides
@pytest.mark.parametrize('ldtype', [torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64])
def test_every_label_dtype(ldtype):
    t, S = sizes()
    labels = blobs(t + 2, t + 2, 100, 14, cell=5)
    got = nuclei.region_geometry(gpu(labels).to(ldtype), max_label=100)
    same_tables(got, ref.geometry(labels, 100))


@pytest.mark.parametrize('wdtype', [torch.bool, torch.uint8, torch.int16, torch.int32, torch.int64])
def test_every_within_dtype(wdtype):
    t, S = sizes()
    labels = blobs(t + 2, 20, 6, 15, cell=4)
    within = np.random.RandomState(16).rand(t + 2, 20) < 0.7
    Wn = gpu(within) if wdtype == torch.bool else (gpu(within).to(torch.int64) * (200 if wdtype == torch.uint8 else -3)).to(wdtype)
    got = nuclei.region_geometry(gpu(labels), max_label=6, within=Wn)
    same_tables(got, ref.geometry(labels, 6, within))


def test_transposed_views():
    t, S = sizes()
    rng = np.random.RandomState(17)
    big, wbig = blobs(t + 9, t + 5, 6, 18, cell=4), (rng.rand(t + 9, t + 5) < 0.6).astype(np.int64)
    L, Wn = gpu(big).T, gpu(wbig).T
    assert not L.is_contiguous() and not Wn.is_contiguous()
    got = nuclei.region_geometry(L, max_label=6, within=Wn)
    same_tables(got, ref.geometry(np.ascontiguousarray(big.T), 6, np.ascontiguousarray(wbig.T)))
    L = gpu(np.repeat(np.repeat(big, 2, 0), 3, 1))[::2, 1::3]
    assert not L.is_contiguous()
    same_tables(nuclei.region_geometry(L, max_label=6), ref.geometry(big, 6))


# ------------------------------------------------------------------ refusals that need the device
def test_labels_that_do_not_fit_int32_are_refused_not_wrapped():
    labels = torch.ones(4, 5, dtype=torch.int64, device=DEV)
    labels[1, 1] = 2 ** 32 + 1                                          # would be label 1 after a narrowing cast
    with pytest.raises(ValueError, match='outside'):
        nuclei.region_geometry(labels, max_label=3)


def test_refused_labels_raise_and_the_next_call_is_clean():
    t, S = sizes()
    labels = random_labels(t + 3, t + 3, 5, 18)
    L = gpu(labels)
    kept = torch.arange(1, 5, dtype=torch.int32, device=DEV)
    calls = (nuclei.region_geometry, nuclei.clear_border, lambda lab, **kw: nuclei.shape_features(lab, kept, **kw))
    for fn in calls:
        with pytest.raises(ValueError, match='outside'):
            fn(L, max_label=4)                                          # label 5 is above max_label
        bad = L.clone()
        bad[t + 1, t + 2] = -3
        with pytest.raises(ValueError, match='outside'):
            fn(bad, max_label=5)
        with pytest.raises(ValueError, match='negative'):
            fn(bad)
    with pytest.raises(ValueError, match='outside'):
        nuclei.region_geometry(bad, max_label=5, within=torch.zeros_like(L))      # whatever `within` says at that pixel
    check(labels)                                                       # the call after a refusal: meta starts at zero again
    # the library counts them: meta is the number of refused pixels, and the rest is still exact
    tables, meta = kernels.get().region_geometry(L, 4)
    assert int(meta) == int((labels == 5).sum()) == ref.refused(labels, 4)
    want = ref.geometry(labels, 4)
    assert np.array_equal(tables[0].cpu().numpy(), want['count']) and np.array_equal(tables[3].cpu().numpy(), want['quads'])
    for bad_kept in (torch.tensor([1, 6], device=DEV), torch.tensor([-1], device=DEV)):
        with pytest.raises(ValueError, match='kept_labels'):
            nuclei.shape_features(L, bad_kept, max_label=5)


# ------------------------------------------------------------------ tissue
@functools.lru_cache(maxsize=None)
def tissue_case():
    labels, gray, within = tissue()
    top = int(labels.max())
    return labels, gray, within, top, ref.geometry(labels, top), ref.geometry(labels, top, within)


def test_tissue_bit_for_bit_and_from_call_to_call():
    labels, gray, within, top, want, want_w = tissue_case()
    L, Wn = gpu(labels), gpu(within)
    a = nuclei.region_geometry(L, max_label=top)
    b = nuclei.region_geometry(L, max_label=top)
    same_tables(a, want)
    for name in TABLES:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    c = nuclei.region_geometry(L, max_label=top, within=Wn)
    same_tables(c, want_w)
    for name in TABLES:
        assert torch.equal(getattr(c, name), getattr(nuclei.region_geometry(L, max_label=top, within=Wn), name)), name


def test_region_shape_on_tissue():
    labels, gray, within, top, want, want_w = tissue_case()
    L = gpu(labels)
    shape, w = check_shape(nuclei.region_geometry(L, max_label=top), want)
    check_shape(nuclei.region_geometry(L, max_label=top, within=gpu(within)), want_w)
    ecc = w['eccentricity'][w['area'] > 0]
    assert ((ecc == 0) | (ecc > 2.0 ** -10)).all()                      # every region is exactly isotropic or far from it
    assert (w['area'] > 0).sum() > 50 and (w['border'] > 0).sum() >= 5  # nuclei, some of them cut by the frame (and the background)


def hand_cases():
    """One label image that holds the hand cases of tests/test_shape_ref_cpu.py, apart from each other."""
    labels = np.zeros((40, 60), np.int32)
    labels[3, 3] = 1                                                    # one pixel
    labels[6:8, 6:8] = 2                                                # a 2 x 2 square
    labels[11, 3] = labels[12, 3] = labels[12, 4] = 3                   # an L-tromino
    labels[16, 3] = labels[17, 4] = 4                                   # two pixels on a diagonal
    labels[20:23, 3:6] = 5
    labels[21, 4] = 0                                                   # a 3 x 3 ring
    labels[26, 3:10] = 6                                                # a horizontal bar
    labels[10:17, 20] = 7                                               # the same bar transposed
    labels[20:23, 20:27] = 8                                            # 3 x 7
    labels[0, 30:33] = 9                                                # on the frame
    yy, xx = np.mgrid[0:40, 0:60]
    labels[(yy - 28) ** 2 + (xx - 45) ** 2 <= 64] = 10                  # a disc: exactly isotropic
    labels[(2 * (yy - 10) - (xx - 45)) ** 2 + ((yy - 10) + 2 * (xx - 45)) ** 2 // 9 <= 60] = 11      # a slanted ellipse
    return labels


def test_region_shape_on_the_hand_cases():
    labels = hand_cases()
    want_g = ref.geometry(labels, 11)
    shape, w = check_shape(nuclei.region_geometry(gpu(labels), max_label=11), want_g)
    s = {k: getattr(shape, k).cpu().numpy() for k in shape._fields}
    for L in (1, 2, 5, 10):                                             # exactly isotropic: the rule gives an exact 0
        assert s['eccentricity'][L] == 0 and s['orientation'][L] == 0 and s['major_axis'][L] == s['minor_axis'][L], L
    assert s['euler8'].tolist()[1:10] == [1, 1, 1, 1, 0, 1, 1, 1, 1] and s['euler4'][4] == 2
    assert s['perimeter_crack'].tolist()[1:6] == [4, 8, 8, 8, 16]
    assert s['orientation'][6] == 0 and s['orientation'][7] == np.float32(math.pi / 2) and s['orientation'][4] == np.float32(math.pi / 4)
    assert s['eccentricity'][6] == 1 and s['major_axis'][6] == 8 and s['minor_axis'][6] == 0
    assert abs(float(s['eccentricity'][8]) - math.sqrt(1 - (8 / 12) / 4.0)) <= ULP      # 3 x 7: var_y = 8 / 12, var_x = 4
    assert s['bbox'][3].tolist() == [11, 3, 13, 5] and s['bbox_fill'][3] == 0.75 and s['polygon_area'][3] == 3.5
    assert s['border'].tolist()[8:10] == [0, 3] and s['feret_max'][6] == 7 and s['feret_min'][6] == 1
    assert 0 < s['eccentricity'][11] < 1 and 0.1 < abs(s['orientation'][11]) < 1.5
    kept = torch.arange(0, 12, dtype=torch.int64, device=DEV)
    feats = nuclei.shape_features(gpu(labels), kept, max_label=11)
    assert feats.dtype == torch.float32 and tuple(feats.shape) == (12, len(nuclei.SHAPE_FEATURE_NAMES))
    names = nuclei.SHAPE_FEATURE_NAMES
    assert feats[:, names.index('holes')].tolist()[1:] == [0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    assert feats[:, names.index('touches_border')].tolist() == [1] + [0] * 8 + [1, 0, 0]


def test_shape_features_on_tissue_beside_nucleus_features():
    labels, gray, within, top, want, want_w = tissue_case()
    L = gpu(labels)
    features, cen, kept = nuclei.nucleus_features(L, gpu(gray), max_label=top)
    got = nuclei.shape_features(L, kept, max_label=top)
    assert got.dtype == torch.float32 and tuple(got.shape) == (features.shape[0], len(nuclei.SHAPE_FEATURE_NAMES))
    w = ref.shape(want)
    table = ref.features(w)[kept.cpu().numpy()]
    w32 = table.astype(np.float32).astype(np.float64)
    names = nuclei.SHAPE_FEATURE_NAMES
    major = table[:, names.index('major_axis')]
    err = np.abs(got.cpu().numpy().astype(np.float64) - w32)
    for j, name in enumerate(names):
        bound = ULP * np.abs(w32[:, j]) + (ULP * major if name == 'minor_axis' else 0.0)
        assert (err[:, j] <= bound).all(), name
    for name in ('area', 'holes', 'touches_border'):                    # integer-valued columns: exact
        assert np.array_equal(got[:, names.index(name)].cpu().numpy(), table[:, names.index(name)].astype(np.float32)), name
    counts = np.bincount(labels.reshape(-1), minlength=top + 1)
    assert np.array_equal(got[:, 0].cpu().numpy(), counts[kept.cpu().numpy()].astype(np.float32))      # each row: its own label's pixels
    assert got[:, names.index('touches_border')].sum() >= 4             # synthetic_tissue cuts a nucleus on each side
    # int32 and int64 kept_labels, and with a domain
    assert torch.equal(nuclei.shape_features(L, kept.to(torch.int64), max_label=top), got)
    within_rows = nuclei.shape_features(L, kept, max_label=top, within=gpu(within))
    assert np.array_equal(within_rows[:, 0].cpu().numpy(), want_w['count'][kept.cpu().numpy()].astype(np.float32))


def test_the_touching_pair_gets_its_own_areas():
    m = two_discs()
    lab, n = nuclei.split_touching(gpu(m), 8)
    assert n == 2
    kept = torch.tensor([1, 2], dtype=torch.int32, device=DEV)
    got = nuclei.shape_features(lab, kept, max_label=n)
    own = np.bincount(lab.cpu().numpy().reshape(-1), minlength=3)
    assert got[:, 0].tolist() == [float(own[1]), float(own[2])] and own[1] + own[2] == int(m.sum())
    names = nuclei.SHAPE_FEATURE_NAMES
    assert got[:, names.index('holes')].tolist() == [0, 0] and got[:, names.index('touches_border')].tolist() == [0, 0]
    whole = nuclei.shape_features(gpu(m.astype(np.int32)), kept[:1], max_label=1)
    assert whole[0, 0] == float(m.sum()) > got[:, 0].max()              # one label over both: what a crop of foreground reports


# ------------------------------------------------------------------ clear_border
@pytest.mark.parametrize('ldtype', [torch.int32, torch.uint8, torch.int64])
def test_clear_border(ldtype):
    t, S = sizes()
    H, W = t + 6, t + 9
    labels = np.zeros((H, W), np.int32)
    labels[0:3, 10:14] = 4                                              # top
    labels[H - 2:, 20:23] = 9                                           # bottom
    labels[30:33, 0:2] = 2                                              # left
    labels[40:44, W - 1] = 12                                           # right
    labels[0, 0] = 7                                                    # a corner ...
    labels[H - 1, W - 1] = 15                                           # ... and the opposite one
    labels[5:9, 5:9] = 3                                                # interior ones stay
    labels[t - 2:t + 2, t - 2:t + 2] = 11
    labels[1:4, 30:33] = 6                                              # one pixel away from the frame
    labels[20, 20] = 4                                                  # a far piece of a cut label goes with it
    got = nuclei.clear_border(gpu(labels).to(ldtype))
    assert got.dtype == ldtype and tuple(got.shape) == (H, W)
    want = ref.clear_border(labels)
    assert np.array_equal(got.cpu().numpy().astype(np.int32), want)
    assert sorted(np.unique(want).tolist()) == [0, 3, 6, 11]            # nothing is renumbered
    assert torch.equal(nuclei.clear_border(gpu(labels).to(ldtype), max_label=20), got)
    labels2, _, _, top, _, _ = tissue_case()
    assert np.array_equal(nuclei.clear_border(gpu(labels2), max_label=top).cpu().numpy(), ref.clear_border(labels2))
    empty = torch.zeros(0, 4, dtype=torch.int32, device=DEV)
    assert tuple(nuclei.clear_border(empty).shape) == (0, 4)
