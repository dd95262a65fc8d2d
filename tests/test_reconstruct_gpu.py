"""Morphological reconstruction on the GPU (csrc/reconstruct.hip through cgc_net_amd.nuclei.reconstruct / h_maxima / regional_maxima /
fill_holes / split_touching(markers='h_maxima')) against tests/reconstruct_ref.py (the definition iterated in numpy; pinned to scipy
and to a brute-force path closure by tests/test_reconstruct_ref_cpu.py).  Every comparison is exact.

The kernel relaxes 64 x 64 tiles with a one-pixel halo, each thread scanning 16 pixels of a row, then of a column, in rounds that are
launches: the shapes sit under, on and one over one and two tiles in both directions, the staircases cross a tile corner diagonally,
and the serpentine needs more than a hundred rounds."""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, nuclei

import geodesic_ref
import reconstruct_ref as ref
from image_cases import DEV, gpu, tissue, two_discs
from test_geodesic_gpu import staircase

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 37), (41, 1), (7, 5), (63, 9), (64, 64), (65, 63), (64, 65), (5, 129), (129, 5), (130, 131), (200, 70)]
DTYPES = [torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32]
LOW, HIGH = ref.INT32_MIN, ref.INT32_MAX


def run(marker, mask, **kw):
    m = marker if torch.is_tensor(marker) else gpu(marker)
    k = mask if torch.is_tensor(mask) else gpu(mask)
    out = nuclei.reconstruct(m, k, **kw)
    assert out.dtype == m.dtype and out.device == m.device and tuple(out.shape) == tuple(m.shape) and out.is_contiguous()
    return out.cpu().numpy()


def check(marker, mask, method, connectivity):
    want = ref.reconstruct(marker, mask, method, connectivity)
    got = run(marker.astype(np.int32), mask.astype(np.int32), method=method, connectivity=connectivity)
    assert np.array_equal(got, want), (method, connectivity, np.argwhere(got != want)[:5])
    return got


def random_mask(rng, shape, kind):
    """int64 values in the int32 range: 'levels' = 3 levels in blobs (large plateaus), 'full' = the whole range with both ends."""
    if kind == 'levels':
        coarse = rng.randint(0, 3, size=(shape[0] // 5 + 2, shape[1] // 5 + 2))
        mask = np.kron(coarse, np.ones((5, 5), np.int64))[:shape[0], :shape[1]]
        flip = rng.rand(*shape) < 0.15
        return np.where(flip, rng.randint(0, 3, size=shape), mask).astype(np.int64)
    mask = rng.randint(LOW, HIGH + 1, size=shape, dtype=np.int64)
    mask.ravel()[rng.randint(mask.size)] = LOW
    mask.ravel()[rng.randint(mask.size)] = HIGH
    return mask


def random_marker(rng, mask, method, kind):
    """A sparse random subset of mask - k (dilation; mask + k for erosion), the neutral end of the range elsewhere."""
    k = rng.randint(0, 3, size=mask.shape) if kind == 'levels' else rng.randint(0, 2 ** 29, size=mask.shape)
    some = rng.rand(*mask.shape) < 0.03
    some.ravel()[rng.randint(mask.size)] = True
    if method == 'dilation':
        return np.where(some, np.maximum(mask - k, LOW), LOW)
    return np.where(some, np.minimum(mask + k, HIGH), HIGH)


# ------------------------------------------------------------------ tile geometry
@pytest.mark.parametrize('kind', ['levels', 'full'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_random_masks(shape, kind):
    rng = np.random.RandomState(31 * shape[0] + shape[1] + (kind == 'full'))
    for method in ('dilation', 'erosion'):
        for connectivity in (1, 2):
            mask = random_mask(rng, shape, kind)
            got = check(random_marker(rng, mask, method, kind), mask, method, connectivity)
            assert (got <= mask).all() if method == 'dilation' else (got >= mask).all()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_marker_cases(shape):
    rng = np.random.RandomState(7 * shape[0] + shape[1])
    for kind in ('levels', 'full'):
        mask = random_mask(rng, shape, kind)
        for connectivity in (1, 2):
            above = np.where(rng.rand(*shape) < 0.05, np.minimum(mask + rng.randint(1, 9, size=shape), HIGH), LOW)
            check(above, mask, 'dilation', connectivity)                                     # above the mask: clamped
            below = np.where(rng.rand(*shape) < 0.05, np.maximum(mask - rng.randint(1, 9, size=shape), LOW), HIGH)
            check(below, mask, 'erosion', connectivity)
            for method in ('dilation', 'erosion'):
                assert np.array_equal(check(mask, mask, method, connectivity), mask)         # marker == mask: the identity
            floor = np.full(shape, LOW, np.int64)
            assert np.array_equal(check(floor, mask, 'dilation', connectivity), floor)       # nothing to spread
            top = np.full(shape, HIGH, np.int64)
            assert np.array_equal(check(top, mask, 'dilation', connectivity), mask)          # everything clamped
            assert np.array_equal(check(top, mask, 'erosion', connectivity), top)


# ------------------------------------------------------------------ across tile corners
@pytest.mark.parametrize('anti', [False, True], ids=['main', 'anti'])
def test_staircase_across_a_tile_corner(anti):
    dom, path = staircase(anti)
    assert path[17] == ((63, 64) if anti else (63, 63)) and path[18] == ((64, 63) if anti else (64, 64))
    mask = np.where(dom, 100, 0).astype(np.int64)
    for end in (0, -1):
        marker = np.full(dom.shape, LOW, np.int64)
        marker[path[end]] = 50
        order = path if end == 0 else path[::-1]
        cut = 18 if end == 0 else len(path) - 18
        got = check(marker, mask, 'dilation', 2)
        assert np.array_equal(got == 50, dom) and (got[~dom] == 0).all()                     # conducted to the far end
        got = check(marker, mask, 'dilation', 1)
        reached = np.zeros_like(dom)
        for y, x in order[:cut]:
            reached[y, x] = True
        assert np.array_equal(got == 50, reached) and (got[~reached] == 0).all()             # stops at the pure corner contact
        got = check(~marker, ~mask, 'erosion', 2)                                            # the dual, upside down
        assert np.array_equal(got == ~np.int64(50), dom)


# ------------------------------------------------------------------ many rounds
def test_serpentine_needs_many_rounds():
    corridor = np.ones((130, 131), bool)
    for i, r in enumerate(range(1, 130, 2)):
        corridor[r, :] = False
        corridor[r, 130 if i % 2 == 0 else 0] = True
    seed = np.zeros_like(corridor)
    seed[0, 0] = True
    assert np.array_equal(ndimage.binary_propagation(seed, mask=corridor), corridor)         # one plateau, 65 passes long
    mask = np.where(corridor, 9, 0).astype(np.int32)
    marker = np.where(seed, 7, LOW).astype(np.int32)
    want = np.where(corridor, 7, 0)                                                          # every wall pixel touches the plateau
    m, k = gpu(marker), gpu(mask)
    first = nuclei.reconstruct(m, k)
    rounds = kernels.get().reconstruct_rounds
    second = nuclei.reconstruct(m, k)
    assert torch.equal(first, second) and np.array_equal(first.cpu().numpy(), want)
    assert rounds > 100                     # two tile edges per pass, 65 passes
    top = nuclei.reconstruct(k, k)          # already at the mask: every tile returns after its load
    assert torch.equal(top, k) and kernels.get().reconstruct_rounds == kernels.GEO_FIRST_BATCH


# ------------------------------------------------------------------ input forms
@functools.lru_cache(maxsize=None)
def form_case():
    rng = np.random.RandomState(13)
    mask = random_mask(rng, (70, 133), 'levels') * 40 + rng.randint(0, 3, size=(70, 133))      # 0 .. 82: fits every dtype but bool
    marker = np.where(rng.rand(70, 133) < 0.02, mask - rng.randint(0, 30, size=(70, 133)), 0).clip(0, None)
    return marker, mask


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_dtypes(dtype):
    marker, mask = form_case()
    if dtype == torch.bool:
        marker, mask = (marker > 40).astype(np.int64), (mask > 40).astype(np.int64)
    for mdt, kdt in ((dtype, dtype), (dtype, torch.int32), (torch.int32, dtype)):
        for method in ('dilation', 'erosion'):
            want = ref.reconstruct(marker, mask, method, 2)
            got = run(gpu(marker).to(mdt), gpu(mask).to(kdt), method=method, connectivity=2)
            assert np.array_equal(got.astype(np.int64), want), (mdt, kdt, method)


def test_views():
    marker, mask = form_case()
    mt, kt = gpu(marker.astype(np.int32)).t(), gpu(mask.astype(np.int16)).t()
    assert not mt.is_contiguous()
    assert np.array_equal(run(mt, kt), ref.reconstruct(marker.T, mask.T))
    wide_m = gpu(np.repeat(np.repeat(marker.astype(np.int16), 2, axis=0), 3, axis=1))[::2, ::3]
    wide_k = gpu(np.repeat(np.repeat(mask.astype(np.uint8), 2, axis=0), 3, axis=1))[::2, ::3]
    assert not wide_m.is_contiguous() and tuple(wide_m.shape) == marker.shape
    assert np.array_equal(run(wide_m, wide_k, method='erosion'), ref.reconstruct(marker, mask, 'erosion'))
    assert np.array_equal(wide_m.cpu().numpy(), marker)                                      # the inputs are left alone


def test_empty_images():
    for shape in ((0, 5), (4, 0), (0, 0)):
        for dtype in (torch.bool, torch.int16):
            t = torch.zeros(shape, dtype=dtype, device=DEV)
            for out in (nuclei.reconstruct(t, t), nuclei.reconstruct(t, t, 'erosion', 2), nuclei.fill_holes(t)):
                assert tuple(out.shape) == shape and out.dtype == dtype
            for out in (nuclei.h_maxima(t, 3), nuclei.regional_maxima(t, 2)):
                assert tuple(out.shape) == shape and out.dtype == torch.bool
        lab, n = nuclei.split_touching(torch.zeros(shape, dtype=torch.uint8, device=DEV), None, growth='geodesic', markers='h_maxima', h=1)
        assert tuple(lab.shape) == shape and lab.dtype == torch.int32 and n == 0


# ------------------------------------------------------------------ h_maxima
def two_peaks(saddle):
    """A plateau of 20 (2 x 3 pixels) and one of 30 (3 x 2) on a floor of 0, joined by a one-pixel-wide ridge at ``saddle``."""
    img = np.zeros((70, 90), np.int32)
    img[10:12, 5:8] = 20
    img[60:63, 80:82] = 30
    img[11, 8:81] = saddle
    img[11:60, 80] = saddle
    return img


@pytest.mark.parametrize('connectivity', [1, 2])
def test_h_maxima_counts_the_dynamic(connectivity):
    h = 6
    for dynamic in (h - 1, h, h + 1):
        img = two_peaks(20 - dynamic)
        got = nuclei.h_maxima(gpu(img), h, connectivity)
        assert got.dtype == torch.bool and got.is_contiguous()
        got = got.cpu().numpy()
        assert np.array_equal(got, ref.h_maxima(img, h, connectivity))
        assert np.array_equal(got, (img == 30) | ((img == 20) & (dynamic >= h)))             # whole summit plateaus, nothing else
    img = two_peaks(12)
    for hh in (9, 30, 31, HIGH):                                                             # above max - min too: the highest summit stays
        assert np.array_equal(nuclei.h_maxima(gpu(img), hh, connectivity).cpu().numpy(), img == 30)
    low = img + (LOW + 5)                                                                    # 35 above the int32 minimum at most
    for hh in (36, 1000, HIGH):                                                              # h larger than that range: all False
        got = nuclei.h_maxima(gpu(low), hh, connectivity)
        assert not got.any() and not ref.h_maxima(low, hh, connectivity).any()
    assert np.array_equal(nuclei.h_maxima(gpu(low), 35, connectivity).cpu().numpy(), img == 30)
    for dtype in (torch.uint8, torch.int8, torch.int16):
        assert np.array_equal(nuclei.h_maxima(gpu(img).to(dtype), 8, connectivity).cpu().numpy(), ref.h_maxima(img, 8, connectivity))
    ends = np.array([[LOW, LOW + 3, LOW, HIGH, HIGH - 2, HIGH]], np.int32)                   # image - h saturates at the floor
    for hh in (1, 2, 3, 4, HIGH):
        assert np.array_equal(nuclei.h_maxima(gpu(ends), hh, connectivity).cpu().numpy(), ref.h_maxima(ends, hh, connectivity))


@pytest.mark.parametrize('kind', ['levels', 'full'])
@pytest.mark.parametrize('shape', [(1, 37), (41, 1), (65, 63), (130, 131)], ids=lambda s: '%dx%d' % s)
def test_regional_maxima(shape, kind):
    rng = np.random.RandomState(3 * shape[0] + shape[1])
    img = random_mask(rng, shape, kind)
    for connectivity in (1, 2):
        got = nuclei.regional_maxima(gpu(img.astype(np.int32)), connectivity).cpu().numpy()
        assert np.array_equal(got, ref.regional_maxima(img, connectivity))
        if kind == 'levels':
            assert np.array_equal(got, ref.plateau_maxima(img, connectivity))
        else:                               # no two neighbours are equal: a maximum is a pixel above all of its neighbours
            assert np.array_equal(got, ndimage.maximum_filter(img, footprint=ref.FOOTPRINTS[connectivity], mode='nearest') == img)
    flat = torch.full(shape, 5, dtype=torch.int8, device=DEV)
    assert nuclei.regional_maxima(flat).all()


# ------------------------------------------------------------------ fill_holes
def rings():
    """bool [150, 160]: a ring, a ring nested in a ring with a dot in the middle, a ring whose hole opens to the outside through a
    one-pixel diagonal gap, a ring across a tile corner, and a half ring whose hole touches the image border."""
    img = np.zeros((150, 160), bool)
    yy, xx = np.mgrid[0:150, 0:160]

    def ring(cy, cx, r0, r1):
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        return (d2 <= r1 * r1) & (d2 >= r0 * r0)

    img |= ring(20, 20, 8, 11)
    img |= ring(30, 110, 25, 28) | ring(30, 110, 12, 15) | ring(30, 110, 0, 2)
    img |= ring(64, 64, 6, 9)
    img |= ring(110, 0, 10, 13)                                                              # cut by the left border: no hole
    img[100:121, 60:81] = True
    img[101:120, 61:80] = False                                                              # a square ring ...
    img[100, 60] = False                                                                     # ... without its corner pixel
    return img


@pytest.mark.parametrize('connectivity', [1, 2])
def test_fill_holes_rings(connectivity):
    img = rings()
    got = nuclei.fill_holes(gpu(img), connectivity)
    assert got.dtype == torch.bool and got.is_contiguous()
    got = got.cpu().numpy()
    assert np.array_equal(got, ndimage.binary_fill_holes(img, structure=ref.FOOTPRINTS[connectivity]))
    assert np.array_equal(got, ref.fill_holes(img, connectivity))
    assert got[30, 110 - 20] and got[30, 110 - 8] and got[20, 20] and got[64, 64]             # between the nested rings too
    assert not got[110, 2]                                                                   # open to the border
    assert got[110, 70] == (connectivity == 1)                                               # the diagonal gap conducts for 8 neighbours
    assert (got | ~img).all() and not got[0].any()


@functools.lru_cache(maxsize=None)
def tissue_holes():
    labels, _, _ = tissue()
    return {c: ref.fill_holes(labels, c) for c in (1, 2)}


@pytest.mark.parametrize('connectivity', [1, 2])
def test_fill_holes_tissue(connectivity):
    labels, _, _ = tissue()
    m = labels > 0
    got = nuclei.fill_holes(gpu(m), connectivity).cpu().numpy()
    want = ndimage.binary_fill_holes(m, structure=ref.FOOTPRINTS[connectivity])
    assert np.array_equal(got, want) and (want & ~m).any()
    filled = nuclei.fill_holes(gpu(labels), connectivity)
    assert filled.dtype == torch.int32
    filled = filled.cpu().numpy()
    assert np.array_equal(filled, tissue_holes()[connectivity])
    assert np.array_equal(filled[labels != 0], labels[labels != 0])                          # labels never lose a pixel
    assert np.array_equal(filled != 0, want)                                                 # exactly the holes are filled
    small = nuclei.fill_holes(gpu(labels.astype(np.int16)), connectivity)
    assert small.dtype == torch.int16 and np.array_equal(small.cpu().numpy(), filled)


def test_fill_holes_of_instance_masks():
    yy, xx = np.mgrid[0:80, 0:100]
    d2 = (yy - 40) ** 2 + (xx - 64) ** 2
    ring = np.where((d2 <= 30 * 30) & (d2 >= 22 * 22), 7, 0).astype(np.uint8)                # one label: closes with that label
    got = nuclei.fill_holes(gpu(ring))
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), np.where(d2 <= 30 * 30, 7, 0))
    two = np.zeros((80, 140), np.int32)
    two[10:70, 10:70], two[10:70, 70:130] = 3, -8                                            # a negative label is a label
    two[30:50, 40:100] = 0                                                                   # one hole between two labels
    got = nuclei.fill_holes(gpu(two)).cpu().numpy()
    assert np.array_equal(got, ref.fill_holes(two))
    assert (got[30:50, 40:70] == 3).all() and (got[30:50, 70:100] == -8).all()               # shared along the geodesic midline
    assert np.array_equal(got[two != 0], two[two != 0]) and (got[:10] == 0).all() and (got[:, 130:] == 0).all()


# ------------------------------------------------------------------ split_touching(markers='h_maxima')
def split_h(mask, h, connectivity=1, min_size=0):
    lab, n = nuclei.split_touching(gpu(mask), None, connectivity, min_size, growth='geodesic', markers='h_maxima', h=h)
    assert type(n) is int and lab.dtype == torch.int32
    return lab.cpu().numpy(), n


def test_distance_in_eighths():
    labels, _, _ = tissue()
    d2 = nuclei.distance_transform(gpu(labels > 0))
    assert np.array_equal(nuclei._eighths(d2).cpu().numpy(), ref.eighths(d2.cpu().numpy()))


@pytest.mark.parametrize('h,connectivity,min_size', [(0.5, 1, 0), (1, 1, 10), (2, 2, 0)])
def test_split_h_maxima_tissue(h, connectivity, min_size):
    labels, _, _ = tissue()
    m = labels > 0
    got, n = split_h(m, h, connectivity, min_size)
    want, wn = ref.split_touching_h_maxima(m, h, connectivity, min_size)
    assert n == wn and np.array_equal(got, want), (n, wn, np.argwhere(got != want)[:5])
    if min_size == 0:
        assert np.array_equal(got != 0, m)                                                   # every mask pixel is labelled


def test_split_h_maxima_two_discs():
    m = two_discs()
    for h in (1, 2.5, 40):                  # two equal summits (80 eighths over a saddle of 64): neither has a higher pixel, both stay
        got, n = split_h(m, h)
        want, wn = ref.split_touching_h_maxima(m, h)
        assert n == wn == 2 and np.array_equal(got, want) and np.array_equal(got != 0, m)
        assert got[24, 17] != got[24, 31] and (got[:, :24] == got[24, 17])[m[:, :24]].all()  # cut on the midline
    assert split_h(m, 1, 2)[1] == 2


def unequal_discs():
    """A disc of radius 20 and one of radius 7 whose centres are 24 apart: they overlap by three pixels.  On the reference the
    distance map has the summits 20 and 7 pixels and the saddle 6 pixels: a core radius below 6 merges the two, one of 7 or more
    (what two_discs needs is 8) loses the small disc's core, and the small summit's dynamic is one pixel."""
    yy, xx = np.mgrid[0:64, 0:72]
    big = (yy - 32) ** 2 + (xx - 26) ** 2 <= 20 * 20
    small = (yy - 32) ** 2 + (xx - 50) ** 2 <= 7 * 7
    return big, small


def test_h_maxima_separates_what_one_core_radius_cannot():
    big, small = unequal_discs()
    m = big | small
    both = np.concatenate([np.pad(m, ((0, 0), (0, 8))), np.pad(two_discs(), ((0, 16), (0, 32)))], axis=0)      # [128, 80]: four nuclei
    # the reference first: this is where the radii come from
    for radius in (4, 8):
        lab, n = geodesic_ref.split_touching_geodesic(m, radius)
        assert n == 1                                                                        # merged (4) / the small core is lost (8)
    lab, n = ref.split_touching_h_maxima(m, 0.5)
    assert n == 2 and lab[32, 26] != lab[32, 50] and min(np.bincount(lab.ravel())[1:]) >= small.sum()
    assert all(geodesic_ref.split_touching_geodesic(both, radius)[1] != 4 for radius in range(1, 13))
    assert ref.split_touching_h_maxima(both, 0.5)[1] == 4
    # the same on the GPU
    for radius in (4, 8):
        core, n = nuclei.split_touching(gpu(m), radius, growth='geodesic')
        assert n == 1 and np.array_equal(core.cpu().numpy(), geodesic_ref.split_touching_geodesic(m, radius)[0])
    got, n = split_h(m, 0.5)
    assert n == 2 and np.array_equal(got, lab) and got[32, 26] != got[32, 50] and np.array_equal(got != 0, m)
    assert split_h(m, 1.5)[1] == ref.split_touching_h_maxima(m, 1.5)[1] == 1                 # the small summit stands one pixel above the saddle
    assert all(nuclei.split_touching(gpu(both), radius, growth='geodesic')[1] != 4 for radius in range(1, 13))
    got, n = split_h(both, 0.5)
    assert n == 4 and np.array_equal(got, ref.split_touching_h_maxima(both, 0.5)[0])
    assert len({got[32, 26], got[32, 50], got[64 + 24, 17], got[64 + 24, 31]}) == 4         # one label per disc centre


def test_split_h_maxima_feeds_nucleus_features():
    labels, gray, _ = tissue()
    lab, n = nuclei.split_touching(gpu(labels > 0), None, min_size=10, growth='geodesic', markers='h_maxima', h=1)
    feats, cen, kept = nuclei.nucleus_features(lab, gpu(gray), max_label=n)
    assert tuple(feats.shape) == (n, nuclei.NUM_FEATURES) and np.array_equal(kept.cpu().numpy(), np.arange(1, n + 1))


# ------------------------------------------------------------------ defaults untouched, argument errors
def test_core_markers_are_the_default():
    labels, _, _ = tissue()
    m = gpu(labels > 0)
    for growth in ('euclidean', 'geodesic'):
        lab, n = nuclei.split_touching(m, 3, 1, 10, growth)
        same, sn = nuclei.split_touching(m, 3, 1, 10, growth, markers='core')
        assert n == sn and torch.equal(lab, same)
    want, wn = geodesic_ref.split_touching_geodesic(labels > 0, 3, 1, 10)
    assert n == wn and np.array_equal(lab.cpu().numpy(), want)


def test_argument_errors():
    ok = torch.zeros(8, 9, dtype=torch.int16, device=DEV)
    calls = (lambda t, **kw: nuclei.reconstruct(t, t, **kw), lambda t, **kw: nuclei.h_maxima(t, 2, **kw),
             lambda t, **kw: nuclei.regional_maxima(t, **kw), lambda t, **kw: nuclei.fill_holes(t, **kw))
    for fn in calls:
        for bad in (ok.cpu(), ok.cpu().numpy(), ok.long(), ok.float()):
            with pytest.raises(TypeError):
                fn(bad)
        with pytest.raises(ValueError):
            fn(ok[None])
        with pytest.raises(ValueError):
            fn(ok, connectivity=3)
    with pytest.raises(ValueError):
        nuclei.reconstruct(ok, ok.t())
    with pytest.raises(TypeError):
        nuclei.reconstruct(ok, ok.long())
    with pytest.raises(ValueError):
        nuclei.reconstruct(ok, ok, method='opening')
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            nuclei.reconstruct(ok, ok.to('cuda:1'))
    for bad in (0, -3, 2 ** 31):
        with pytest.raises(ValueError):
            nuclei.h_maxima(ok, bad)
    with pytest.raises(TypeError):
        nuclei.h_maxima(ok, 1.5)
    for kw in (dict(markers='h_maxima', h=1), dict(growth='geodesic', markers='h_maxima'), dict(growth='geodesic', markers='h_maxima', h=0.1),
               dict(markers='peaks'), dict(h=1), dict(growth='geodesic', h=1)):
        with pytest.raises(ValueError):
            nuclei.split_touching(ok, 2, **kw)
    with pytest.raises(ValueError):
        kernels.get().morph_reconstruct(ok.int(), ok.int(), 4)
